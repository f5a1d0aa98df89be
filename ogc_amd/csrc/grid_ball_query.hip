// grid_ball_query.hip — the fixed-radius query of a cloud in itself over the cell lists of grid.hip, with the rows of the
// reference's index-ordered scan (ball_query_gpu.cu:9-45):
//   ball_query_grid     one LANE PER CANDIDATE: a wavefront takes eight centres consecutive in cell order, deals the
//                       candidates of the union of their neighbourhoods (nine contiguous runs) to its 64 lanes and
//                       tests every centre against all lanes at once (centre coordinates as scalars, two centres per
//                       packed instruction); ballots turn hits into list slots; eight lanes per centre rank-sort the
//                       list by point index -> first nsample, padded with the first: the row the reference produces
//                       by scanning in index order and stopping after nsample hits;
//   ball_query_cells    four lanes per centre for the usual row lengths of sparse neighbourhoods.
#include <stdlib.h>

#include "grid_dev.h"

namespace ogc_grid {

// Ball query of a cloud against itself over the cell lists: ONE LANE PER CANDIDATE.
// A wavefront takes eight centres that are consecutive in cell order.  Centres on the same (y, z) row of cells form a
// batch (usually the whole wavefront is one batch); the union of their 27-cell neighbourhoods is a box of nine
// contiguous runs, whose candidates are dealt to the 64 lanes (16-byte records, one load each).  Each centre of the
// batch is then tested by all lanes at once — its coordinates are wave-uniform scalars, two centres per packed
// instruction, the squared distance is the reference's fp32 expression — and one ballot turns the hits into
// consecutive slots of the centre's hit list (hit counts live in scalar registers).  Testing a candidate outside a
// centre's own 27 cells is harmless (the distance decides), so the box needs no per-centre bookkeeping.
// Finish: eight lanes per centre rank-sort the hit list by point index (indices are distinct), keep the first
// nsample, pad with the smallest, 16-byte stores — the row the reference produces by scanning in index order and
// stopping after nsample hits.  A centre with more hits than the list holds is redone through an LDS bitmap over
// point indices (set a bit per hit, read the first nsample set bits), also exact.
// Clouds flagged dense by the build (the 27 cells hold a large share of the cloud, so cell lists buy nothing and
// rows saturate early) are scanned in INDEX order instead, by the same wavefronts: hits then arrive in the order
// of the output and a wavefront stops as soon as its eight rows are full.
// (the body of the kernel: ball_query_cells_kernel below runs it too, for the wavefronts its short lists cannot hold)
__device__ __forceinline__ void ball_query_grid_body(int lane, int first_centre, int *gq_smem, int n, int m, float radius2, int nsample,
                                                     int hit_cap, int stride_cells, const float *__restrict__ xyz,
                                                     const GridHdr *__restrict__ hdrs, const int *__restrict__ cell_start,
                                                     const float4 *__restrict__ sorted_pts, int *__restrict__ idx_out) {
    const int b = blockIdx.y;
    OGC_PROBE_T(pt0);
    const GridHdr h = hdrs[b];
    int *hits = gq_smem;                                       // [QPW][hit_cap]
    int *outr = gq_smem + QPW * hit_cap;                       // [QPW][nsample] sorted rows
    unsigned *bitmap = reinterpret_cast<unsigned *>(outr + QPW * nsample); // [ceil(n / 32)], overflow path only
    const int *cs = cell_start + (size_t)b * stride_cells;
    const float4 *pts = sorted_pts + (size_t)b * n;

    // every group of eight lanes holds the eight centres (lane & 7), so 8-lane butterflies see the whole set
    const int pc = first_centre + (lane & (QPW - 1));
    float4 me = make_float4(NAN, NAN, NAN, __int_as_float(-1));
    if (pc < n) me = pts[pc]; // positions >= h.npts hold the non-finite points: no hits, an all-zero row
    const bool live = pc < h.npts;
    int cnt_s[QPW]; // wave-uniform hit counts (may exceed hit_cap)
#pragma unroll
    for (int c = 0; c < QPW; ++c) cnt_s[c] = 0;
    unsigned sorted_rows = 0; // rows written in ascending order already (index-order scan, bitmap path)
    int box_total, b0, s1, b1, s2, b2, s3, b3, s4, b4, s5, b5, s6, b6, s7, b7, s8, b8;
    const unsigned live_mask = (unsigned)__builtin_amdgcn_ballot_w64(live) & 0xFFu;

    if (h.dense) {
        // ---- index-order scan of the whole cloud: rows come out sorted, stop when all rows are full
        const float *src = xyz + (size_t)b * n * 3;
        sorted_rows = 0xFFu;
        for (int f0 = 0; f0 < n; f0 += OGC_WAVE) {
            const int f = f0 + lane;
            float x = NAN, y = NAN, z = NAN;
            if (f < n) { x = src[f * 3]; y = src[f * 3 + 1]; z = src[f * 3 + 2]; }
            bool all_full = true;
#pragma unroll
            for (int c = 0; c < QPW; c += 2) {
                if (!((live_mask >> c) & 3u)) continue;
                const ogc_v2f qx = {lane_bcast(me.x, c), lane_bcast(me.x, c + 1)};
                const ogc_v2f qy = {lane_bcast(me.y, c), lane_bcast(me.y, c + 1)};
                const ogc_v2f qz = {lane_bcast(me.z, c), lane_bcast(me.z, c + 1)};
                const ogc_v2f d = sqdist_pair(qx, qy, qz, x, y, z);
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    if (cnt_s[c + u] >= nsample) continue;
                    const bool hit = (u == 0 ? d.x : d.y) < radius2;
                    const unsigned long long mask = __builtin_amdgcn_ballot_w64(hit);
                    if (mask != 0) {
                        if (hit) {
                            const int slot = cnt_s[c + u] + (int)__builtin_amdgcn_mbcnt_hi(
                                (unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
                            if (slot < nsample) outr[(c + u) * nsample + slot] = f;
                        }
                        cnt_s[c + u] += __popcll(mask);
                    }
                    if (cnt_s[c + u] < nsample && ((live_mask >> (c + u)) & 1u)) all_full = false;
                }
            }
            if (all_full) break;
        }
    } else {
        OGC_GRID_AXES(h, me.x, me.y, me.z, fx, fy, fz);
        const int cx = cell_coord(fx, h.minx, h.inv_h, h.gx);
        const int cy = cell_coord(fy, h.miny, h.inv_h, h.gy);
        const int cz = cell_coord(fz, h.minz, h.inv_h, h.gz);
        const bool slab = h.slab != 0;
        const int cr = slab ? cy : cx, gr = slab ? h.gy : h.gx; // the coordinate a batch's box ranges over
        unsigned todo = live_mask;
        while (todo != 0) {
            const int c0 = __ffs(todo) - 1;
            const int y0 = lane_bcast(cy, c0), z0 = lane_bcast(cz, c0);
            const bool mine = live && (slab || cy == y0) && cz == z0; // (slab: a batch is the centres of one z)
            const unsigned batch = (unsigned)__builtin_amdgcn_ballot_w64(mine) & todo;
            todo &= ~batch;
            int xlo = mine ? cr : 0x7fffffff, xhi = mine ? cr : -1;
#pragma unroll
            for (int off = 1; off < QPW; off <<= 1) {
                xlo = min(xlo, __shfl_xor(xlo, off, 64));
                xhi = max(xhi, __shfl_xor(xhi, off, 64));
            }
            const int bx0 = max(lane_bcast(xlo, 0) - 1, 0), bx1 = min(lane_bcast(xhi, 0) + 1, gr - 1);
            OGC_BOX_SETUP(slab, bx0, bx1, y0, z0)
            const float4 nothing = make_float4(NAN, NAN, NAN, 0.0f); // NaN: never a hit
            float4 ahead = nothing; // the next round's candidate is in flight while this round is tested
            if (lane < box_total) ahead = pts[OGC_BOX_POSITION(lane)];
            for (int f0 = 0; f0 < box_total; f0 += OGC_WAVE) {
                const float4 cand = ahead;
                const int fn = f0 + OGC_WAVE + lane;
                ahead = nothing;
                if (fn < box_total) ahead = pts[OGC_BOX_POSITION(fn)];
                const int v = __float_as_int(cand.w);
#pragma unroll
                for (int c = 0; c < QPW; c += 2) {
                    if (!((batch >> c) & 3u)) continue; // wave-uniform
                    const ogc_v2f qx = {lane_bcast(me.x, c), lane_bcast(me.x, c + 1)};
                    const ogc_v2f qy = {lane_bcast(me.y, c), lane_bcast(me.y, c + 1)};
                    const ogc_v2f qz = {lane_bcast(me.z, c), lane_bcast(me.z, c + 1)};
                    const ogc_v2f d = sqdist_pair(qx, qy, qz, cand.x, cand.y, cand.z);
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        if (!((batch >> (c + u)) & 1u)) continue;
                        const bool hit = (u == 0 ? d.x : d.y) < radius2;
                        const unsigned long long mask = __builtin_amdgcn_ballot_w64(hit);
                        if (mask == 0) continue;
                        if (hit) {
                            const int slot = cnt_s[c + u] + (int)__builtin_amdgcn_mbcnt_hi(
                                (unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
                            if (slot < hit_cap) hits[(c + u) * hit_cap + slot] = v;
                        }
                        cnt_s[c + u] += __popcll(mask);
                    }
                }
            }
        }
    }
    OGC_PROBE_T(pt1);
    // hit counts: lane c < 8 holds the count of centre c
    int cnt = 0;
#pragma unroll
    for (int c = 0; c < QPW; ++c) cnt = lane == c ? cnt_s[c] : cnt;
    if (h.dense) cnt = min(cnt, nsample);

    // centres whose hit list overflowed: exact redo through a bitmap over point indices
    unsigned over = h.dense ? 0u : (unsigned)__builtin_amdgcn_ballot_w64(lane < QPW && cnt > hit_cap);
    while (over != 0) {
        const int c = __ffs(over) - 1;
        over &= over - 1;
        sorted_rows |= 1u << c;
        const int words = (n + 31) >> 5;
        for (int w = lane; w < words; w += OGC_WAVE) bitmap[w] = 0u;
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
        const float qx = lane_bcast(me.x, c), qy = lane_bcast(me.y, c), qz = lane_bcast(me.z, c);
        OGC_GRID_AXES(h, qx, qy, qz, gfx_, gfy_, gfz_);
        const int ccx = cell_coord(gfx_, h.minx, h.inv_h, h.gx);
        const int ccy = cell_coord(gfy_, h.miny, h.inv_h, h.gy);
        const int ccz = cell_coord(gfz_, h.minz, h.inv_h, h.gz);
        const bool slab_o = h.slab != 0;
        const int bx0 = max((slab_o ? ccy : ccx) - 1, 0), bx1 = min((slab_o ? ccy : ccx) + 1, (slab_o ? h.gy : h.gx) - 1);
        OGC_BOX_SETUP(slab_o, bx0, bx1, ccy, ccz)
        for (int f0 = 0; f0 < box_total; f0 += OGC_WAVE) {
            const int f = f0 + lane;
            if (f < box_total) {
                const float4 cand = pts[OGC_BOX_POSITION(f)];
                if (ogc_sqdist(qx, qy, qz, cand.x, cand.y, cand.z) < radius2) {
                    const unsigned v = (unsigned)__float_as_int(cand.w);
                    atomicOr(&bitmap[v >> 5], 1u << (v & 31u));
                }
            }
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
        int found = 0;
        for (int w0 = 0; w0 < words && found < nsample; w0 += OGC_WAVE) {
            const int w = w0 + lane;
            unsigned bits = w < words ? bitmap[w] : 0u;
            const int pcn = __popc(bits);
            int incl = pcn;
#pragma unroll
            for (int off = 1; off < OGC_WAVE; off <<= 1) {
                const int up = __shfl_up(incl, off, 64);
                if (lane >= off) incl += up;
            }
            int pos = found + incl - pcn;
            while (bits != 0u && pos < nsample) {
                outr[c * nsample + pos] = (w << 5) + (__ffs(bits) - 1);
                bits &= bits - 1u;
                ++pos;
            }
            found += lane_bcast(incl, OGC_WAVE - 1);
        }
        if (lane == c) cnt = min(found, nsample);
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();

    OGC_PROBE_T(pt2);
    // finish: eight lanes per centre
    const int sub = lane & (SUB - 1), qi = lane >> 3;
    const int total_hits = __shfl(cnt, qi, 64);
    const int q = __float_as_int(__shfl(me.w, qi, 64));
    int *row = outr + qi * nsample;
    if (!((sorted_rows >> qi) & 1u)) {
        // rank sort (the indices are distinct): element e goes to position #{f : hits[f] < hits[e]}
        const int *mine_hits = hits + qi * hit_cap;
        for (int e = sub; e < total_hits; e += SUB) {
            const int ve = mine_hits[e];
            int rank = 0;
            for (int f = 0; f < total_hits; ++f) rank += mine_hits[f] < ve ? 1 : 0;
            if (rank < nsample) row[rank] = ve;
        }
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
    OGC_PROBE_T(pt3);
    if (q >= 0) {
        const int kept = min(total_hits, nsample);
        const int first = kept > 0 ? row[0] : 0;
        int *o = idx_out + ((size_t)b * m + q) * nsample;
        if ((nsample & 3) == 0) { // 16-byte stores
            for (int j = sub * 4; j < nsample; j += SUB * 4) {
                int4 val;
                val.x = j < kept ? row[j] : first;
                val.y = j + 1 < kept ? row[j + 1] : first;
                val.z = j + 2 < kept ? row[j + 2] : first;
                val.w = j + 3 < kept ? row[j + 3] : first;
                *reinterpret_cast<int4 *>(o + j) = val;
            }
        } else {
            for (int j = sub; j < nsample; j += SUB) o[j] = j < kept ? row[j] : first;
        }
    }
    OGC_PROBE_T(pt4);
    OGC_PROBE_ADD(16, pt0, pt1);
    OGC_PROBE_ADD(17, pt1, pt2);
    OGC_PROBE_ADD(18, pt2, pt3);
    OGC_PROBE_ADD(19, pt3, pt4);
}

__global__ __launch_bounds__(OGC_WAVE) void ball_query_grid_kernel(int n, int m, float radius2, int nsample,
                                                                   int hit_cap, int stride_cells,
                                                                   const float *__restrict__ xyz,
                                                                   const GridHdr *__restrict__ hdrs,
                                                                   const int *__restrict__ cell_start,
                                                                   const float4 *__restrict__ sorted_pts,
                                                                   int *__restrict__ idx_out) {
    extern __shared__ __attribute__((aligned(16))) int gq_smem[];
    ball_query_grid_body(threadIdx.x, blockIdx.x * QPW, gq_smem, n, m, radius2, nsample, hit_cap, stride_cells, xyz, hdrs, cell_start,
                         sorted_pts, idx_out);
}

// ---- the same query with FOUR lanes per centre, for sparse neighbourhoods -----------------------------------------------
// ball_query_grid_kernel deals the candidates of eight centres' common box to the 64 lanes and tests every centre against
// every lane: with the ~60 candidates and 12 hits per centre of the loss's shape (8192 points in 60 x 4 x 80, r = 2) most
// of its ~780 vector instructions per wavefront are bookkeeping — nine-run position lookups, a ballot, a scalar branch and
// a slot computation per (centre, round), scalar broadcasts of the centres, a quadratic rank sort through LDS.  Here a
// wavefront takes SIXTEEN centres consecutive in cell order and each gets four lanes, which walk the centre's own nine
// runs (the three cells around it in x of each of the 3 x 3 rows): lane s tests candidates s and s + 4 of a run with one
// packed distance, a hit's list slot is a population count over the group's bits of the two ballots, and a miss is
// stored to a spare slot instead of branching.  Lists of up to BQ_FAST hits are then sorted IN REGISTERS by a bitonic
// network over 4 lanes x 8 keys (exchanges at distance < 8 inside a lane, the others by quad permutations) and the
// rows leave straight from the registers — no loop, no LDS round trip after two reads.  The rows are those of the
// reference's index-ordered scan, as with the other kernel.  A wavefront with a longer list, and every wavefront of a
// cloud the build flagged dense or heavy, runs the general body above (twice: eight centres each).
#ifndef OGC_BQ_MINWAVES
#define OGC_BQ_MINWAVES 8   // wavefronts per SIMD the register budget leaves room for (tools/bq_probe.hip builds variants)
#endif
template <int NS, int WPB>
__global__ __launch_bounds__(OGC_WAVE * WPB, OGC_BQ_MINWAVES) void ball_query_cells_kernel(int n, int m, float radius2, int stride_cells, int lds_ints,
                                                                       const float *__restrict__ xyz,
                                                                       const GridHdr *__restrict__ hdrs,
                                                                       const int *__restrict__ cell_start,
                                                                       const float4 *__restrict__ sorted_pts,
                                                                       int *__restrict__ idx_out) {
    extern __shared__ __attribute__((aligned(16))) int gq_smem_all[];
    // WPB independent wavefronts per workgroup (nothing is shared between them: a workgroup is only the unit of dispatch)
    const int lane = threadIdx.x & (OGC_WAVE - 1), wave_in_block = threadIdx.x >> 6;
    const int grp = blockIdx.x * WPB + wave_in_block; // sixteen centres
    int *gq_smem = gq_smem_all + wave_in_block * lds_ints;
    const int b = blockIdx.y, sub = lane & (CL - 1), g = lane >> 2;
    OGC_PROBE_T(pt0);
    const GridHdr h = hdrs[b];
    bool general = h.dense != 0 || h.heavy != 0;
    if (!general) {
        const int *cs = cell_start + (size_t)b * stride_cells;
        const float4 *pts = sorted_pts + (size_t)b * n;
        const int pc = grp * CPW + g;
        float4 me = make_float4(NAN, NAN, NAN, __int_as_float(-1));
        if (pc < n) me = pts[pc]; // positions >= h.npts hold the non-finite points: no hits, an all-zero row
        const bool live = pc < h.npts;
        int *mine = gq_smem + g * BQ_LIST; // the centre's strip
        int *seg = mine + sub * BQ_SEG;    // my own hit slots
        {   // every slot starts as +inf: the sort reads the first eight of each lane whatever was found
            const int4 inf4 = make_int4(0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff);
            int4 *l4 = reinterpret_cast<int4 *>(seg);
#pragma unroll
            for (int i = 0; i < 4; ++i) l4[i] = inf4;
        }
        // the centre's cell, as the build computed it (a live centre is finite: the conversion saturates where cell_coord
        // clamps, and the clamp to the grid follows either way)
        OGC_GRID_AXES(h, me.x, me.y, me.z, gfx, gfy, gfz);
        const int cx = min(cell_floor(gfx, h.minx, h.inv_h), h.gx - 1);
        const int cy = min(cell_floor(gfy, h.miny, h.inv_h), h.gy - 1);
        const int cz = min(cell_floor(gfz, h.minz, h.inv_h), h.gz - 1);
        const int x0 = max(cx - 1, 0), x1 = min(cx + 1, h.gx - 1);
        const bool slab = h.slab != 0; // (wave-uniform)
        // run r = the cells x0 .. x1 of row (cy + r % 3 - 1, cz + r / 3 - 1): lane s fetches runs s and s + 4, all fetch run 8
        // (no branch around the loads and all six in flight together: rows outside the grid read a clamped row and get
        // length 0 afterwards).  Slab grids: run r < 3 = the cells (any x, cy - 1 .. cy + 1) of z = cz + r - 1, lane s fetches run s.
        auto row_of = [&](int r, bool &inside) {
            const int r3 = r / 3;
            const int y = cy + (r - 3 * r3) - 1, z = cz + r3 - 1;
            inside = live && y >= 0 && y < h.gy && z >= 0 && z < h.gz;
            return h.gx * (min(max(y, 0), h.gy - 1) + h.gy * min(max(z, 0), h.gz - 1));
        };
        bool in_a, in_b, in_c;
        int row_a = row_of(sub, in_a), row_b = row_of(sub + 4, in_b), row_c = row_of(8, in_c);
        int first_a = row_a + x0, last_a = row_a + x1 + 1;
        if (slab) {
            const int z = cz + sub - 1;
            in_a = live && sub < 3 && z >= 0 && z < h.gz;
            const int zc = min(max(z, 0), h.gz - 1);
            first_a = h.gx * (max(cy - 1, 0) + h.gy * zc);
            last_a = h.gx * (min(cy + 1, h.gy - 1) + h.gy * zc) + h.gx;
            row_b = row_c = first_a - x0; // (their loads repeat lane s's first one; the runs do not exist)
            in_b = in_c = false;
        }
        int lo_a = cs[first_a], end_a = cs[last_a];
        int lo_b = cs[row_b + x0], end_b = cs[row_b + x1 + 1];
        int lo_c = cs[row_c + x0], end_c = cs[row_c + x1 + 1];
        asm volatile("" : "+v"(lo_a), "+v"(end_a), "+v"(lo_b), "+v"(end_b), "+v"(lo_c), "+v"(end_c));
        const int len_a = in_a ? end_a - lo_a : 0, len_b = in_b ? end_b - lo_b : 0, len_c = in_c ? end_c - lo_c : 0;

        // Every lane appends ITS hits to ITS sixteen slots — no ballot, no slot arithmetic across the group (that was ~13 of
        // the ~26 vector instructions a tested candidate cost); a miss is stored to slot 16 instead of branching, and so is
        // the seventeenth hit of a lane (the count goes on: such a wavefront is redone by the general body).
        int cnt_l = 0; // my hits
        bool crowded = false; // (wave-uniform) a single centre's candidates do not fit the LDS strip: the general body takes over
        // (slots 16 .. 19 of a segment are spare: a miss goes to 16 + (centre pair mod 4), so that the eight centres whose strips
        // start in the same bank spread their — frequent — miss stores over four banks instead of one)
        const int miss = 16 + ((g >> 1) & 3);
        auto slots = [&](bool has_a, bool near_a, bool has_b, bool near_b, int ia, int ib) {
            const bool hit_a = has_a && near_a, hit_b = has_b && near_b;
            seg[hit_a ? min(cnt_l, 16) : miss] = ia;
            cnt_l += hit_a ? 1 : 0;
            seg[hit_b ? min(cnt_l, 16) : miss] = ib;
            cnt_l += hit_b ? 1 : 0;
        };
        const char *pts_bytes = reinterpret_cast<const char *>(pts);
        auto record = [&](int position) { // (positions past the end of a run are read — the array is padded — and discarded)
            return *reinterpret_cast<const float4 *>(pts_bytes + ((unsigned)position << 4));
        };
        if (slab) {
            // three long runs, walked side by side: step t tests the candidates 8 t .. 8 t + 7 of each (six loads in flight per
            // lane).  Positions are kept as byte offsets; a lane whose runs have ended keeps reading while others in the wavefront
            // go on — at most BQ_RUN records past a run's end: the next cloud's records or the padding behind the last cloud.
            crowded = __builtin_amdgcn_ballot_w64(len_a > BQ_RUN) != 0ull;
            const int b0 = quad_bcast<0>(in_a ? lo_a : 0), b1 = quad_bcast<1>(in_a ? lo_a : 0), b2 = quad_bcast<2>(in_a ? lo_a : 0);
            const unsigned e0 = (unsigned)(b0 + quad_bcast<0>(len_a)) << 4, e1 = (unsigned)(b1 + quad_bcast<1>(len_a)) << 4,
                           e2 = (unsigned)(b2 + quad_bcast<2>(len_a)) << 4;
            unsigned q0 = (unsigned)(b0 + sub) << 4, q1 = (unsigned)(b1 + sub) << 4, q2 = (unsigned)(b2 + sub) << 4;
            auto rec = [&](unsigned byte_offset) { return *reinterpret_cast<const float4 *>(pts_bytes + byte_offset); };
            constexpr unsigned NEXT = CL * 16u; // my second candidate of a step
            // (Software-pipelining this loop — the loads of step t + 1 issued before step t is tested, to shorten the wavefront's chain
            // of dependent round trips — needs 24 more registers than the 64 that eight wavefronts per SIMD leave: 116-140 bytes of
            // scratch per lane and 46 us instead of 17 for the kernel.  Measured at the end of round 5 and dropped.)
            if (!crowded)
                for (;;) {
                    const float4 a0 = rec(q0), c0 = rec(q0 + NEXT);
                    const float4 a1 = rec(q1), c1 = rec(q1 + NEXT);
                    const float4 a2 = rec(q2), c2 = rec(q2 + NEXT);
                    __builtin_amdgcn_sched_barrier(0);
                    const ogc_v2f d0 = sqdist_pair(ogc_v2f{a0.x, c0.x}, ogc_v2f{a0.y, c0.y}, ogc_v2f{a0.z, c0.z}, me.x, me.y, me.z);
                    slots(q0 < e0, d0.x < radius2, q0 + NEXT < e0, d0.y < radius2, __float_as_int(a0.w), __float_as_int(c0.w));
                    const ogc_v2f d1 = sqdist_pair(ogc_v2f{a1.x, c1.x}, ogc_v2f{a1.y, c1.y}, ogc_v2f{a1.z, c1.z}, me.x, me.y, me.z);
                    slots(q1 < e1, d1.x < radius2, q1 + NEXT < e1, d1.y < radius2, __float_as_int(a1.w), __float_as_int(c1.w));
                    const ogc_v2f d2 = sqdist_pair(ogc_v2f{a2.x, c2.x}, ogc_v2f{a2.y, c2.y}, ogc_v2f{a2.z, c2.z}, me.x, me.y, me.z);
                    slots(q2 < e2, d2.x < radius2, q2 + NEXT < e2, d2.y < radius2, __float_as_int(a2.w), __float_as_int(c2.w));
                    q0 += 2 * NEXT; q1 += 2 * NEXT; q2 += 2 * NEXT;
                    if (__builtin_amdgcn_ballot_w64(q0 < e0 || q1 < e1 || q2 < e2) == 0ull) break;
                }
        } else
        // three runs at a time: six candidate loads in flight per lane
#pragma unroll
        for (int r0 = 0; r0 < 9; r0 += 3) {
            int lo[3], hi[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const int r = r0 + i;
                const int l = r == 0 ? quad_bcast<0>(lo_a) : r == 1 ? quad_bcast<1>(lo_a) : r == 2 ? quad_bcast<2>(lo_a)
                            : r == 3 ? quad_bcast<3>(lo_a) : r == 4 ? quad_bcast<0>(lo_b) : r == 5 ? quad_bcast<1>(lo_b)
                            : r == 6 ? quad_bcast<2>(lo_b) : r == 7 ? quad_bcast<3>(lo_b) : lo_c;
                const int w = r == 0 ? quad_bcast<0>(len_a) : r == 1 ? quad_bcast<1>(len_a) : r == 2 ? quad_bcast<2>(len_a)
                            : r == 3 ? quad_bcast<3>(len_a) : r == 4 ? quad_bcast<0>(len_b) : r == 5 ? quad_bcast<1>(len_b)
                            : r == 6 ? quad_bcast<2>(len_b) : r == 7 ? quad_bcast<3>(len_b) : len_c;
                lo[i] = l;
                hi[i] = l + w;
            }
            float4 ca[3], cb[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                ca[i] = record(lo[i] + sub);
                cb[i] = record(lo[i] + sub + CL);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const ogc_v2f d = sqdist_pair(ogc_v2f{ca[i].x, cb[i].x}, ogc_v2f{ca[i].y, cb[i].y}, ogc_v2f{ca[i].z, cb[i].z},
                                              me.x, me.y, me.z);
                const int p = lo[i] + sub;
                slots(p < hi[i], d.x < radius2, p + CL < hi[i], d.y < radius2, __float_as_int(ca[i].w), __float_as_int(cb[i].w));
                // a run longer than eight candidates (wave-uniform test)
                int pp = p + 2 * CL;
                while (__builtin_amdgcn_ballot_w64(pp < hi[i]) != 0ull) {
                    const float4 a = record(min(pp, n - 1)), c2 = record(min(pp + CL, n - 1));
                    const ogc_v2f d2 = sqdist_pair(ogc_v2f{a.x, c2.x}, ogc_v2f{a.y, c2.y}, ogc_v2f{a.z, c2.z}, me.x, me.y, me.z);
                    slots(pp < hi[i], d2.x < radius2, pp + CL < hi[i], d2.y < radius2, __float_as_int(a.w), __float_as_int(c2.w));
                    pp += 2 * CL;
                }
            }
        }
        OGC_PROBE_T(pt1);
        // hits of my centre (the same number in its four lanes)
        int cnt = cnt_l + __builtin_amdgcn_update_dpp(0, cnt_l, 0xB1, 0xF, 0xF, true); // quad_perm [1,0,3,2]
        cnt += __builtin_amdgcn_update_dpp(0, cnt, 0x4E, 0xF, 0xF, true);               // quad_perm [2,3,0,1]
        general = crowded || __builtin_amdgcn_ballot_w64(cnt > BQ_CAP || cnt_l > 16) != 0ull;
        if (!general) {
            __builtin_amdgcn_s_waitcnt(0xc07f);
            __builtin_amdgcn_wave_barrier();
            int4 k0 = *reinterpret_cast<const int4 *>(seg);
            int4 k1 = *reinterpret_cast<const int4 *>(seg + 4);
            // The sort below takes eight keys per lane.  A lane with more than eight hits (one wavefront in ~8 on the C4 scenes),
            // or a centre with more than BQ_FAST: the four lanes' hits are first moved to the front of the centre's strip, one
            // after the other — the list the long-list code further down expects — and read back eight per lane.
            if (__builtin_amdgcn_ballot_w64(cnt_l > 8 || cnt > BQ_FAST) != 0ull) {
                const int4 k2 = *reinterpret_cast<const int4 *>(seg + 8);
                const int4 k3 = *reinterpret_cast<const int4 *>(seg + 12);
                const int own[16] = {k0.x, k0.y, k0.z, k0.w, k1.x, k1.y, k1.z, k1.w, k2.x, k2.y, k2.z, k2.w, k3.x, k3.y, k3.z, k3.w};
                const int c0 = quad_bcast<0>(cnt_l), c1 = quad_bcast<1>(cnt_l), c2 = quad_bcast<2>(cnt_l);
                const int before = (sub > 0 ? c0 : 0) + (sub > 1 ? c1 : 0) + (sub > 2 ? c2 : 0);
                __builtin_amdgcn_s_waitcnt(0xc07f);
                __builtin_amdgcn_wave_barrier(); // everybody has read its slots
                int *spare = mine + BQ_CAP + sub;  // (a write nobody reads)
#pragma unroll
                for (int r = 0; r < 16; ++r) *(r < cnt_l ? mine + before + r : spare) = own[r];
#pragma unroll
                for (int r = 0; r < 8; ++r) *(sub * 8 + r >= cnt ? mine + sub * 8 + r : spare) = 0x7fffffff;
                __builtin_amdgcn_s_waitcnt(0xc07f);
                __builtin_amdgcn_wave_barrier();
                k0 = *reinterpret_cast<const int4 *>(mine + sub * 8);
                k1 = *reinterpret_cast<const int4 *>(mine + sub * 8 + 4);
            }
            int x[8] = {k0.x, k0.y, k0.z, k0.w, k1.x, k1.y, k1.z, k1.w};
            // bitonic network, element e = 8 * lane + register, every exchange ascending (each merge starts with the
            // "flip" e <-> e ^ (k - 1), then half-cleaners e <-> e ^ j)
#define OGC_BQ_INTRA(MASK)                                                  \
            _Pragma("unroll") for (int r_ = 0; r_ < 8; ++r_)                \
                if ((r_ ^ (MASK)) > r_) {                                   \
                    const int lo_ = min(x[r_], x[r_ ^ (MASK)]);             \
                    x[r_ ^ (MASK)] = max(x[r_], x[r_ ^ (MASK)]);            \
                    x[r_] = lo_;                                            \
                }
            // partner = register (r ^ RMASK) of the lane given by the quad permutation QP; the lower lane keeps the minimum
#define OGC_BQ_INTER(QP, RMASK, UPPER)                                                                  \
            {                                                                                           \
                int p_[8];                                                                              \
                _Pragma("unroll") for (int r_ = 0; r_ < 8; ++r_)                                        \
                    p_[r_] = __builtin_amdgcn_update_dpp(0, x[r_ ^ (RMASK)], QP, 0xF, 0xF, true);       \
                _Pragma("unroll") for (int r_ = 0; r_ < 8; ++r_)                                        \
                    x[r_] = (UPPER) ? max(x[r_], p_[r_]) : min(x[r_], p_[r_]);                          \
            }
            const bool odd = (sub & 1) != 0, high = (sub & 2) != 0;
            OGC_BQ_INTRA(1)                                                     // runs of 2
            OGC_BQ_INTRA(3) OGC_BQ_INTRA(1)                                     // 4
            OGC_BQ_INTRA(7) OGC_BQ_INTRA(2) OGC_BQ_INTRA(1)                     // 8
            OGC_BQ_INTER(0xB1, 7, odd) OGC_BQ_INTRA(4) OGC_BQ_INTRA(2) OGC_BQ_INTRA(1)                              // 16: lane ^ 1
            OGC_BQ_INTER(0x1B, 7, high) OGC_BQ_INTER(0xB1, 0, odd) OGC_BQ_INTRA(4) OGC_BQ_INTRA(2) OGC_BQ_INTRA(1)  // 32: lane ^ 3, ^ 1
#undef OGC_BQ_INTRA
#undef OGC_BQ_INTER
            const int q = __float_as_int(me.w);
            const int kept = min(cnt, NS);
            const int first = cnt > 0 ? quad_bcast<0>(x[0]) : 0;
            int *o = idx_out + ((size_t)b * m + max(q, 0)) * NS;
            OGC_PROBE_T(pf2);
            if (cnt <= BQ_FAST && q >= 0) {
                // lane L holds the sorted entries 8 L .. 8 L + 7.  Stores in which the group's four lanes cover 64
                // CONTIGUOUS bytes need lane L to write entries 4 L .. 4 L + 3 (then 16 + 4 L ..): an exchange inside the
                // quad (a store instruction whose lanes write every other 16 bytes leaves half-written lines everywhere)
                int v[8];
#pragma unroll
                for (int r = 0; r < 8; ++r) v[r] = sub * 8 + r < kept ? x[r] : first;
                int s1[4], s2[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int a1 = __builtin_amdgcn_update_dpp(0, v[r], 0x50, 0xF, 0xF, true);     // quad_perm [0,0,1,1]
                    const int b1 = __builtin_amdgcn_update_dpp(0, v[r + 4], 0x50, 0xF, 0xF, true);
                    const int a2 = __builtin_amdgcn_update_dpp(0, v[r], 0xFA, 0xF, 0xF, true);     // quad_perm [2,2,3,3]
                    const int b2 = __builtin_amdgcn_update_dpp(0, v[r + 4], 0xFA, 0xF, 0xF, true);
                    s1[r] = odd ? b1 : a1;
                    s2[r] = odd ? b2 : a2;
                }
                const int j0 = sub * 4;
                if (j0 < NS) store_row16(o + j0, make_int4(s1[0], s1[1], s1[2], s1[3]));
                if (16 + j0 < NS) store_row16(o + 16 + j0, make_int4(s2[0], s2[1], s2[2], s2[3]));
                const int4 pad = make_int4(first, first, first, first);
#pragma unroll
                for (int j = BQ_FAST; j < NS; j += 16) store_row16(o + j + j0, pad);
            }
            // lists of 33 .. BQ_CAP hits (rare where this kernel is used), one at a time by the WHOLE wavefront: lane e takes
            // element e, its rank is #{f : hits[f] < hits[e]} (distinct indices) from broadcast 16-byte reads of the list,
            // entries are stored one by one.  (Four lanes doing this for their own centre take ~10 us, and so does sending
            // the wavefront through the general body: the kernel ends with its slowest wavefront.)
            unsigned long long big = __builtin_amdgcn_ballot_w64(sub == 0 && cnt > BQ_FAST);
            while (big != 0ull) {
                const int src = __ffsll((long long)big) - 1;
                big &= big - 1ull;
                const int cc = lane_bcast(cnt, src), qq = lane_bcast(q, src);
                int *list = gq_smem + (src >> 2) * BQ_LIST;
                if (lane < 4) list[cc + lane] = 0x7fffffff; // sentinels: the 16-byte reads run past the end
                __builtin_amdgcn_s_waitcnt(0xc07f);
                __builtin_amdgcn_wave_barrier();
                const int ve = lane < cc ? list[lane] : 0x7fffffff;
                int rank = 0;
                for (int f = 0; f < cc; f += 4) {
                    const int4 w = *reinterpret_cast<const int4 *>(list + f);
                    rank += (w.x < ve ? 1 : 0) + (w.y < ve ? 1 : 0) + (w.z < ve ? 1 : 0) + (w.w < ve ? 1 : 0);
                }
                const unsigned long long zero = __builtin_amdgcn_ballot_w64(lane < cc && rank == 0);
                const int lowest = lane_bcast(ve, __ffsll((long long)zero) - 1);
                if (qq >= 0) {
                    int *oc = idx_out + ((size_t)b * m + qq) * NS;
                    if (lane < cc && rank < NS) oc[rank] = ve;
                    if (cc + lane < NS) oc[cc + lane] = lowest;
                }
            }
            OGC_PROBE_T(pf3);
            OGC_PROBE_ADD(16, pt0, pt1);
            OGC_PROBE_ADD(18, pt1, pf2);
            OGC_PROBE_ADD(19, pf2, pf3);
            return;
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier(); // the general body reuses the LDS
    }
#pragma unroll 1
    for (int half = 0; half < CPW / QPW; ++half)
        ball_query_grid_body(lane, grp * CPW + half * QPW, gq_smem, n, m, radius2, NS, BQ_CAP, stride_cells, xyz, hdrs,
                             cell_start, sorted_pts, idx_out);
}

} // namespace ogc_grid

using namespace ogc_grid;

// OGC_BQ_CELLS=0 in the environment: the general kernel for every row length (A/B runs, tests of both kernels)
static bool ogc_bq_cells_enabled() {
    const char *e = getenv("OGC_BQ_CELLS");
    return !(e && e[0] == '0');
}

namespace {
constexpr int BQ_CELLS_WPB = 1; // wavefronts per workgroup of the four-lane kernel (a workgroup is only its unit of dispatch)

// the query kernels of ogc_ball_query on a built grid (four lanes per centre for the usual row lengths; the general kernel —
// eight centres per wavefront — otherwise)
int launch_ball_query(const GridLayout &L, void *grid, int b, int n, int m, float radius, int nsample, const float *xyz, int *idx,
                      hipStream_t s) {
    GridHdr *hdrs = L.hdrs(grid);
    int *cell_start = L.cell_start(grid);
    float4 *sorted_pts = L.sorted_pts(grid);
    const int stride_cells = STRIDE_CELLS;
    const int hit_cap = ball_query_hit_cap(nsample);
    const int lds4_ints = (int)((ball_query_cells_lds(n, nsample) + 15) / 16 * 4); // per wavefront
    const dim3 grid4(ogc_divup(ogc_divup(n, CPW), BQ_CELLS_WPB), b);
#define OGC_BQ_CELLS(NS)                                                                                                     \
    hipLaunchKernelGGL((ball_query_cells_kernel<NS, BQ_CELLS_WPB>), grid4, dim3(OGC_WAVE * BQ_CELLS_WPB),                    \
                       (size_t)lds4_ints * 4 * BQ_CELLS_WPB, s, n, m, radius * radius, stride_cells, lds4_ints, xyz, hdrs,   \
                       cell_start, sorted_pts, idx)
    const bool cells = ogc_bq_cells_enabled();
    if (nsample == 64 && cells) OGC_BQ_CELLS(64);
    else if (nsample == 32 && cells) OGC_BQ_CELLS(32);
    else if (nsample == 16 && cells) OGC_BQ_CELLS(16);
    else
        hipLaunchKernelGGL(ball_query_grid_kernel, dim3(ogc_divup(n, QPW), b), dim3(OGC_WAVE),
                           ball_query_body_lds(n, nsample, hit_cap), s, n, m, radius * radius, nsample, hit_cap, stride_cells, xyz,
                           hdrs, cell_start, sorted_pts, idx);
#undef OGC_BQ_CELLS
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        ogc_set_error("ogc_ball_query (grid): launch failed: %s", hipGetErrorString(e));
        return OGC_ERR_LAUNCH;
    }
    return OGC_OK;
}

bool ball_query_grid_applies(int n, int nsample, float radius) {
    return n >= 1024 && ball_query_body_lds(n, nsample, ball_query_hit_cap(nsample)) <= 64 * 1024 && radius > 0.0f && radius < 3.0e38f;
}
} // namespace

int ogc_ball_query_grid(int b, int n, int m, float radius, int nsample, const float *new_xyz, const float *xyz,
                        int *idx, hipStream_t s) {
    // the cell-ordered traversal needs the centres to BE the points (ball_query(pc, pc), the reference's only live
    // use: losses/seg_loss_unsup.py:151, losses/flow_loss_unsup.py:84); other centre sets use the all-pairs scan
    const bool same = (new_xyz == xyz) && (m == n);
    if (!same || !ball_query_grid_applies(n, nsample, radius)) return OGC_ERR_UNSUPPORTED;
    const GridLayout L(b, n);
    void *ws = ogc_workspace(s, L.total());
    if (!ws) return OGC_ERR_UNSUPPORTED;
    launch_grid_build(b, n, radius, 0, STRIDE_CELLS, xyz, L.hdrs(ws), L.cell_start(ws), L.sorted_pts(ws), s);
    return launch_ball_query(L, ws, b, n, m, radius, nsample, xyz, idx, s);
}

// ---- the same query on a grid built by ogc_cell_grid_build (fused extension, include/ogc_ops.h) ---------------------------------
extern "C" int ogc_ball_query_cells(int b, int n, float radius, int nsample, const float *xyz, const void *grid, float grid_radius,
                                    int *idx, ogc_stream_t stream) {
    OGC_REQUIRE(b >= 0 && n >= 0 && nsample >= 0, "ogc_ball_query_cells: negative dimension");
    if (b == 0 || n == 0 || nsample == 0) return OGC_OK;
    OGC_REQUIRE(xyz && grid && idx, "ogc_ball_query_cells: null pointer");
    OGC_REQUIRE((long long)b * n * nsample < (1ll << 31), "ogc_ball_query_cells: idx exceeds 32-bit indexing");
    // cells are 1.01 x the radius the grid was built for: a query of up to that radius finds its hits in the 27 cells around it
    if (!(radius <= grid_radius) || !ball_query_grid_applies(n, nsample, radius)) {
        ogc_set_error("ogc_ball_query_cells: radius %g exceeds the grid's (%g), or a shape the cell lists do not take (n=%d, "
                      "nsample=%d)", (double)radius, (double)grid_radius, n, nsample);
        return OGC_ERR_UNSUPPORTED;
    }
    return launch_ball_query(GridLayout(b, n), const_cast<void *>(grid), b, n, n, radius, nsample, xyz, idx, (hipStream_t)stream);
}

// grid_knn.hip — exact nearest-neighbour searches over the cell lists of grid.hip: "the k smallest (distance, index) keys" of
// the reference's stable insertion (interpolate_gpu.cu:36-52), by
//   knn_grid_kernel        eight (sixteen, thirty-two) lanes per query scan the cells shell by shell until the k-th distance is covered;
//   knn_wave_kernel        plain k-NN, k <= 32: the whole wavefront on one query at a time, selection by a moving threshold;
//   knn_cells_kernel       the radius-limited search of a cloud in itself: four lanes per query over the 27 cells around it;
//   three_nn_grid_kernel   one lane per query, the three smallest keys in registers.
#include <stdlib.h>

#include "grid_dev.h"

namespace ogc_grid {

// Exact k nearest neighbours over the cell lists: "the k smallest (distance, index) keys", which is what the
// reference's stable insertion computes (interpolate_gpu.cu:36-52).  EIGHT lanes per query, as in the ball query.
// The query's block of (2R+1)^3 cells is scanned shell by shell (R = 1, 2, ...): every point closer than R*h lies
// inside the block (the query is projected into the box first; projection is contractive per axis), so the search
// stops as soon as k keys are held and the k-th distance is below (R*h)^2 (with a 0.1 % guard for the fp32 cell
// quotient) — or the block covers the whole grid.  The kept set is an unordered LDS array with its maximum tracked;
// a candidate is admitted iff its key is below that maximum (strict '<' on (distance, index)), exactly the
// reference's rule whatever the order in which candidates are met.
// ---- the first block of a plain k-NN as ONE sorting network ------------------------------------------------------------------
// 8 NK keys of a query (NK per lane of its 8-lane group, element e = lane * NK + register) sorted ascending by a bitonic
// network: compare-exchange distances below NK stay inside a lane (register pairs, compile-time indices), the others are
// lane exchanges (ds_swizzle xor 1 / 2 / 4).  All eight groups of the wavefront run the same instruction stream, so the
// cost is per wavefront, not per admitted candidate as with the insert-and-rescan of `consider` (which serialises over
// the candidates of all eight queries: ~60 % of the kernel's instructions at k = 32).
template <int X>
__device__ __forceinline__ u64 knn_xor_lane(u64 v) {
    const unsigned lo = (unsigned)__builtin_amdgcn_ds_swizzle((int)(unsigned)v, (X << 10) | 0x1F);
    const unsigned hi = (unsigned)__builtin_amdgcn_ds_swizzle((int)(unsigned)(v >> 32), (X << 10) | 0x1F);
    return ((u64)hi << 32) | lo;
}

template <int NK, int SUBT>
__device__ __forceinline__ void knn_sort_keys(u64 (&key)[NK], int sub) {
    constexpr int N = SUBT * NK;
#pragma unroll
    for (int size = 2; size <= N; size <<= 1) {
#pragma unroll
        for (int d = size >> 1; d >= 1; d >>= 1) {
            if (d >= NK) {
                const int lx = d / NK;
                const bool lower = (sub & lx) == 0;
#pragma unroll
                for (int t = 0; t < NK; ++t) {
                    const u64 other = lx == 1 ? knn_xor_lane<1>(key[t]) : (lx == 2 ? knn_xor_lane<2>(key[t]) : (lx == 4 ? knn_xor_lane<4>(key[t]) : (lx == 8 ? knn_xor_lane<8>(key[t]) : knn_xor_lane<16>(key[t]))));
                    const bool up = ((sub * NK + t) & size) == 0;
                    const bool take = (up == lower) ? other < key[t] : other > key[t];
                    key[t] = take ? other : key[t];
                }
            } else {
#pragma unroll
                for (int t = 0; t < NK; ++t) {
                    if ((t & d) == 0) {
                        const bool up = ((sub * NK + t) & size) == 0;
                        const u64 a = key[t], c = key[t | d];
                        const bool sw = up ? c < a : a < c;
                        key[t] = sw ? c : a;
                        key[t | d] = sw ? a : c;
                    }
                }
            }
        }
    }
}

// keys of the flat candidate list `mine[0 .. total)` (total <= 8 NK), sorted; the k smallest go to kept[] in ascending order.
// Returns the number kept.
template <int NK, int SUBT>
__device__ __forceinline__ int knn_first_block(const float4 *__restrict__ pts, const int *mine, int total, float qx, float qy,
                                               float qz, int sub, int k, u64 *kept, int have) {
    // slots 0 .. have - 1: the keys kept so far (a later shell merges into them); then the `total` new candidates
    constexpr int SUB = SUBT; // lanes per query (shadows the file's constant)
    u64 key[NK];
    float4 cand[NK];
#pragma unroll
    for (int t = 0; t < NK; ++t) { // all loads in flight; slot t * 8 + sub (any assignment will do: everything is sorted)
        const int f = t * SUB + sub - have;
        cand[t] = make_float4(NAN, NAN, NAN, 0.f);
        if (f >= 0 && f < total) cand[t] = pts[mine[f]];
    }
    int valid = 0;
#pragma unroll
    for (int t = 0; t < NK; ++t) {
        const float d = ogc_sqdist(qx, qy, qz, cand[t].x, cand[t].y, cand[t].z);
        bool ok = d < INFINITY; // NaN / inf are never selected (empty slots hold NaN)
        key[t] = ok ? (((u64)__float_as_uint(d) << 32) | (unsigned)__float_as_int(cand[t].w)) : ~0ull;
        if (t * SUB + sub < have) { key[t] = kept[t * SUB + sub]; ok = true; }
        valid += ok ? 1 : 0;
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier(); // kept[] is rewritten below
    valid += __builtin_amdgcn_ds_swizzle(valid, (1 << 10) | 0x1F);
    valid += __builtin_amdgcn_ds_swizzle(valid, (2 << 10) | 0x1F);
    valid += __builtin_amdgcn_ds_swizzle(valid, (4 << 10) | 0x1F);
    if constexpr (SUBT >= 16) valid += __builtin_amdgcn_ds_swizzle(valid, (8 << 10) | 0x1F);
    if constexpr (SUBT == 32) valid += __builtin_amdgcn_ds_swizzle(valid, (16 << 10) | 0x1F);
    knn_sort_keys<NK, SUBT>(key, sub);
    const int keep = min(valid, k);
#pragma unroll
    for (int t = 0; t < NK; ++t) {
        const int e = sub * NK + t;
        if (e < keep) kept[e] = key[t];
    }
    return keep;
}

// MODE 0: squared distances (ogc_knn).  MODE 1: sqrt + radius clamp of the indices (ogc_knn_clamped).
template <int MODE, int SUBT = 8>
__global__ __launch_bounds__(OGC_WAVE, 4) void knn_grid_kernel(int n, int m, int k, float radius, float lim2, int stride_cells,
                                                            int deferred, const float *__restrict__ unknown,
                                                            const GridHdr *__restrict__ hdrs,
                                                            const int *__restrict__ cell_start,
                                                            const float4 *__restrict__ sorted_pts,
                                                            float *__restrict__ dist_out, int *__restrict__ idx_out) {
    extern __shared__ __attribute__((aligned(16))) u64 kq_smem[];
    // SUBT lanes per query: 8 (eight queries per wavefront), or 16 (four) for launches that leave most of the chip idle — few
    // queries of one or two clouds, FlowStep3D at B = 1 — where a wavefront's serial work per query, not the number of wavefronts, is the time
    constexpr int SUB = SUBT, QPW = OGC_WAVE / SUBT;
    const int lane = threadIdx.x, b = blockIdx.y;
    const int sub = lane & (SUB - 1), qi = lane / SUB;
    u64 *kept = kq_smem + (size_t)qi * k;           // [QPW][k]
    u64 *outk = kq_smem + (size_t)(QPW + qi) * k;   // [QPW][k]
    int *flat = reinterpret_cast<int *>(kq_smem + (size_t)2 * QPW * k); // [QPW][KNN_FLAT_CAP] positions of the first shell
    const GridHdr h = hdrs[b];
    // deferred: knn_cells_kernel ran first.  It did every row of a cloud it could take except the rows it marked with
    // idx[row][0] = -1 (a list longer than its register sort), and nothing of a cloud flagged knn_general.
    // (deferred == 2: knn_wave_kernel ran first on EVERY cloud — whatever knn_general says — and marked the rows it left)
    if (deferred && (deferred == 2 || !h.knn_general) && !h.pending) return;
    int p = blockIdx.x * QPW + qi;
    if (deferred && (deferred == 2 || !h.knn_general) && p < n && idx_out[((size_t)b * n + p) * k] != -1) p = n; // done already: no work, no output
    const int *cs = cell_start + (size_t)b * stride_cells;
    const float4 *pts = sorted_pts + (size_t)b * m;
    const unsigned below = (1u << sub) - 1u;

    float qx = NAN, qy = NAN, qz = NAN;
    if (p < n) {
        const float *u = unknown + ((size_t)b * n + p) * 3;
        qx = u[0]; qy = u[1]; qz = u[2];
    }
    int cnt = 0, maxpos = 0;
    u64 maxkey = 0;
    // Radius-limited search (MODE 1 with a radius): a neighbour beyond the radius is replaced by the nearest one in the
    // output whatever it is, so only candidates WITHIN the radius are kept (in C4's smoothness term ~2 of the ~27 a
    // block holds — the kept set, its maximum tracking and the final rank sort shrink accordingly); the nearest
    // candidate of all is tracked on the side for the rows that have nobody within the radius.
    // within  <=>  sqrtf(d2) <= radius  <=>  d2 <= lim2, lim2 = the largest float whose (correctly rounded) root is
    // <= radius (sqrtf is monotone), found among the neighbours of radius^2 by the host (knn_radius_limit2).
    const bool limited = MODE == 1 && radius >= 0.0f;
    u64 best_any = ~0ull; // per lane: the smallest key this lane has seen (limited mode)
    bool kept_sorted = false; // kept[0 .. cnt) is in ascending order (straight from the sorting network of the first block)
    int total_scanned = 0;
    auto rescan_max = [&]() {
        u64 mk = 0;
        int mp = 0;
        for (int e = sub; e < k; e += SUB) {
            const u64 v = kept[e];
            if (v >= mk) { mk = v; mp = e; }
        }
#pragma unroll
        for (int off = 1; off < SUB; off <<= 1) {
            const u64 ov = shfl_xor_u64(mk, off);
            const int op = __shfl_xor(mp, off, 64);
            if (ov > mk) { mk = ov; mp = op; }
        }
        maxkey = mk;
        maxpos = mp;
    };
    // one round of the scan: the group's lane `sub` holds candidate `cand` (valid or not)
    auto consider = [&](bool valid, const float4 cand) {
        bool adm = false;
        u64 key = 0;
        if (valid) {
            const float d = ogc_sqdist(qx, qy, qz, cand.x, cand.y, cand.z);
            if (d < INFINITY) { // NaN / inf are never selected
                key = ((u64)__float_as_uint(d) << 32) | (unsigned)__float_as_int(cand.w);
                adm = cnt < k || key < maxkey;
                if (limited) {
                    best_any = key < best_any ? key : best_any;
                    adm = adm && d <= lim2;
                }
            }
        }
        const u64 ball = __builtin_amdgcn_ballot_w64(adm);
        if (ball == 0) return;
        const unsigned slice = (unsigned)(ball >> (qi * SUB)) & (SUB == 32 ? 0xFFFFFFFFu : ((1u << (SUB & 31)) - 1u));
        if (slice == 0) return;
        const int nh = __popc(slice);
        kept_sorted = false;
        if (cnt + nh <= k) {
            if (adm) kept[cnt + __popc(slice & below)] = key;
            cnt += nh;
            if (cnt == k) rescan_max();
        } else {
            for (int t = 0; t < SUB; ++t) {
                if (!((slice >> t) & 1u)) continue;
                const u64 kt = shfl_u64(key, qi * SUB + t);
                if (cnt < k) {
                    if (sub == 0) kept[cnt] = kt;
                    if (++cnt == k) rescan_max();
                } else if (kt < maxkey) {
                    if (sub == 0) kept[maxpos] = kt;
                    rescan_max();
                }
            }
        }
    };
    // scan the run [j0, j1) of the cell-sorted arrays with the 8 lanes of the group
    auto scan_run = [&](int j0, int j1) {
        for (int j = j0 + sub; __builtin_amdgcn_ballot_w64(j < j1) != 0; j += SUB) {
            float4 cand = make_float4(NAN, NAN, NAN, 0.f);
            if (j < j1) cand = pts[j];
            consider(j < j1, cand);
        }
    };

    const bool active = p < n && h.npts > 0 && qx == qx && qy == qy && qz == qz; // NaN queries select nothing
    if (active) {
        const float edge = 1.0f / h.inv_h;
        OGC_GRID_AXES(h, qx, qy, qz, fx, fy, fz);
        const int cx = min(max(cell_coord(fx, h.minx, h.inv_h, h.gx), 0), h.gx - 1);
        const int cy = min(max(cell_coord(fy, h.miny, h.inv_h, h.gy), 0), h.gy - 1);
        const int cz = min(max(cell_coord(fz, h.minz, h.inv_h, h.gz), 0), h.gz - 1);
        const int rmax = max(max(max(cx, h.gx - 1 - cx), max(cy, h.gy - 1 - cy)), max(cz, h.gz - 1 - cz));
        const int R0 = limited ? 1 : 2; // radius (in cells) of the block scanned first
        for (int R = R0;; ++R) {
            const int xa = max(cx - R, 0), xb = min(cx + R, h.gx - 1);
            // Shell R as ONE flat list of record positions (LDS), scanned eight candidates at a time with the next load in
            // flight.  A shell is (2R + 1)^2 rows of cells; a face row (or any row of the first block) contributes its
            // whole x-extent as one run of the cell-sorted array, an inner row its two end cells.  Walking the runs one
            // after the other is a dependent (bounds -> records) round trip per run with most of the eight lanes idle (a
            // run holds a handful of points); here the lanes fetch the bounds of all runs (two passes: lengths, then
            // positions), and the records are then read back to back.
            bool done_flat = false;
            {
                const int side = 2 * R + 1, nrows = side * side;
                const float inv_side = 1.0f / (float)side;
                auto row_runs = [&](int r, int &s0, int &l0, int &s1, int &l1) {
                    s0 = l0 = s1 = l1 = 0;
                    const int rz = (int)(((float)r + 0.5f) * inv_side); // r / side without an integer division (r < 2^12)
                    const int z = cz + rz - R, y = cy + (r - rz * side) - R;
                    if (r >= nrows || z < 0 || z >= h.gz || y < 0 || y >= h.gy) return;
                    const int rowc = h.gx * (y + h.gy * z);
                    const bool face = R == R0 || z == cz - R || z == cz + R || y == cy - R || y == cy + R;
                    if (face) {
                        s0 = cs[rowc + xa];
                        l0 = cs[rowc + xb + 1] - s0;
                    } else {
                        if (cx - R >= 0) { s0 = cs[rowc + cx - R]; l0 = cs[rowc + cx - R + 1] - s0; }
                        if (cx + R <= h.gx - 1) { s1 = cs[rowc + cx + R]; l1 = cs[rowc + cx + R + 1] - s1; }
                    }
                };
                int mine_total = 0;
                for (int r = sub; r < nrows; r += SUB) {
                    int s0, l0, s1, l1;
                    row_runs(r, s0, l0, s1, l1);
                    mine_total += l0 + l1;
                }
                int incl = mine_total;
#pragma unroll
                for (int off = 1; off < SUB; off <<= 1) {
                    const int up = __shfl_up(incl, off, SUB);
                    if (sub >= off) incl += up;
                }
                const int total = __shfl(incl, qi * SUB + SUB - 1, 64);
                if (total <= KNN_FLAT_CAP) {
                    int *mine = flat + qi * KNN_FLAT_CAP;
                    int w = incl - mine_total;
                    for (int r = sub; r < nrows; r += SUB) {
                        int s0, l0, s1, l1;
                        row_runs(r, s0, l0, s1, l1);
                        for (int i = 0; i < l0; ++i) mine[w + i] = s0 + i;
                        w += l0;
                        for (int i = 0; i < l1; ++i) mine[w + i] = s1 + i;
                        w += l1;
                    }
                    __builtin_amdgcn_s_waitcnt(0xc07f);
                    __builtin_amdgcn_wave_barrier();
                    if (!limited && R == R0 && total <= 128) {
                        // plain k-NN, first block: select by sorting instead of insert-and-rescan (later shells admit few
                        // candidates — the kept maximum filters them — and a merge network per shell measured slower)
                        cnt = knn_first_block<128 / SUB, SUB>(pts, mine, total, qx, qy, qz, sub, k, kept, 0);
                        __builtin_amdgcn_s_waitcnt(0xc07f);
                        __builtin_amdgcn_wave_barrier();
                        kept_sorted = true;
                        if (cnt == k) { maxkey = kept[k - 1]; maxpos = k - 1; }
                        total_scanned = -1; // (marks: nothing left for the loop below)
                    }
                    const float4 nothing = make_float4(NAN, NAN, NAN, 0.f);
                    int f = total_scanned < 0 ? total : sub;
                    total_scanned = 0;
                    float4 cur = nothing;
                    if (f < total) cur = pts[mine[f]];
                    while (__builtin_amdgcn_ballot_w64(f < total) != 0) {
                        const int fn = f + SUB;
                        float4 nxt = nothing;
                        if (fn < total) nxt = pts[mine[fn]];
                        consider(f < total, cur);
                        cur = nxt;
                        f = fn;
                    }
                    __builtin_amdgcn_wave_barrier(); // the list is rewritten by the next shell
                    done_flat = true;
                }
            }
            if (!done_flat) {
                for (int z = max(cz - R, 0); z <= min(cz + R, h.gz - 1); ++z)
                    for (int y = max(cy - R, 0); y <= min(cy + R, h.gy - 1); ++y) {
                        const int rowc = h.gx * (y + h.gy * z);
                        const bool face = R == R0 || z == cz - R || z == cz + R || y == cy - R || y == cy + R;
                        if (face) { // the whole x-extent of this row belongs to shell R (for R = R0: the full first block)
                            scan_run(cs[rowc + xa], cs[rowc + xb + 1]);
                        } else {    // inner row: only the two end cells are new
                            if (cx - R >= 0) scan_run(cs[rowc + cx - R], cs[rowc + cx - R + 1]);
                            if (cx + R <= h.gx - 1) scan_run(cs[rowc + cx + R], cs[rowc + cx + R + 1]);
                        }
                    }
            }
            if (R >= rmax) break; // the block covers the grid
            const float cover = (float)R * edge * 0.999f;
            if (cnt == k) {
                if (__uint_as_float((unsigned)(maxkey >> 32)) < cover * cover) break;
            }
            if (limited && cover >= radius) {
                // every point within the radius has been seen (unseen points are farther than R * edge >= 1.001 r).
                // Entry 0 must still be the true nearest neighbour: stop only when the nearest seen candidate lies
                // inside the covered ball (always the case when somebody is within the radius).
                u64 best = best_any;
#pragma unroll
                for (int off = 1; off < SUB; off <<= 1) {
                    const u64 ob = shfl_xor_u64(best, off);
                    best = ob < best ? ob : best;
                }
                if (best != ~0ull && __uint_as_float((unsigned)(best >> 32)) < cover * cover) break;
            }
        }
    }
    // rank sort (keys are distinct: the index is part of the key) — unless the kept set is still the sorted output of
    // the first block's network
    if (kept_sorted) {
        outk = kept;
    } else {
        for (int e = sub; e < cnt; e += SUB) {
            const u64 ve = kept[e];
            int rank = 0;
            for (int f = 0; f < cnt; ++f) rank += kept[f] < ve ? 1 : 0;
            outk[rank] = ve;
        }
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
    if (p < n) {
        const size_t base = ((size_t)b * n + p) * k;
        int first = cnt > 0 ? (int)(unsigned)outk[0] : 0;
        if (limited && cnt == 0) { // nobody within the radius: every entry is the nearest neighbour of all
            u64 best = best_any;
#pragma unroll
            for (int off = 1; off < SUB; off <<= 1) {
                const u64 ob = shfl_xor_u64(best, off);
                best = ob < best ? ob : best;
            }
            first = best != ~0ull ? (int)(unsigned)best : 0;
        }
        for (int j = sub; j < k; j += SUB) {
            float d = INFINITY;
            int id = 0;
            if (j < cnt) {
                const u64 key = outk[j];
                d = __uint_as_float((unsigned)(key >> 32));
                id = (int)(unsigned)key;
            }
            if (MODE == 1) {
                d = sqrtf(d);
                if (d > radius && radius >= 0.0f) { id = first; d = INFINITY; } // clamped entries carry dist = +inf
            }
            dist_out[base + j] = d;
            idx_out[base + j] = id;
        }
    }
}

// ---- plain k-NN (k <= 32) with the WHOLE WAVEFRONT on one query at a time --------------------------------------------------
// knn_grid_kernel gives a query eight lanes: the candidates of its first block (5^3 cells, ~120 points) are sorted by a 128-key
// network of 64-bit compare-exchanges, five instructions each, and a query whose k-th neighbour lies outside that block — about
// half of them: the cells are half the EXPECTED k-th distance — walks a second shell by insertion while the other seven queries of
// the wavefront wait: ~5400 vector instructions per eight queries, 0.30 of the issue peak at 16 x 8192 x 8192, k = 32.
// Selecting k of a few hundred candidates does not need them sorted.  Here a wavefront takes its queries one after the other:
//   * cells of ~2 points (k / 16 per cell), block = 5 x 5 x 5 cells = 25 runs of the cell-sorted array, ~250 candidates covering
//     1.28 x the expected k-th distance; lanes 0 .. 24 fetch the runs' bounds, a wave scan numbers the candidates, the lanes
//     write their runs' positions into a flat LDS list and every lane then loads up to four candidates: one round trip each;
//   * a THRESHOLD on the squared distance is moved until between k and 64 candidates lie at or below it: each trial is four
//     compares whose masks are counted by the scalar unit; the first guess comes from the cell edge (the density), the next ones
//     from count ~ T^(3/2) — two or three trials;
//   * those <= 64 candidates are compacted into one (distance, index) key per lane and sorted by a 21-stage bitonic network
//     ACROSS THE LANES (one 64-bit compare-exchange per lane and stage); lanes 0 .. k - 1 then hold the row, in order, and
//     store it as two coalesced pieces.
// Exact by the argument of knn_grid_kernel: everything outside the selection is farther than everything inside, keys are
// distinct, and the row is accepted only when the k-th distance lies inside the ball the block is known to cover (or the block
// covers the grid).  A query whose block does not (sparse regions, more than 256 candidates, more than 64 ties at the
// threshold) is marked idx[row][0] = -1 for knn_grid_kernel, launched afterwards in `deferred == 2` mode.
constexpr int KW_PER_LANE = 12;                      // candidates per lane, at most
constexpr int KW_CAND = KW_PER_LANE * OGC_WAVE;      // per query and block
// (cells: grid_header with knn_div = -(candidates wanted in the clipped block) = -min(7 k, 230))

__device__ __forceinline__ u64 kw_xor_lane(u64 v, int d) {
    const unsigned lo = __shfl_xor((unsigned)v, d, 64), hi = __shfl_xor((unsigned)(v >> 32), d, 64);
    return ((u64)hi << 32) | lo;
}

template <int MODE>
__global__ __launch_bounds__(OGC_WAVE, 8) void knn_wave_kernel(int n, int m, int k, float radius, int stride_cells, int qpw,
                                                               const float *__restrict__ unknown, GridHdr *__restrict__ hdrs,
                                                               const int *__restrict__ cell_start,
                                                               const float4 *__restrict__ sorted_pts,
                                                               float *__restrict__ dist_out, int *__restrict__ idx_out) {
    __shared__ int flat[KW_CAND];
    __shared__ u64 slots[OGC_WAVE];
    const int lane = threadIdx.x, b = blockIdx.y;
    const GridHdr h = hdrs[b];
    const int *cs = cell_start + (size_t)b * stride_cells;
    const float4 *pts = sorted_pts + (size_t)b * m;
    const float edge = 1.0f / h.inv_h;
    // first threshold: the block (five cells per axis) was sized for ~7 k candidates; a ball holding `want` ~ 1.45 k of them at
    // that density has the volume fraction want / (7 k) of the 125-cell cube (the count model of the trials below corrects it)
    const float want = fminf(1.45f * (float)k, 48.0f);
    const float rk = edge * cbrtf(125.0f * want / (4.18879f * fminf(7.0f * (float)k, 230.0f)));
    const float t_first = rk * rk;
    // row of the block a lane fetches the bounds of: (2R + 1)^2 rows, R = 2 (25 lanes) and R = 3 (49 lanes)
    const int ry2 = lane % 5, rz2 = lane / 5, ry3 = lane % 7, rz3 = lane / 7;
    bool any_left = false;
    // the wavefront's queries (qpw <= 8), one per lane: coordinates and the cell of the projection into the grid, computed once
    // side by side instead of once per query on every lane
    float mqx = NAN, mqy = NAN, mqz = NAN;
    {
        const int pl = blockIdx.x * qpw + lane;
        if (lane < qpw && pl < n) {
            const float *u = unknown + ((size_t)b * n + pl) * 3;
            mqx = u[0]; mqy = u[1]; mqz = u[2];
        }
    }
    int mcx, mcy, mcz;
    {
        OGC_GRID_AXES(h, mqx, mqy, mqz, fx, fy, fz);
        mcx = min(max(cell_coord(fx, h.minx, h.inv_h, h.gx), 0), h.gx - 1);
        mcy = min(max(cell_coord(fy, h.miny, h.inv_h, h.gy), 0), h.gy - 1);
        mcz = min(max(cell_coord(fz, h.minz, h.inv_h, h.gz), 0), h.gz - 1);
    }
    for (int qn = 0; qn < qpw; ++qn) {
        const int p = (blockIdx.x * qpw + qn);
        if (p >= n) break;
        const float qx = lane_bcast(mqx, qn), qy = lane_bcast(mqy, qn), qz = lane_bcast(mqz, qn);
        const size_t base = ((size_t)b * n + p) * k;
        const bool active = h.npts > 0 && qx == qx && qy == qy && qz == qz; // NaN queries select nothing
        int cnt = 0;
        u64 key = ~0ull;
        bool accept = true;
        if (active) {
            const int cx = lane_bcast(mcx, qn), cy = lane_bcast(mcy, qn), cz = lane_bcast(mcz, qn);
            const int rmax = max(max(max(cx, h.gx - 1 - cx), max(cy, h.gy - 1 - cy)), max(cz, h.gz - 1 - cz));
            float T = t_first;
            // the block of (2R + 1)^3 cells, R = 2; a query whose k-th neighbour is not inside the ball that block covers tries
            // R = 3 (the WHOLE block again: the wavefront re-reads ~250 records it had, instead of carrying them)
            for (int R = 2; R <= 3; ++R) {
                accept = true;
                const int xa = max(cx - R, 0), xb = min(cx + R, h.gx - 1);
                const int side = 2 * R + 1;
                int s_r = 0, l_r = 0;
                {
                    const int y = cy + (R == 2 ? ry2 : ry3) - R, z = cz + (R == 2 ? rz2 : rz3) - R;
                    if (lane < side * side && y >= 0 && y < h.gy && z >= 0 && z < h.gz) {
                        const int rowc = h.gx * (y + h.gy * z);
                        s_r = cs[rowc + xa];
                        l_r = cs[rowc + xb + 1] - s_r;
                    }
                }
                // inclusive scan over the wavefront in six DPP steps (row shifts, then the row broadcasts)
                int incl = l_r;
                incl += __builtin_amdgcn_update_dpp(0, incl, 0x111, 0xF, 0xF, true);   // row_shr:1
                incl += __builtin_amdgcn_update_dpp(0, incl, 0x112, 0xF, 0xF, true);   // row_shr:2
                incl += __builtin_amdgcn_update_dpp(0, incl, 0x114, 0xF, 0xF, true);   // row_shr:4
                incl += __builtin_amdgcn_update_dpp(0, incl, 0x118, 0xF, 0xF, true);   // row_shr:8
                incl += __builtin_amdgcn_update_dpp(0, incl, 0x142, 0xA, 0xF, true);   // row_bcast:15 into rows 1, 3
                incl += __builtin_amdgcn_update_dpp(0, incl, 0x143, 0xC, 0xF, true);   // row_bcast:31 into rows 2, 3
                const int total = __builtin_amdgcn_readlane(incl, 63);
                if (total > KW_CAND) { accept = false; break; }     // a crowded block: left to knn_grid_kernel
                const int w = incl - l_r;
                for (int i = 0; __builtin_amdgcn_ballot_w64(i < l_r) != 0ull; ++i)
                    if (i < l_r) flat[w + i] = s_r + i;
                __builtin_amdgcn_s_waitcnt(0xc07f);
                __builtin_amdgcn_wave_barrier();
                const int nch = (total + OGC_WAVE - 1) / OGC_WAVE;  // candidates per lane (wave-uniform)
                float d[KW_PER_LANE];
                int valid = 0;
#pragma unroll
                for (int j = 0; j < KW_PER_LANE; ++j) {
                    d[j] = INFINITY;
                    if (j < nch) {
                        const int f = lane + OGC_WAVE * j;
                        float4 rec = make_float4(NAN, NAN, NAN, 0.f);
                        if (f < total) {
                            rec = pts[flat[f]];
                            flat[f] = __float_as_int(rec.w);     // (only this lane reads slot f: the list now holds the point's index)
                        }
                        const float dj = ogc_sqdist(qx, qy, qz, rec.x, rec.y, rec.z);
                        const bool ok = dj < INFINITY;        // NaN / inf are never selected (empty slots hold NaN)
                        d[j] = ok ? dj : INFINITY;
                        valid += __popcll(__builtin_amdgcn_ballot_w64(ok));
                    }
                }
                // the threshold: between min(k, valid) and 64 candidates at or below it
                int below = 0;
                if (valid <= k) {
                    T = __int_as_float(0x7f7fffff);            // no more candidates than the row holds: all of them (every finite distance)
                    below = valid;
                } else {
                    float lo_t = 0.0f, hi_t = 3.0e38f;         // count(lo_t) < k, count(hi_t) > 64 (once tried)
                    bool found = false;
                    if (!(T < 3.0e38f)) T = t_first;
                    for (int it = 0; it < 24; ++it) {
                        int c = 0;
#pragma unroll
                        for (int j = 0; j < KW_PER_LANE; ++j)
                            if (j < nch) c += __popcll(__builtin_amdgcn_ballot_w64(d[j] <= T));
                        if (c >= k && c <= OGC_WAVE) { below = c; found = true; break; }
                        if (c < k) lo_t = T; else hi_t = T;
                        // next trial: count ~ T^(3/2), kept strictly inside the bracket; bisection once the model stalls
                        float next = T * __powf(want / fmaxf((float)c, 0.5f), 2.0f / 3.0f);
                        if (it >= 6 || !(next > lo_t) || !(next < hi_t)) next = hi_t < 3.0e38f ? 0.5f * (lo_t + hi_t) : 2.0f * fmaxf(T, 1.0e-30f);
                        if (!(next > lo_t) || !(next < hi_t)) break; // the bracket has no float left: ties
                        T = next;
                    }
                    if (!found) { accept = false; break; }      // more than 64 - k ties at the k-th distance: knn_grid_kernel
                }
                int slot_base = 0;
#pragma unroll
                for (int j = 0; j < KW_PER_LANE; ++j) {
                    if (j < nch) {
                        const bool sel = d[j] <= T;
                        const unsigned long long mask = __builtin_amdgcn_ballot_w64(sel);
                        if (mask != 0ull) {
                            const int slot = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, (unsigned)slot_base));
                            if (sel) slots[slot] = ((u64)__float_as_uint(d[j]) << 32) | (unsigned)flat[lane + OGC_WAVE * j];
                            slot_base += __popcll(mask);
                        }
                    }
                }
                __builtin_amdgcn_s_waitcnt(0xc07f);
                __builtin_amdgcn_wave_barrier();
                key = lane < below ? slots[lane] : ~0ull;
                // bitonic network over the 64 lanes, ascending: per stage ONE 64-bit compare; which lanes keep the smaller key is a
                // constant of the stage (ascending block == lower lane of the pair), so "take the partner's key" is the compare's
                // mask xor that constant — a scalar instruction — fed to the two selects (the keys are distinct, sentinels apart,
                // which may go either way); partners by ds_swizzle (xor 1 .. 16) or a lane permutation (xor 32)
#pragma unroll
                for (int size = 2; size <= OGC_WAVE; size <<= 1) {
#pragma unroll
                    for (int dd = size >> 1; dd >= 1; dd >>= 1) {
                        const u64 other = dd == 1 ? knn_xor_lane<1>(key) : dd == 2 ? knn_xor_lane<2>(key) : dd == 4 ? knn_xor_lane<4>(key)
                                        : dd == 8 ? knn_xor_lane<8>(key) : dd == 16 ? knn_xor_lane<16>(key) : kw_xor_lane(key, 32);
                        u64 keep_max = 0ull; // lanes that keep the LARGER key in this stage (compile-time constant)
#pragma unroll
                        for (int l = 0; l < OGC_WAVE; ++l)
                            if ((((l & size) == 0) || size == OGC_WAVE) != ((l & dd) == 0)) keep_max |= 1ull << l;
                        const u64 take = __builtin_amdgcn_ballot_w64(other < key) ^ keep_max;
                        unsigned lo = (unsigned)key, hi = (unsigned)(key >> 32);
                        asm("v_cndmask_b32 %0, %0, %2, %4\n\tv_cndmask_b32 %1, %1, %3, %4"
                            : "+v"(lo), "+v"(hi) : "v"((unsigned)other), "v"((unsigned)(other >> 32)), "s"(take));
                        key = ((u64)hi << 32) | lo;
                    }
                }
                cnt = min(below, k);
                __builtin_amdgcn_wave_barrier(); // (flat / slots are rewritten by the next block or query)
                // the k-th neighbour must lie inside the ball the block covers — unless the block is the whole grid
                const float cover = (float)R * edge * 0.999f;
                const unsigned kth_hi = (unsigned)(__shfl(key, max(cnt - 1, 0), 64) >> 32);
                if (rmax <= R || (cnt == k && __uint_as_float(kth_hi) < cover * cover)) break;
                accept = false;                                 // (R = 3 did not cover it either: knn_grid_kernel's shells)
            }
        }
        if (!accept) {
            if (lane == 0) idx_out[base] = -1;
            any_left = true;
            continue;
        }
        const int first = cnt > 0 ? (int)(unsigned)__shfl(key, 0, 64) : 0;
        if (lane < k) {
            float dv = INFINITY;
            int iv = 0;
            if (lane < cnt) {
                dv = __uint_as_float((unsigned)(key >> 32));
                iv = (int)(unsigned)key;
            }
            if (MODE == 1) {
                dv = sqrtf(dv);
                if (dv > radius && radius >= 0.0f) { iv = first; dv = INFINITY; } // clamped entries carry dist = +inf
            }
            dist_out[base + lane] = dv;
            idx_out[base + lane] = iv;
        }
    }
    if (any_left && lane == 0) hdrs[b].pending = 1;
}


// ---- three nearest neighbours over the cell lists: ONE LANE PER QUERY ------------------------------------------------------------
// three_nn (interpolate_gpu.cu:81-124: the feature-propagation modules' inverse-distance weights, 8192 targets against the 2048
// centres of the level above) as an all-pairs scan tests every target against every centre.  Here a lane takes one target and
// walks the cells around it shell by shell — rows of the (2R + 1)^3 block, a row's x-extent being one run of the cell-sorted
// array — keeping the three smallest (distance, index) keys in registers; it stops when the third distance lies inside the
// ball the scanned block is known to cover (R h, as knn_grid_kernel), or the block covers the grid.  The reference keeps
// the EARLIER index among equal distances (strict '<' while scanning in index order): the smallest keys, whatever the order
// in which candidates are met.  The grid holds ~1.5 points per cell, so the first block (27 cells, ~40 candidates against
// 2048) ends ~95 % of the searches.  Lanes of a wavefront are unrelated targets: every loop runs to its longest lane.
__global__ __launch_bounds__(OGC_WAVE, 8) void three_nn_grid_kernel(int n, int m, int stride_cells, const float *__restrict__ unknown,
                                                                    const GridHdr *__restrict__ hdrs,
                                                                    const int *__restrict__ cell_start,
                                                                    const float4 *__restrict__ sorted_pts,
                                                                    float *__restrict__ dist2, int *__restrict__ idx) {
    const int lane = threadIdx.x, b = blockIdx.y, q = blockIdx.x * OGC_WAVE + lane;
    const GridHdr h = hdrs[b];
    const int *cs = cell_start + (size_t)b * stride_cells;
    const float4 *pts = sorted_pts + (size_t)b * m;
    float qx = NAN, qy = NAN, qz = NAN;
    if (q < n) {
        const float *u = unknown + ((size_t)b * n + q) * 3;
        qx = u[0]; qy = u[1]; qz = u[2];
    }
    const u64 none = (u64)0x7f800000u << 32; // (+inf, index 0): what the reference's rows hold where nothing was found
    u64 k1 = none, k2 = none, k3 = none;
    const float edge = 1.0f / h.inv_h;
    OGC_GRID_AXES(h, qx, qy, qz, fx, fy, fz);
    const int cx = min(max(cell_coord(fx, h.minx, h.inv_h, h.gx), 0), h.gx - 1);
    const int cy = min(max(cell_coord(fy, h.miny, h.inv_h, h.gy), 0), h.gy - 1);
    const int cz = min(max(cell_coord(fz, h.minz, h.inv_h, h.gz), 0), h.gz - 1);
    const int rmax = max(max(max(cx, h.gx - 1 - cx), max(cy, h.gy - 1 - cy)), max(cz, h.gz - 1 - cz));
    bool open = q < n && h.npts > 0 && qx == qx && qy == qy && qz == qz; // (a NaN target selects nothing)
    auto scan_run = [&](int j0, int j1) {
        for (int j = j0; j < j1; ++j) {
            const float4 c = pts[j];
            const float d = ogc_sqdist(qx, qy, qz, c.x, c.y, c.z);
            const u64 key = ((u64)__float_as_uint(d) << 32) | (unsigned)__float_as_int(c.w);
            const bool c1 = key < k1, c2 = key < k2, c3 = key < k3;
            k3 = c2 ? k2 : (c3 ? key : k3);
            k2 = c1 ? k1 : (c2 ? key : k2);
            k1 = c1 ? key : k1;
        }
    };
    for (int R = 1; __builtin_amdgcn_ballot_w64(open) != 0ull; ++R) {
        if (open) {
            const int xa = max(cx - R, 0), xb = min(cx + R, h.gx - 1);
            for (int z = max(cz - R, 0); z <= min(cz + R, h.gz - 1); ++z)
                for (int y = max(cy - R, 0); y <= min(cy + R, h.gy - 1); ++y) {
                    const int rowc = h.gx * (y + h.gy * z);
                    const bool face = R == 1 || z == cz - R || z == cz + R || y == cy - R || y == cy + R;
                    if (face) { // the row's whole x-extent belongs to shell R (R = 1: the full first block)
                        scan_run(cs[rowc + xa], cs[rowc + xb + 1]);
                    } else {    // inner row: only the two end cells are new
                        if (cx - R >= 0) scan_run(cs[rowc + cx - R], cs[rowc + cx - R + 1]);
                        if (cx + R <= h.gx - 1) scan_run(cs[rowc + cx + R], cs[rowc + cx + R + 1]);
                    }
                }
            const float cover = (float)R * edge * 0.999f;
            if (R >= rmax || __uint_as_float((unsigned)(k3 >> 32)) < cover * cover) open = false;
        }
    }
    if (q < n) {
        float *o = dist2 + ((size_t)b * n + q) * 3;
        int *oi = idx + ((size_t)b * n + q) * 3;
        o[0] = __uint_as_float((unsigned)(k1 >> 32)); o[1] = __uint_as_float((unsigned)(k2 >> 32)); o[2] = __uint_as_float((unsigned)(k3 >> 32));
        oi[0] = (int)(unsigned)k1; oi[1] = (int)(unsigned)k2; oi[2] = (int)(unsigned)k3;
    }
}

// ---- radius-limited k-NN of a cloud in itself with FOUR lanes per query ---------------------------------------------------
// ogc_knn_clamped(pc, pc) with a radius (the smoothness term's lists, losses/seg_loss_unsup.py:150: k = 32 within 1 m — about 3
// of the ~10 candidates the 27 cells hold): a neighbour beyond the radius is replaced by the nearest one whatever it is, so the
// row is "the points within the radius, ascending by (distance, index), first K of them, the rest = the first".  That is the
// ball query's traversal with another sort key: the structure of ball_query_cells_kernel — sixteen queries (= points, in cell
// order) per wavefront, four lanes each walking the query's nine runs, slots from the ballots' bits, lists of up to 32 keys
// sorted in registers (64-bit keys here) and stored straight from the registers.  knn_grid_kernel, launched after it in
// `deferred` mode, does what is left: rows marked idx[row][0] = -1 (more than 32 points within the radius) and whole clouds
// the build flagged knn_general (cells shorter than the radius, crowded cells).  Same results as knn_grid_kernel alone.
constexpr int KQ_LIST = BQ_FAST + 4; // keys per list (slot BQ_FAST takes the misses)

template <int K>
__global__ __launch_bounds__(OGC_WAVE, 8) void knn_cells_kernel(int n, float lim2, int stride_cells, GridHdr *__restrict__ hdrs,
                                                                const int *__restrict__ cell_start,
                                                                const float4 *__restrict__ sorted_pts,
                                                                float *__restrict__ dist_out, int *__restrict__ idx_out) {
    extern __shared__ __attribute__((aligned(16))) u64 kc_smem[];
    const int lane = threadIdx.x, b = blockIdx.y, sub = lane & (CL - 1), g = lane >> 2;
    const GridHdr h = hdrs[b];
    if (h.knn_general) return;
    const int *cs = cell_start + (size_t)b * stride_cells;
    const float4 *pts = sorted_pts + (size_t)b * n;
    const int pc = blockIdx.x * CPW + g;
    float4 me = make_float4(NAN, NAN, NAN, __int_as_float(-1));
    if (pc < n) me = pts[pc]; // positions >= h.npts hold the non-finite points: nobody within the radius
    const bool live = pc < h.npts;
    u64 *mine = kc_smem + g * KQ_LIST;
    {   // every list starts as BQ_FAST +inf keys: the sort reads all of them
        const int4 inf4 = make_int4(-1, -1, -1, -1);
        int4 *l4 = reinterpret_cast<int4 *>(mine + sub * (BQ_FAST / CL));
#pragma unroll
        for (int i = 0; i < BQ_FAST / CL / 2; ++i) l4[i] = inf4;
    }
    OGC_GRID_AXES(h, me.x, me.y, me.z, gfx, gfy, gfz);
    const int cx = min(cell_floor(gfx, h.minx, h.inv_h), h.gx - 1);
    const int cy = min(cell_floor(gfy, h.miny, h.inv_h), h.gy - 1);
    const int cz = min(cell_floor(gfz, h.minz, h.inv_h), h.gz - 1);
    const int x0 = max(cx - 1, 0), x1 = min(cx + 1, h.gx - 1);
    const bool slab = h.slab != 0; // (wave-uniform; see ball_query_cells_kernel)
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
        row_b = row_c = first_a - x0;
        in_b = in_c = false;
    }
    int lo_a = cs[first_a], end_a = cs[last_a];
    int lo_b = cs[row_b + x0], end_b = cs[row_b + x1 + 1];
    int lo_c = cs[row_c + x0], end_c = cs[row_c + x1 + 1];
    asm volatile("" : "+v"(lo_a), "+v"(end_a), "+v"(lo_b), "+v"(end_b), "+v"(lo_c), "+v"(end_c));
    const int len_a = in_a ? end_a - lo_a : 0, len_b = in_b ? end_b - lo_b : 0, len_c = in_c ? end_c - lo_c : 0;

    int cnt = 0; // points within the radius of my query (the same number in its four lanes)
    const unsigned below_a = (1u << sub) - 1u, below_b = 0xFu | (below_a << 4);
    const int shift = CL * g;
    auto slots = [&](bool has_a, bool near_a, bool has_b, bool near_b, u64 ka, u64 kb) {
        const unsigned long long ma = __builtin_amdgcn_ballot_w64(has_a) & __builtin_amdgcn_ballot_w64(near_a);
        const unsigned long long mb = __builtin_amdgcn_ballot_w64(has_b) & __builtin_amdgcn_ballot_w64(near_b);
        const unsigned bits = ((unsigned)(ma >> shift) & 0xFu) | (((unsigned)(mb >> shift) & 0xFu) << 4);
        const int sa = cnt + __popc(bits & below_a), sb = cnt + __popc(bits & below_b);
        mine[(has_a && near_a) ? min(sa, BQ_FAST) : BQ_FAST] = ka;
        mine[(has_b && near_b) ? min(sb, BQ_FAST) : BQ_FAST] = kb;
        cnt += __popc(bits);
    };
    const char *pts_bytes = reinterpret_cast<const char *>(pts);
    auto record = [&](int position) { // (positions past the end of a run are read — the array is padded — and discarded)
        return *reinterpret_cast<const float4 *>(pts_bytes + ((unsigned)position << 4));
    };
    auto key_of = [](float d, float w) { return ((u64)__float_as_uint(d) << 32) | (unsigned)__float_as_int(w); };
    if (slab) {
        int p0 = quad_bcast<0>(lo_a), p1 = quad_bcast<1>(lo_a), p2 = quad_bcast<2>(lo_a);
        const int hi0 = p0 + quad_bcast<0>(len_a), hi1 = p1 + quad_bcast<1>(len_a), hi2 = p2 + quad_bcast<2>(len_a);
        p0 += sub; p1 += sub; p2 += sub;
        const int last = n - 1;
        for (;;) {
            const float4 a0 = record(min(p0, last)), b0 = record(min(p0 + CL, last));
            const float4 a1 = record(min(p1, last)), b1 = record(min(p1 + CL, last));
            const float4 a2 = record(min(p2, last)), b2 = record(min(p2 + CL, last));
            __builtin_amdgcn_sched_barrier(0);
            const ogc_v2f d0 = sqdist_pair(ogc_v2f{a0.x, b0.x}, ogc_v2f{a0.y, b0.y}, ogc_v2f{a0.z, b0.z}, me.x, me.y, me.z);
            slots(p0 < hi0, d0.x <= lim2, p0 + CL < hi0, d0.y <= lim2, key_of(d0.x, a0.w), key_of(d0.y, b0.w));
            const ogc_v2f d1 = sqdist_pair(ogc_v2f{a1.x, b1.x}, ogc_v2f{a1.y, b1.y}, ogc_v2f{a1.z, b1.z}, me.x, me.y, me.z);
            slots(p1 < hi1, d1.x <= lim2, p1 + CL < hi1, d1.y <= lim2, key_of(d1.x, a1.w), key_of(d1.y, b1.w));
            const ogc_v2f d2 = sqdist_pair(ogc_v2f{a2.x, b2.x}, ogc_v2f{a2.y, b2.y}, ogc_v2f{a2.z, b2.z}, me.x, me.y, me.z);
            slots(p2 < hi2, d2.x <= lim2, p2 + CL < hi2, d2.y <= lim2, key_of(d2.x, a2.w), key_of(d2.y, b2.w));
            p0 += 2 * CL; p1 += 2 * CL; p2 += 2 * CL;
            if (__builtin_amdgcn_ballot_w64(p0 < hi0 || p1 < hi1 || p2 < hi2) == 0ull) break;
        }
    } else
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
            // (query - candidate) squared, summed as (x + y) + z: the expression of knn_grid_kernel / the reference, per half
            const ogc_v2f d = sqdist_pair(ogc_v2f{ca[i].x, cb[i].x}, ogc_v2f{ca[i].y, cb[i].y}, ogc_v2f{ca[i].z, cb[i].z},
                                          me.x, me.y, me.z);
            const int p = lo[i] + sub;
            slots(p < hi[i], d.x <= lim2, p + CL < hi[i], d.y <= lim2, key_of(d.x, ca[i].w), key_of(d.y, cb[i].w));
            int pp = p + 2 * CL;
            while (__builtin_amdgcn_ballot_w64(pp < hi[i]) != 0ull) { // a run longer than eight candidates
                const float4 a = record(min(pp, n - 1)), c2 = record(min(pp + CL, n - 1));
                const ogc_v2f d2 = sqdist_pair(ogc_v2f{a.x, c2.x}, ogc_v2f{a.y, c2.y}, ogc_v2f{a.z, c2.z}, me.x, me.y, me.z);
                slots(pp < hi[i], d2.x <= lim2, pp + CL < hi[i], d2.y <= lim2, key_of(d2.x, a.w), key_of(d2.y, c2.w));
                pp += 2 * CL;
            }
        }
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
    const int q = __float_as_int(me.w);
    if (cnt > BQ_FAST) { // more keys than the register sort holds: the row goes to knn_grid_kernel
        if (sub == 0 && q >= 0) {
            idx_out[((size_t)b * n + q) * K] = -1;
            hdrs[b].pending = 1;
        }
    }
    u64 x[8];
    {
        const int4 *l4 = reinterpret_cast<const int4 *>(mine + sub * 8);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int4 v = l4[i];
            x[2 * i] = ((u64)(unsigned)v.y << 32) | (unsigned)v.x;
            x[2 * i + 1] = ((u64)(unsigned)v.w << 32) | (unsigned)v.z;
        }
    }
    // bitonic network over 4 lanes x 8 keys, element e = 8 * lane + register, every exchange ascending (see ball_query_cells_kernel)
#define OGC_KQ_INTRA(MASK)                                                  \
    _Pragma("unroll") for (int r_ = 0; r_ < 8; ++r_)                        \
        if ((r_ ^ (MASK)) > r_) {                                           \
            const u64 a_ = x[r_], b_ = x[r_ ^ (MASK)];                      \
            x[r_] = a_ < b_ ? a_ : b_;                                      \
            x[r_ ^ (MASK)] = a_ < b_ ? b_ : a_;                             \
        }
#define OGC_KQ_INTER(QP, RMASK, UPPER)                                                                              \
    {                                                                                                               \
        u64 p_[8];                                                                                                  \
        _Pragma("unroll") for (int r_ = 0; r_ < 8; ++r_) {                                                          \
            const u64 v_ = x[r_ ^ (RMASK)];                                                                         \
            const unsigned lo_ = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)v_, QP, 0xF, 0xF, true);   \
            const unsigned hi_ = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(v_ >> 32), QP, 0xF, 0xF, true); \
            p_[r_] = ((u64)hi_ << 32) | lo_;                                                                        \
        }                                                                                                           \
        _Pragma("unroll") for (int r_ = 0; r_ < 8; ++r_) {                                                          \
            const bool mine_less_ = x[r_] < p_[r_];                                                                 \
            x[r_] = (mine_less_ != (UPPER)) ? x[r_] : p_[r_];                                                       \
        }                                                                                                           \
    }
    const bool odd = (sub & 1) != 0, high = (sub & 2) != 0;
    OGC_KQ_INTRA(1)
    OGC_KQ_INTRA(3) OGC_KQ_INTRA(1)
    OGC_KQ_INTRA(7) OGC_KQ_INTRA(2) OGC_KQ_INTRA(1)
    OGC_KQ_INTER(0xB1, 7, odd) OGC_KQ_INTRA(4) OGC_KQ_INTRA(2) OGC_KQ_INTRA(1)
    OGC_KQ_INTER(0x1B, 7, high) OGC_KQ_INTER(0xB1, 0, odd) OGC_KQ_INTRA(4) OGC_KQ_INTRA(2) OGC_KQ_INTRA(1)
#undef OGC_KQ_INTRA
#undef OGC_KQ_INTER
    const int kept = min(cnt, K);
    const int first = cnt > 0 ? quad_bcast<0>((int)(unsigned)x[0]) : 0;
    // entry j: (sqrt(d2), index) for j < kept, else (+inf, first).  Lane L holds entries 8 L .. 8 L + 7; it writes entries
    // 4 L .. 4 L + 3 and 16 + 4 L .. (64 contiguous bytes per row and store): an exchange inside the quad.
    int vi[8];
    float vd[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const bool real = sub * 8 + r < kept;
        vi[r] = real ? (int)(unsigned)x[r] : first;
        vd[r] = real ? sqrtf(__uint_as_float((unsigned)(x[r] >> 32))) : INFINITY;
    }
    int i1[4], i2[4];
    float d1[4], d2[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int ia1 = __builtin_amdgcn_update_dpp(0, vi[r], 0x50, 0xF, 0xF, true), ib1 = __builtin_amdgcn_update_dpp(0, vi[r + 4], 0x50, 0xF, 0xF, true);
        const int ia2 = __builtin_amdgcn_update_dpp(0, vi[r], 0xFA, 0xF, 0xF, true), ib2 = __builtin_amdgcn_update_dpp(0, vi[r + 4], 0xFA, 0xF, 0xF, true);
        const int da1 = __builtin_amdgcn_update_dpp(0, __float_as_int(vd[r]), 0x50, 0xF, 0xF, true);
        const int db1 = __builtin_amdgcn_update_dpp(0, __float_as_int(vd[r + 4]), 0x50, 0xF, 0xF, true);
        const int da2 = __builtin_amdgcn_update_dpp(0, __float_as_int(vd[r]), 0xFA, 0xF, 0xF, true);
        const int db2 = __builtin_amdgcn_update_dpp(0, __float_as_int(vd[r + 4]), 0xFA, 0xF, 0xF, true);
        i1[r] = odd ? ib1 : ia1;
        i2[r] = odd ? ib2 : ia2;
        d1[r] = __int_as_float(odd ? db1 : da1);
        d2[r] = __int_as_float(odd ? db2 : da2);
    }
    if (q >= 0 && cnt <= BQ_FAST) {
        const size_t base = ((size_t)b * n + q) * K;
        const int j0 = sub * 4;
        if (j0 < K) {
            *reinterpret_cast<int4 *>(idx_out + base + j0) = make_int4(i1[0], i1[1], i1[2], i1[3]);
            *reinterpret_cast<float4 *>(dist_out + base + j0) = make_float4(d1[0], d1[1], d1[2], d1[3]);
        }
        if (16 + j0 < K) {
            *reinterpret_cast<int4 *>(idx_out + base + 16 + j0) = make_int4(i2[0], i2[1], i2[2], i2[3]);
            *reinterpret_cast<float4 *>(dist_out + base + 16 + j0) = make_float4(d2[0], d2[1], d2[2], d2[3]);
        }
    }
}

} // namespace ogc_grid

using namespace ogc_grid;

// OGC_KNN_CELLS=0 in the environment: knn_grid_kernel alone (A/B runs, tests of both paths)
static bool ogc_knn_cells_enabled() {
    const char *e = getenv("OGC_KNN_CELLS");
    return !(e && e[0] == '0');
}

namespace {
constexpr int KNN_GRID_MIN_POINTS = 256; // smallest cloud searched through cells (ogc_knn_grid)
constexpr int KNN_WAVE_MAX_K = 32;       // longest row of knn_wave_kernel (one key per lane after the threshold: k .. 64 candidates)

// d2 <= lim2  <=>  sqrtf(d2) <= radius: the largest float whose correctly rounded root does not exceed the radius
float knn_radius_limit2(int mode, float radius) {
    float lim2 = INFINITY;
    if (mode == 1 && radius >= 0.0f) {
        lim2 = radius * radius;
        while (lim2 > 0.0f && sqrtf(lim2) > radius) lim2 = nextafterf(lim2, 0.0f);
        for (int it = 0; it < 4; ++it) {
            const float up = nextafterf(lim2, INFINITY);
            if (up < INFINITY && sqrtf(up) <= radius) lim2 = up;
        }
    }
    return lim2;
}

template <int MODE, int SUBT>
void launch_knn_grid(int b, int n, int m, int k, float radius, float lim2, int deferred, const float *unknown, GridHdr *hdrs,
                     int *cell_start, float4 *sorted_pts, float *dist, int *idx, hipStream_t s) {
    hipLaunchKernelGGL((knn_grid_kernel<MODE, SUBT>), dim3(ogc_divup(n, OGC_WAVE / SUBT), b), dim3(OGC_WAVE), knn_grid_lds(k), s, n, m, k,
                       radius, lim2, STRIDE_CELLS, deferred, unknown, hdrs, cell_start, sorted_pts, dist, idx);
}

// the query kernels of ogc_knn / ogc_knn_clamped on a built grid.  cells: four lanes per query over the 27 cells around it first;
// knn_grid_kernel afterwards only does what that kernel left (marked rows, clouds flagged knn_general)
int launch_knn(const GridLayout &L, void *grid, int mode, int b, int n, int m, int k, float radius, bool cells, const float *unknown,
               float *dist, int *idx, hipStream_t s, bool wave = false) {
    GridHdr *hdrs = L.hdrs(grid);
    int *cell_start = L.cell_start(grid);
    float4 *sorted_pts = L.sorted_pts(grid);
    const int stride_cells = STRIDE_CELLS;
    const float lim2 = knn_radius_limit2(mode, radius);
    int deferred = 0;
    if (cells) {
        const dim3 grid4(ogc_divup(n, CPW), b);
        const size_t lds4 = sizeof(u64) * CPW * KQ_LIST;
#define OGC_KNN_CELLS(K)                                                                                              \
    hipLaunchKernelGGL(knn_cells_kernel<K>, grid4, dim3(OGC_WAVE), lds4, s, n, lim2, stride_cells, hdrs, cell_start, \
                       sorted_pts, dist, idx)
        if (k == 32) OGC_KNN_CELLS(32);          // the row lengths of the configs' smoothness terms (4 / 8: flow losses, OGC-DR)
        else if (k == 16) OGC_KNN_CELLS(16);
        else if (k == 8) OGC_KNN_CELLS(8);
        else OGC_KNN_CELLS(4);
#undef OGC_KNN_CELLS
        deferred = 1;
    } else if (wave) {
        // the whole wavefront on one query at a time (k <= 32); knn_grid_kernel afterwards does the rows it marked
        const long long queries = (long long)b * n;
        int qpw = (int)(queries / 8192);
        qpw = qpw < 1 ? 1 : (qpw > 8 ? 8 : qpw);
        const dim3 gridw(ogc_divup(n, qpw), b);
        if (mode == 1)
            hipLaunchKernelGGL(knn_wave_kernel<1>, gridw, dim3(OGC_WAVE), 0, s, n, m, k, radius, stride_cells, qpw, unknown, hdrs,
                               cell_start, sorted_pts, dist, idx);
        else
            hipLaunchKernelGGL(knn_wave_kernel<0>, gridw, dim3(OGC_WAVE), 0, s, n, m, k, radius, stride_cells, qpw, unknown, hdrs,
                               cell_start, sorted_pts, dist, idx);
        deferred = 2;
    }
    // sixteen lanes per query (four queries per wavefront) when eight would leave most SIMDs without a wavefront: the launch's time
    // is then one wavefront's serial work (FlowStep3D at B = 1: 4096 queries = 512 wavefronts of ~48 us; forward 7.45 -> 7.07 ms).
    // (measured, tools/bench_ops.py --ops knn,knnc, 8 -> 16 lanes: 1 x 8192 x 8192, k = 32 0.079 -> 0.056 ms; 16 x 2048 <- 8192, k = 64
    // 0.264 -> 0.238; 16 x 512 <- 1024, k = 64 0.190 -> 0.116; but 16 x 8192 x 8192 0.240 -> 0.249, and the radius-limited searches,
    // which keep a handful of candidates, lose from 2048 wavefronts on: 16 x 1024 <- 2048 0.037 -> 0.042)
    const bool limited = mode == 1 && radius >= 0.0f;
    const long long waves8 = (long long)b * ogc_divup(n, QPW);
    const bool wide = waves8 <= (limited ? 1024 : 4096);
    // ... and thirty-two (two queries per wavefront) for the smallest launches (FlowStep3D's 2048-point levels at B = 1)
    const bool wider = waves8 <= (limited ? 256 : 1024); // (1 x 8192 x 8192: 0.056 -> 0.050 ms)
    const auto launch = mode == 1 ? (wider ? launch_knn_grid<1, 32> : wide ? launch_knn_grid<1, 16> : launch_knn_grid<1, 8>)
                                  : (wider ? launch_knn_grid<0, 32> : wide ? launch_knn_grid<0, 16> : launch_knn_grid<0, 8>);
    launch(b, n, m, k, radius, lim2, deferred, unknown, hdrs, cell_start, sorted_pts, dist, idx, s);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        ogc_set_error("ogc_knn (grid): launch failed: %s", hipGetErrorString(e));
        return OGC_ERR_LAUNCH;
    }
    return OGC_OK;
}

bool knn_cells_applies(int mode, int n, int m, int k, float radius, bool same) {
    return mode == 1 && radius > 0.0f && radius < 1.0e18f && same && n == m && (k == 4 || k == 8 || k == 16 || k == 32) &&
           ogc_knn_cells_enabled();
}
} // namespace

// k-NN over cell lists.  Returns OGC_OK after queueing build + query, or OGC_ERR_UNSUPPORTED (caller: all-pairs scan).
int ogc_knn_grid(int mode, int b, int n, int m, int k, float radius, const float *unknown, const float *known,
                 float *dist, int *idx, hipStream_t s) {
    // below KNN_GRID_MIN_POINTS (1024 until round 4) the all-pairs scan, one lane per query — at B = 1 a 512-point level of
    // FlowStep3D is 16 wavefronts scanning for 160 us, against ~60 us of build + search here (forward 7.70 -> 7.55 ms)
    if (m < KNN_GRID_MIN_POINTS || m <= 4 * k || knn_grid_lds(k) > 64 * 1024) return OGC_ERR_UNSUPPORTED;
    const GridLayout L(b, m);
    void *ws = ogc_workspace(s, L.total());
    if (!ws) return OGC_ERR_UNSUPPORTED;
    // radius-limited search of a cloud in itself (the smoothness term's neighbour lists): the build then prefers cells of edge
    // 1.01 r when balls are sparsely filled
    const bool cells = knn_cells_applies(mode, n, m, k, radius, unknown == known);
    // points per cell = k / knn_div
    // 33.5 = cell edge of half the expected k-th neighbour distance.  The first block's 128-key sort wants ~120 candidates in its 125
    // cells; where the cloud is denser than its bounding box suggests (scenes: ground, objects) a block holds more and the query falls
    // back to insertion, so full launches on scene-like clouds want SMALLER cells, while a launch that leaves the chip under-filled
    // (one wavefront's latency) wants fewer, fuller cells.  Measured (ms; uniform slab / synthetic scene, 16 x 8192 x 8192):
    //   k = 32: div 28 0.219 / 0.374, 33.5 0.240 / 0.305, 40 0.263 / 0.279;  k = 64: 33.5 - / 1.234, 40 - / 1.026, 48 - / 0.872
    //   (16 x 2048 <- 8192, k = 64: 33.5 0.239 / 0.453, 48 0.205 / 0.346);  1 x 8192 x 8192, k = 32: 28 0.044 / 0.043, 33.5 0.050 / 0.050
    const bool small_launch = (long long)b * ogc_divup(n, QPW) <= 1024;
    float knn_div = 33.5f;
    if (small_launch) knn_div = (k >= 24 && k <= 40) ? 28.0f : 33.5f;
    else if (k >= 56) knn_div = m >= 4096 ? 48.0f : 33.5f;
    // (k = 24..40 on full launches stays at 33.5: 40 trades 0.305 -> 0.281 on scenes for 0.240 -> 0.264 on uniform clouds and 0.257 -> 0.309
    // at 8 x 16384 x 16384)
    // k <= 32 outside the radius-limited self search: a wavefront per query over cells of k / 16 points (knn_wave_kernel)
    const bool wave = !cells && k <= KNN_WAVE_MAX_K;
    if (wave) knn_div = -(7.0f * (float)k < 230.0f ? 7.0f * (float)k : 230.0f);
    launch_grid_build(b, m, mode == 1 ? radius : 0.0f, k, STRIDE_CELLS, known, L.hdrs(ws), L.cell_start(ws), L.sorted_pts(ws), s,
                      cells ? 1 : 0, knn_div);
    return launch_knn(L, ws, mode, b, n, m, k, radius, cells, unknown, dist, idx, s, wave);
}

// ---- the radius-limited search on a grid built by ogc_cell_grid_build (fused extension, include/ogc_ops.h) --------------------------
extern "C" int ogc_knn_clamped_cells(int b, int n, int k, float radius, const float *xyz, void *grid, float grid_radius, float *dist,
                                     int *idx, ogc_stream_t stream) {
    OGC_REQUIRE(b >= 0 && n >= 0 && k >= 1, "ogc_knn_clamped_cells: bad dimension");
    if (b == 0 || n == 0) return OGC_OK;
    OGC_REQUIRE(xyz && grid && dist && idx, "ogc_knn_clamped_cells: null pointer");
    if (!(radius > 0.0f) || !(radius <= grid_radius) || n < 1024 || n <= 4 * k || knn_grid_lds(k) > 64 * 1024) {
        ogc_set_error("ogc_knn_clamped_cells: needs 0 < radius <= the grid's radius (%g vs %g), n >= 1024, n > 4 k", (double)radius,
                      (double)grid_radius);
        return OGC_ERR_UNSUPPORTED;
    }
    return launch_knn(GridLayout(b, n), grid, 1, b, n, n, k, radius, knn_cells_applies(1, n, n, k, radius, true), xyz, dist, idx,
                      (hipStream_t)stream);
}

// three_nn over cell lists.  OGC_OK after queueing build + query, OGC_ERR_UNSUPPORTED when the caller should run its scan
// (few known points: the scan is as fast).
int ogc_three_nn_grid(int b, int n, int m, const float *unknown, const float *known, float *dist2, int *idx, hipStream_t s) {
    if (m < 1024) return OGC_ERR_UNSUPPORTED;
    const GridLayout L(b, m);
    void *ws = ogc_workspace(s, L.total());
    if (!ws) return OGC_ERR_UNSUPPORTED;
    // density: 3 / 2 = 1.5 points per cell — the ball of radius h around a target (what the first block covers) then holds
    // ~6 of them, three or more for ~95 % of the targets
    launch_grid_build(b, m, 0.0f, 3, STRIDE_CELLS, known, L.hdrs(ws), L.cell_start(ws), L.sorted_pts(ws), s, 0, 2.0f);
    hipLaunchKernelGGL(three_nn_grid_kernel, dim3(ogc_divup(n, OGC_WAVE), b), dim3(OGC_WAVE), 0, s, n, m, STRIDE_CELLS, unknown,
                       L.hdrs(ws), L.cell_start(ws), L.sorted_pts(ws), dist2, idx);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        ogc_set_error("ogc_three_nn (grid): launch failed: %s", hipGetErrorString(e));
        return OGC_ERR_LAUNCH;
    }
    return OGC_OK;
}

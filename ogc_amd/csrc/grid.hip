// grid.hip — the uniform grid (cell lists) behind the fixed-radius query and the k-NN searches, whose results are identical to
// the brute-force scans.  The searches themselves: grid_ball_query.hip, grid_knn.hip; what the three share: grid_dev.h.
//
// The reference's ball query (ball_query_gpu.cu:9-45) tests every centre against every point: 8*N*M flop for
// ~2.3 MB of input/output per 8192-point cloud, i.e. compute-bound by two orders of magnitude.  A radius query only
// needs the points of the 27 cells around the centre when the cell edge is >= the radius.  Per call:
//   grid_build_kernel   one workgroup per cloud, the cloud held in registers: bounding box -> cell edge h >= 1.01 r
//                       (enlarged until the grid has <= GRID_MAX_CELLS cells; density-based for k-NN) -> LDS
//                       histogram -> scan -> scatter: cell_start[], and the points re-ordered by cell as 16-byte
//                       records (x, y, z, index), so a query reads a candidate with one load from a contiguous run
//                       (grid_build_split_kernel: the same by several workgroups per cloud).
// Exactness: a hit satisfies |dx| < r in every axis, the cell coordinate is floor((x - min) / h) with h >= 1.01 r, so
// the cell coordinates of a centre and any of its hits differ by at most one even with fp32 rounding of the
// quotient (relative error 1e-7 * up to 16384 cells << 0.01); points with non-finite coordinates can never be
// hits (their distance is inf/NaN) and are left out of the grid.
#include <stdlib.h>

#include "grid_dev.h"

namespace ogc_grid {

constexpr int BUILD_THREADS = 1024;

// v^(1/dims) for the cell edge
__device__ __forceinline__ float dims_root(float v, int dims) { return dims == 1 ? v : (dims == 2 ? sqrtf(v) : cbrtf(v)); }

// Grid parameters from the bounding box, by ONE lane per workgroup, in single precision: the edge only steers which candidates
// a search meets.  What the searches rely on holds for ANY origin, edge and cell counts: cell = min(floor((x - min) / h), g - 1)
// clamped at 0 is monotone in x, so two points closer than r <= h / 1.01 along an axis are at most one cell apart (a 1 % margin
// against the 1e-7 relative error of the fp32 quotient and of r * 1.01f itself).  (This used to be double-precision pow / cbrt /
// division chains: ~2200 cycles on the one lane everybody waits for; now ~a quarter.)
__device__ __forceinline__ GridHdr grid_header(const float (&lo)[3], const float (&hi)[3], int n, float radius,
                                               int knn_k, float knn_div, int prefer_cells) {
    GridHdr h;
    bool cells_ok = false;
    const bool any = lo[0] <= hi[0];
    float ext[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) ext[a] = any ? fminf(hi[a] - lo[a], 3.0e38f) : 0.0f; // (a difference of finite numbers may overflow)
    float edge = radius * 1.01f;
    const float maxext = fmaxf(ext[0], fmaxf(ext[1], ext[2]));
    if (knn_k > 0) {
        // k-NN mode: pick the edge from the mean density so that the 3^d block around a query holds ~2.5 k points
        // (d = number of axes with a non-negligible extent: flat or linear clouds get fewer cells per block)
        int dims = 0;
        float vol = 1.0f;
#pragma unroll
        for (int a = 0; a < 3; ++a)
            if (ext[a] > 1e-3f * maxext && ext[a] > 0.0f) { ++dims; vol *= ext[a]; }
        // cell edge = HALF the expected distance of the k-th neighbour (rho h^d = k / (V_d 2^d), V_d the unit ball): the
        // search then ends after the 5^d block (R = 2), ~3.7 k candidates in 3-D, where an edge of 0.73 r_k (the former
        // 2.5 k points per 3^d block) also needed R = 2 but scanned 11.6 k
        const float inv_n = 1.0f / (float)max(n, 1);
        const float per_cell = fmaxf((float)knn_k / (dims == 3 ? knn_div : (dims == 2 ? 12.6f : 4.0f)), 0.5f);
        edge = dims > 0 ? dims_root(vol * per_cell * inv_n, dims) : 1.0f;
        if (knn_div < 0.0f && dims > 0) {
            // knn_wave_kernel: the edge that puts ~(-knn_div) points into the query's block of five cells per axis CLIPPED to the
            // bounding box — a road scene 4 m high is two or three cells thick whatever the edge, so the block is a slab and its
            // cells may be much longer than the mean density of the box suggests (which counts a ball that the slab cuts off)
            const float target = -knn_div;
            const float rho = (float)max(n, 1) / vol;
            edge = dims_root(target / (rho * (dims == 3 ? 125.0f : (dims == 2 ? 25.0f : 5.0f))), dims);
            for (int it = 0; it < 3; ++it) {
                float fixed = 1.0f;
                int freed = 0;
#pragma unroll
                for (int a = 0; a < 3; ++a)
                    if (ext[a] > 1e-3f * maxext && ext[a] > 0.0f) {
                        if (5.0f * edge >= ext[a]) fixed *= ext[a]; else ++freed;
                    }
                if (freed == 0) break;
                edge = dims_root(target / (rho * fixed * (freed == 3 ? 125.0f : (freed == 2 ? 25.0f : 5.0f))), freed);
            }
        }
        // radius-clamped search (ogc_knn_clamped): neighbours beyond `radius` are replaced by the nearest one anyway,
        // so the search may stop once the scanned block covers the radius.  When the radius is SHORTER than the
        // density-based edge, cells of edge 1.01 r make that one shell of far fewer candidates (but never less than
        // ~one point per cell: the nearest neighbour of a query in an empty region must still be found by shells).
        if (radius > 0.0f && radius < 3.0e38f && dims > 0) {
            const float one_per_cell = dims_root(vol * inv_n, dims);
            const float limited = fmaxf(radius * 1.01f, one_per_cell);
            if (limited < edge) edge = limited;
            // A radius-limited search of the cloud in itself (prefer_cells): when a ball holds few points (mean <= 18 at the
            // mean density) knn_cells_kernel finds them all in the 27 cells of edge 1.01 r around a query and sorts them in
            // registers — the ball query's grid, far fewer candidates than the shells of the density-based one.
            if (prefer_cells && radius < 1.0e12f) {
                const float r = radius;
                const float ball = dims == 3 ? 4.18879f * r * r * r : (dims == 2 ? 3.14159f * r * r : 2.0f * r);
                if ((float)n * ball <= 18.0f * vol) {
                    edge = fmaxf(edge, r * 1.01f); // (no finer than the density asks for: the build's cost grows with the cell count)
                    cells_ok = true;
                }
            }
        }
    }
    if (!(edge > 0.0f) || !isfinite(edge)) edge = fmaxf(maxext, 1.0f);    // degenerate: one cell per axis
    edge = fmaxf(edge, maxext * 1e-6f);                                   // keep the quotient well inside int range
    float g0 = 1.0f, g1 = 1.0f, g2 = 1.0f;
    for (int it = 0; it < 64; ++it) {
        const float inv = 1.0f / edge;
        g0 = floorf(ext[0] * inv) + 1.0f; g1 = floorf(ext[1] * inv) + 1.0f; g2 = floorf(ext[2] * inv) + 1.0f;
        const float total = g0 * g1 * g2;
        if (total <= (float)GRID_MAX_CELLS) break;
        edge *= cbrtf(total * (1.0f / (float)GRID_MAX_CELLS)) * 1.02f;
    }
    // Cell order.  A radius search visits the cells (x - 1 .. x + 1, y - 1 .. y + 1, z - 1 .. z + 1): nine runs of the
    // cell-sorted array when x runs fastest.  When one axis has at most two cells (a road scene a few metres high searched with
    // r = 2 m) and THAT axis runs fastest, the cells (all of it, y - 1 .. y + 1) of one z are contiguous: three runs, three
    // times as long — the query kernels' cost is per run, not per candidate.  Otherwise x stays the fastest axis.
    int fast = 0;
    if (knn_k == 0 || prefer_cells != 0) {
        if (g0 > 2.0f && g1 <= 2.0f && g1 <= g2) fast = 1;
        else if (g0 > 2.0f && g2 <= 2.0f) fast = 2;
    }
    // (fast, mid, slow) = (x, y, z) | (y, x, z) | (z, x, y)
    const float l0 = any ? lo[0] : 0.f, l1 = any ? lo[1] : 0.f, l2 = any ? lo[2] : 0.f;
    h.minx = fast == 0 ? l0 : (fast == 1 ? l1 : l2);
    h.miny = fast == 0 ? l1 : l0;
    h.minz = fast == 2 ? l1 : l2;
    h.inv_h = 1.0f / edge;
    h.gx = (int)(fast == 0 ? g0 : (fast == 1 ? g1 : g2));
    h.gy = (int)(fast == 0 ? g1 : g0);
    h.gz = (int)(fast == 2 ? g1 : g2);
    h.fast = fast;
    h.slab = h.gx <= 2 ? 1 : 0;
    h.npts = 0;
    h.dense = 0;
    h.heavy = 0;
    h.knn_general = (cells_ok || prefer_cells == 2) ? 0 : 1;   // (2: a grid shared by several searches, built for their largest radius)
    h.pending = 0;
    return h;
}

// One workgroup per cloud.  PPT > 0: every thread keeps its PPT points (and their cells) in registers, so the cloud
// is read from memory once; PPT == 0: any size, the three passes re-read the cloud.  Five barriers in all: the
// bounding box and the cell-count scan are wave-level (DPP / shuffles) with one 16-entry exchange through LDS each.
template <int PPT>
__global__ __launch_bounds__(BUILD_THREADS) void grid_build_kernel(float knn_div, int n, float radius, int knn_k, int prefer_cells,
                                                                   int stride_cells,
                                                                   const float *__restrict__ xyz,
                                                                   GridHdr *__restrict__ hdrs,
                                                                   int *__restrict__ cell_start,
                                                                   float4 *__restrict__ sorted_pts) {
    __shared__ int s_cnt[GRID_MAX_CELLS]; // histogram -> exclusive starts -> scatter cursors
    __shared__ float s_red[6][BUILD_THREADS / 64];
    __shared__ int s_wave[BUILD_THREADS / 64];
    __shared__ int s_tail; // cursor for points left out of the grid (non-finite coordinates)
    __shared__ GridHdr s_hdr;
    constexpr int R = PPT > 0 ? PPT : 1;
    const int t = threadIdx.x, b = blockIdx.x, lane = t & 63, wave = t >> 6;
    const float *pts = xyz + (size_t)b * n * 3;
    float px[R], py[R], pz[R];
    int cell[R];

    OGC_PROBE_BUILD(0);
    // 1. load + bounding box of the finite points
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    auto widen = [&](float x, float y, float z) {
        if (isfinite(x) && isfinite(y) && isfinite(z)) {
            mn[0] = fminf(mn[0], x); mn[1] = fminf(mn[1], y); mn[2] = fminf(mn[2], z);
            mx[0] = fmaxf(mx[0], x); mx[1] = fmaxf(mx[1], y); mx[2] = fmaxf(mx[2], z);
        }
    };
    // (PPT > 0: thread t owns the points t * PPT .. t * PPT + PPT - 1 — 3 PPT consecutive floats, read as 16-byte
    // loads when the cloud's size and base allow it: 6 loads instead of 24 strided ones for PPT = 8)
    if (PPT > 0) {
        const bool wide = PPT % 4 == 0 && (n & 3) == 0 && (((size_t)(const void *)pts) & 15) == 0;
        if (wide && (t + 1) * R <= n) {
            float f[3 * R];
            const float4 *p4 = reinterpret_cast<const float4 *>(pts + (size_t)t * R * 3);
#pragma unroll
            for (int i = 0; i < 3 * R / 4; ++i) {
                const float4 v = p4[i];
                f[4 * i] = v.x; f[4 * i + 1] = v.y; f[4 * i + 2] = v.z; f[4 * i + 3] = v.w;
            }
#pragma unroll
            for (int i = 0; i < R; ++i) { px[i] = f[3 * i]; py[i] = f[3 * i + 1]; pz[i] = f[3 * i + 2]; }
        } else {
#pragma unroll
            for (int i = 0; i < R; ++i) {
                const int k = t * R + i;
                px[i] = py[i] = pz[i] = NAN;
                if (k < n) { px[i] = pts[k * 3]; py[i] = pts[k * 3 + 1]; pz[i] = pts[k * 3 + 2]; }
            }
        }
    }
    for (int c = t; c < GRID_MAX_CELLS; c += BUILD_THREADS) s_cnt[c] = 0; // overlaps the loads
    if (PPT > 0) {
#pragma unroll
        for (int i = 0; i < R; ++i) widen(px[i], py[i], pz[i]);
    } else {
        for (int k = t; k < n; k += BUILD_THREADS) widen(pts[k * 3], pts[k * 3 + 1], pts[k * 3 + 2]);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float lo = -ogc_wave_max_f32(-mn[a]), hi = ogc_wave_max_f32(mx[a]);
        if (lane == 0) { s_red[a][wave] = lo; s_red[3 + a][wave] = hi; }
    }
    OGC_PROBE_BUILD(1);
    __syncthreads();
    OGC_PROBE_BUILD(2);
    // the grid parameters are derived ONCE (double-precision pow / cbrt / floor loops: hundreds of instructions that
    // used to run on all 1024 threads of the one CU a cloud gets) and handed to the others through LDS
    if (wave == 0) {
        float lo[3], hi[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float l = lane < BUILD_THREADS / 64 ? s_red[a][lane] : INFINITY;
            const float u = lane < BUILD_THREADS / 64 ? s_red[3 + a][lane] : -INFINITY;
            lo[a] = -ogc_wave_max_f32(-l);
            hi[a] = ogc_wave_max_f32(u);
        }
        if (lane == 0) s_hdr = grid_header(lo, hi, n, radius, knn_k, knn_div, prefer_cells);
    }
    __syncthreads();
    OGC_PROBE_BUILD(3);
    GridHdr h = s_hdr;
    const int ncell = h.gx * h.gy * h.gz;
    // (a finite coordinate: the float -> int conversion saturates where cell_coord clamps to [-2, g + 1], and the clamp to
    // the grid follows either way — the same cell, without cell_coord's two branches per axis)
    auto cell_of = [&](float x, float y, float z) -> int {
        OGC_GRID_AXES(h, x, y, z, fx, fy, fz);
        const int cx = min(cell_floor(fx, h.minx, h.inv_h), h.gx - 1);
        const int cy = min(cell_floor(fy, h.miny, h.inv_h), h.gy - 1);
        const int cz = min(cell_floor(fz, h.minz, h.inv_h), h.gz - 1);
        return (isfinite(x) && isfinite(y) && isfinite(z)) ? cx + h.gx * (cy + h.gy * cz) : -1;
    };

    // 2. histogram (LDS atomics)
    if (PPT > 0) {
#pragma unroll
        for (int i = 0; i < R; ++i) {
            cell[i] = (t * R + i < n) ? cell_of(px[i], py[i], pz[i]) : -2;
            if (cell[i] >= 0) atomicAdd(&s_cnt[cell[i]], 1);
        }
    } else {
        for (int k = t; k < n; k += BUILD_THREADS) {
            const int c = cell_of(pts[k * 3], pts[k * 3 + 1], pts[k * 3 + 2]);
            if (c >= 0) atomicAdd(&s_cnt[c], 1);
        }
    }
    __syncthreads();
    OGC_PROBE_BUILD(4);

    // 3. exclusive scan of s_cnt[0..ncell): a contiguous chunk per thread, wave scan of the chunk sums, wave totals
    const int per = (ncell + BUILD_THREADS - 1) / BUILD_THREADS;
    const int c0 = min(t * per, ncell), c1 = min(c0 + per, ncell);
    int sum = 0;
    for (int c = c0; c < c1; ++c) sum += s_cnt[c];
    int incl = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int up = __shfl_up(incl, off, 64);
        if (lane >= off) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    OGC_PROBE_BUILD(5);
    int before = 0, npts = 0;
#pragma unroll
    for (int w = 0; w < BUILD_THREADS / 64; ++w) {
        const int v = s_wave[w];
        if (w < wave) before += v;
        npts += v;
    }
    int run = before + incl - sum;
    int *cs = cell_start + (size_t)b * stride_cells;
    for (int c = c0; c < c1; ++c) {
        const int cnt = s_cnt[c];
        s_cnt[c] = run; // becomes the scatter cursor
        cs[c] = run;
        run += cnt;
    }
    if (t == 0) {
        cs[ncell] = npts;
        s_tail = npts;
        h.npts = npts;
        // mean number of candidates a centre would test (27 cells at the mean occupancy).  When that is a large share
        // of the cloud the cell lists buy nothing, and rows saturate early, which an index-ordered scan exploits (it
        // stops after nsample hits) while a cell-ordered scan cannot.
        const float per_query = 27.0f * (float)npts / (float)ncell;
        h.dense = per_query > 0.25f * (float)n ? 1 : 0;
        // ball_query_cells_kernel sorts lists of up to 32 hits: with full cells around it a centre has ~0.15 * per_query hits
        // (ball / 27 cells), so beyond a mean of ~18 too many wavefronts would have to repeat their work in the general body
        h.heavy = per_query > 120.0f ? 1 : 0;
        // knn_cells_kernel (radius-limited search over the 27 cells around a query) needs cells at least as long as the radius —
        // the same bound knn_grid_kernel stops its shells with — and lists that fit its register sort
        if (!(1.0f * (1.0f / h.inv_h) * 0.999f >= radius) || per_query > 120.0f) h.knn_general = 1;
        hdrs[b] = h;
    }
    __syncthreads();
    OGC_PROBE_BUILD(6);

    // 4. scatter (order inside a cell is arbitrary; the queries order their results themselves).  One 16-byte record
    //    per point: x, y, z and the point's index (bit pattern), so a query reads a candidate with a single load.
    //    Points with non-finite coordinates are in no cell; they are listed after the cells so that a same-set query
    //    still emits their (empty) rows.
    float4 *sp = sorted_pts + (size_t)b * n;
    if (PPT > 0) {
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const int k = t * R + i;
            if (cell[i] >= 0) sp[atomicAdd(&s_cnt[cell[i]], 1)] = make_float4(px[i], py[i], pz[i], __int_as_float(k));
            else if (cell[i] == -1) sp[atomicAdd(&s_tail, 1)] = make_float4(NAN, NAN, NAN, __int_as_float(k));
        }
    } else {
        for (int k = t; k < n; k += BUILD_THREADS) {
            const float x = pts[k * 3], y = pts[k * 3 + 1], z = pts[k * 3 + 2];
            const int c = cell_of(x, y, z);
            if (c >= 0) sp[atomicAdd(&s_cnt[c], 1)] = make_float4(x, y, z, __int_as_float(k));
            else sp[atomicAdd(&s_tail, 1)] = make_float4(NAN, NAN, NAN, __int_as_float(k));
        }
    }
    OGC_PROBE_BUILD(7);
}

// The same build by SEVERAL workgroups per cloud, with nothing exchanged between them.  One workgroup per cloud is one CU per
// cloud: 16 of 256 CUs for a batch of 16, each pushing 8192 16-byte records and the cell starts through its own store path
// (the launch ends when those drain), its histogram and scatter serialised on one LDS.  Here every workgroup of a cloud reads
// the WHOLE cloud (L2-resident after the first reader), derives the same bounding box and header, and computes every point's
// cell — but owns only a contiguous range of cells [c_lo, c_hi): it counts the points below its range (its base offset), builds
// the histogram / scan / cursors of its own range in LDS and scatters only the points that fall into it.  No grid barrier, no
// flag: redundant arithmetic instead of communication.  Results: the same cell starts; the order of the points inside a cell
// is arbitrary in both kernels (LDS atomics), which no query depends on.
constexpr int SPLIT_MIN = 8;                                // parts per cloud (at least): a part owns <= GRID_MAX_CELLS / 8 cells
constexpr int SPLIT_CELLS = GRID_MAX_CELLS / SPLIT_MIN;

template <int PPT>
__global__ __launch_bounds__(BUILD_THREADS) void grid_build_split_kernel(float knn_div, int nb, int split, int n, float radius,
                                                                         int knn_k, int prefer_cells, int stride_cells,
                                                                         const float *__restrict__ xyz,
                                                                         GridHdr *__restrict__ hdrs,
                                                                         int *__restrict__ cell_start,
                                                                         float4 *__restrict__ sorted_pts) {
    __shared__ int s_cnt[SPLIT_CELLS]; // histogram -> scatter cursors of the cells [c_lo, c_hi)
    __shared__ float4 s_stage[BUILD_THREADS / 64 * 64 * 6]; // 6 KiB per wavefront: the transposition of the coalesced loads
    __shared__ float s_red[6][BUILD_THREADS / 64];
    __shared__ int s_wave[BUILD_THREADS / 64], s_counts[BUILD_THREADS / 64];
    __shared__ int s_tail;
    __shared__ GridHdr s_hdr;
    static_assert(PPT > 0 && PPT % 8 == 0, "the split build keeps the cloud in registers, eight points per thread and pass");
    const int t = threadIdx.x, b = blockIdx.x % nb, part = blockIdx.x / nb, lane = t & 63, wave = t >> 6;
    const float *pts = xyz + (size_t)b * n * 3;
    float px[PPT], py[PPT], pz[PPT];
    int cell[PPT];
    // thread t owns the points 8192 * pass + 8 t + i (i < 8) of pass = 0 .. PPT / 8 - 1
    auto point_index = [&](int i) { return (i >> 3) * (8 * BUILD_THREADS) + t * 8 + (i & 7); };

    OGC_PROBE_BUILD(0);
    // 1. load + bounding box of the finite points.  A wavefront's 512 points of a pass are 6 KiB of contiguous memory: it
    //    reads them as six fully coalesced 16-byte loads per lane (lane L takes the 16-byte pieces L, L + 64, ...), parks
    //    them in its own LDS strip and reads back the 96 contiguous bytes of ITS eight points.  (Reading those 96 bytes
    //    straight from memory — lanes 96 bytes apart, 48 cache lines per load instruction, every line visited by six
    //    instructions — took 8.7 k cycles for the cloud, i.e. most of the kernel.)
    const bool wide = (n & 3) == 0 && (((size_t)(const void *)pts) & 15) == 0;
    if (wide) {
        float4 *strip = s_stage + wave * (64 * 6);
        const int n4 = n * 3 / 4; // 16-byte pieces of the cloud
#pragma unroll
        for (int pass = 0; pass < PPT / 8; ++pass) {
            const int base4 = (pass * (8 * BUILD_THREADS) + wave * 512) * 3 / 4; // first piece of the wavefront's 512 points
            const float4 *p4 = reinterpret_cast<const float4 *>(pts) + base4;
            float4 v[6];
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                v[j] = make_float4(NAN, NAN, NAN, NAN);
                if (base4 + lane + 64 * j < n4) v[j] = p4[lane + 64 * j];
            }
            if (pass > 0) __builtin_amdgcn_wave_barrier(); // (the strip is read by this wavefront only)
#pragma unroll
            for (int j = 0; j < 6; ++j) strip[lane + 64 * j] = v[j];
            __builtin_amdgcn_s_waitcnt(0xc07f);
            __builtin_amdgcn_wave_barrier();
            float f[24];
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const float4 w = strip[lane * 6 + j];
                f[4 * j] = w.x; f[4 * j + 1] = w.y; f[4 * j + 2] = w.z; f[4 * j + 3] = w.w;
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) { px[pass * 8 + i] = f[3 * i]; py[pass * 8 + i] = f[3 * i + 1]; pz[pass * 8 + i] = f[3 * i + 2]; }
            __builtin_amdgcn_s_waitcnt(0xc07f);
        }
    } else {
#pragma unroll
        for (int i = 0; i < PPT; ++i) {
            const int k = point_index(i);
            px[i] = py[i] = pz[i] = NAN;
            if (k < n) { px[i] = pts[k * 3]; py[i] = pts[k * 3 + 1]; pz[i] = pts[k * 3 + 2]; }
        }
    }
    for (int c = t; c < SPLIT_CELLS; c += BUILD_THREADS) s_cnt[c] = 0;
    // bounding box: minima / maxima of ALL coordinates first (v_min3 / v_max3 ignore NaNs) — three instructions per point
    // instead of twelve — next to a running sum of the coordinates' magnitudes, which is finite iff every coordinate is (or
    // overflows: a false alarm).  A point with a non-finite coordinate is in no cell, and must not lend its other coordinates
    // to the box either (grid_build_kernel takes the box over fully finite points; one stray (NaN, 1e30, 0) would stretch this
    // one until the grid is a single cell): when the sum is not finite the box is taken again over the finite points only
    // (once, all workgroups of the cloud alike).
    bool filtered = false;
    for (;;) {
        float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
        bool odd_one = false; // some coordinate of mine is NaN or infinite
        if (!filtered) {
            float mag0 = 0.0f, mag1 = 0.0f;
#pragma unroll
            for (int i = 0; i < PPT; i += 2) {
                mn[0] = ogc_min3_f32(mn[0], px[i], px[i + 1]); mx[0] = ogc_max3_f32(mx[0], px[i], px[i + 1]);
                mn[1] = ogc_min3_f32(mn[1], py[i], py[i + 1]); mx[1] = ogc_max3_f32(mx[1], py[i], py[i + 1]);
                mn[2] = ogc_min3_f32(mn[2], pz[i], pz[i + 1]); mx[2] = ogc_max3_f32(mx[2], pz[i], pz[i + 1]);
            }
            if (n >= PPT * BUILD_THREADS) { // (wave-uniform: every slot of mine is a point of the cloud)
#pragma unroll
                for (int i = 0; i < PPT; i += 2) {
                    mag0 += (fabsf(px[i]) + fabsf(py[i])) + fabsf(pz[i]);
                    mag1 += (fabsf(px[i + 1]) + fabsf(py[i + 1])) + fabsf(pz[i + 1]);
                }
            } else { // slots beyond n hold NaN fillers of the loads above: they must not raise the alarm
#pragma unroll
                for (int i = 0; i < PPT; ++i)
                    if (point_index(i) < n) mag0 += (fabsf(px[i]) + fabsf(py[i])) + fabsf(pz[i]);
            }
            odd_one = !(mag0 + mag1 < INFINITY);
        } else {
#pragma unroll
            for (int i = 0; i < PPT; ++i) {
                const float x = px[i], y = py[i], z = pz[i];
                if (isfinite(x) && isfinite(y) && isfinite(z)) {
                    mn[0] = fminf(mn[0], x); mn[1] = fminf(mn[1], y); mn[2] = fminf(mn[2], z);
                    mx[0] = fmaxf(mx[0], x); mx[1] = fmaxf(mx[1], y); mx[2] = fmaxf(mx[2], z);
                }
            }
        }
        const bool wave_odd = __builtin_amdgcn_ballot_w64(odd_one) != 0ull;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float lo = -ogc_wave_max_f32(-mn[a]), hi = ogc_wave_max_f32(mx[a]);
            if (lane == 0) { s_red[a][wave] = lo; s_red[3 + a][wave] = hi; }
        }
        if (lane == 0) s_wave[wave] = wave_odd ? 1 : 0; // (s_wave is free until the scan)
        OGC_PROBE_BUILD(1);
        __syncthreads();
        OGC_PROBE_BUILD(2);
        if (wave == 0) {
            float lo[3], hi[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float l = lane < BUILD_THREADS / 64 ? s_red[a][lane] : INFINITY;
                const float u = lane < BUILD_THREADS / 64 ? s_red[3 + a][lane] : -INFINITY;
                lo[a] = -ogc_wave_max_f32(-l);
                hi[a] = ogc_wave_max_f32(u);
            }
            const bool any_odd = __builtin_amdgcn_ballot_w64(lane < BUILD_THREADS / 64 && s_wave[lane] != 0) != 0ull;
            if (lane == 0) {
                s_hdr = grid_header(lo, hi, n, radius, knn_k, knn_div, prefer_cells);
                s_hdr.pending = (any_odd && !filtered) ? 1 : 0; // (borrowed as the "take the box again" flag; 0 when the loop ends)
            }
        }
        __syncthreads();
        if (s_hdr.pending == 0) break;
        filtered = true;
        __syncthreads(); // everybody has read the flag before lane 0 writes the header again
    }
    // (the loop ends behind a barrier: the header is visible)
    OGC_PROBE_BUILD(3);
    GridHdr h = s_hdr;
    const int ncell = h.gx * h.gy * h.gz;
    const int per = (ncell + split - 1) / split;                 // <= SPLIT_CELLS: split >= SPLIT_MIN
    const int c_lo = min(part * per, ncell), c_hi = min(c_lo + per, ncell);

    // 2. cells of ALL points; histogram of my range; how many points lie below it / in the grid at all
    int counts = 0; // valid | below << 16   (n <= 16384: 15 bits each)
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
        const float x = px[i], y = py[i], z = pz[i];
        OGC_GRID_AXES(h, x, y, z, fx, fy, fz);
        const int cx = cell_clamped(fx, h.minx, h.inv_h, h.gx);
        const int cy = cell_clamped(fy, h.miny, h.inv_h, h.gy);
        const int cz = cell_clamped(fz, h.minz, h.inv_h, h.gz);
        const bool fin = fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY;
        const int c = (point_index(i) < n) ? (fin ? cx + h.gx * (cy + h.gy * cz) : -1) : -2;
        cell[i] = c;
        counts += (c >= 0 ? 1 : 0) + ((c >= 0 && c < c_lo) ? 0x10000 : 0);
        if (c >= c_lo && c < c_hi) atomicAdd(&s_cnt[c - c_lo], 1);
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) counts += __shfl_xor(counts, off, 64);
    if (lane == 0) s_counts[wave] = counts;
    __syncthreads();
    OGC_PROBE_BUILD(4);

    // 3. exclusive scan of my range's counts, offset by the points below the range
    const int nloc = c_hi - c_lo;
    const int chunk = (nloc + BUILD_THREADS - 1) / BUILD_THREADS;
    const int c0 = min(t * chunk, nloc), c1 = min(c0 + chunk, nloc);
    int sum = 0;
    for (int c = c0; c < c1; ++c) sum += s_cnt[c];
    int incl = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int up = __shfl_up(incl, off, 64);
        if (lane >= off) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    OGC_PROBE_BUILD(5);
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < BUILD_THREADS / 64; ++w) {
        before += w < wave ? s_wave[w] : 0;
        total += s_counts[w];
    }
    const int npts = total & 0xFFFF, below = total >> 16;
    int run = below + before + incl - sum;
    int *cs = cell_start + (size_t)b * stride_cells;
    for (int c = c0; c < c1; ++c) {
        const int cnt = s_cnt[c];
        s_cnt[c] = run; // becomes the scatter cursor
        cs[c_lo + c] = run;
        run += cnt;
    }
    if (t == 0 && part == 0) {
        cs[ncell] = npts;
        h.npts = npts;
        // (the flags of grid_build_kernel: see there)
        const float per_query = 27.0f * (float)npts / (float)ncell;
        h.dense = per_query > 0.25f * (float)n ? 1 : 0;
        h.heavy = per_query > 120.0f ? 1 : 0;
        if (!(1.0f * (1.0f / h.inv_h) * 0.999f >= radius) || per_query > 120.0f) h.knn_general = 1;
        hdrs[b] = h;
    }
    if (t == 0) s_tail = npts;
    __syncthreads();
    OGC_PROBE_BUILD(6);

    // 4. scatter the points of my range (part 0: also the points outside the grid, behind all cells)
    float4 *sp = sorted_pts + (size_t)b * n;
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
        const int k = point_index(i), c = cell[i];
        if (c >= c_lo && c < c_hi) sp[atomicAdd(&s_cnt[c - c_lo], 1)] = make_float4(px[i], py[i], pz[i], __int_as_float(k));
        else if (c == -1 && part == 0) sp[atomicAdd(&s_tail, 1)] = make_float4(NAN, NAN, NAN, __int_as_float(k));
    }
    OGC_PROBE_BUILD(7);
}

// parts per cloud of the split build (0: one workgroup per cloud).  OGC_GRID_SPLIT in the environment overrides (A/B runs).
static int grid_build_parts(int n) {
    static const int forced = [] { const char *e = getenv("OGC_GRID_SPLIT"); return e ? atoi(e) : -1; }();
    if (n > 16 * BUILD_THREADS) return 0;
    if (forced >= 0) return forced == 0 ? 0 : (forced < SPLIT_MIN ? SPLIT_MIN : (forced > 32 ? 32 : forced));
    return n <= 8 * BUILD_THREADS ? 8 : 16;
}

void launch_grid_build(int b, int n, float radius, int knn_k, int stride_cells, const float *xyz, GridHdr *hdrs, int *cell_start,
                       float4 *sorted_pts, hipStream_t s, int prefer_cells, float knn_div) {
    const int parts = grid_build_parts(n);
    if (parts > 0 && n <= 8 * BUILD_THREADS)
        hipLaunchKernelGGL(grid_build_split_kernel<8>, dim3(b * parts), dim3(BUILD_THREADS), 0, s, knn_div, b, parts, n, radius, knn_k,
                           prefer_cells, stride_cells, xyz, hdrs, cell_start, sorted_pts);
    else if (parts > 0)
        hipLaunchKernelGGL(grid_build_split_kernel<16>, dim3(b * parts), dim3(BUILD_THREADS), 0, s, knn_div, b, parts, n, radius, knn_k,
                           prefer_cells, stride_cells, xyz, hdrs, cell_start, sorted_pts);
    else if (n <= 8 * BUILD_THREADS)
        hipLaunchKernelGGL(grid_build_kernel<8>, dim3(b), dim3(BUILD_THREADS), 0, s, knn_div, n, radius, knn_k, prefer_cells, stride_cells, xyz,
                           hdrs, cell_start, sorted_pts);
    else if (n <= 16 * BUILD_THREADS)
        hipLaunchKernelGGL(grid_build_kernel<16>, dim3(b), dim3(BUILD_THREADS), 0, s, knn_div, n, radius, knn_k, prefer_cells, stride_cells,
                           xyz, hdrs, cell_start, sorted_pts);
    else
        hipLaunchKernelGGL(grid_build_kernel<0>, dim3(b), dim3(BUILD_THREADS), 0, s, knn_div, n, radius, knn_k, prefer_cells, stride_cells, xyz,
                           hdrs, cell_start, sorted_pts);
}

} // namespace ogc_grid

using namespace ogc_grid;

// ---- one grid for several radius searches of a batch of clouds in themselves (fused extension, include/ogc_ops.h) ------------
extern "C" long long ogc_cell_grid_bytes(int b, int n) {
    if (b < 0 || n < 0) return -1;
    return (long long)GridLayout(b, n).total();
}

extern "C" int ogc_cell_grid_build(int b, int n, float radius, const float *xyz, void *grid, ogc_stream_t stream) {
    OGC_REQUIRE(b >= 0 && n >= 0, "ogc_cell_grid_build: negative dimension");
    if (b == 0 || n == 0) return OGC_OK;
    OGC_REQUIRE(xyz && grid, "ogc_cell_grid_build: null pointer");
    if (!(radius > 0.0f) || !(radius < 3.0e38f) || n < 1024) {
        ogc_set_error("ogc_cell_grid_build: needs a finite positive radius and clouds of at least 1024 points (n=%d, r=%g)", n,
                      (double)radius);
        return OGC_ERR_UNSUPPORTED;
    }
    const GridLayout L(b, n);
    launch_grid_build(b, n, radius, 0, STRIDE_CELLS, xyz, L.hdrs(grid), L.cell_start(grid), L.sorted_pts(grid), (hipStream_t)stream, 2);
    OGC_CHECK_LAUNCH("ogc_cell_grid_build");
    return OGC_OK;
}

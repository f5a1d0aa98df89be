// surface_thin.hip — first-come greedy thinning of surface candidates, exact.  The rule is the sequential one:
// walking a mesh's candidates in index order, candidate i is kept iff no KEPT candidate j < i of the same mesh has
//     ((dx*dx) + (dy*dy)) + (dz*dz) <= r_m * r_m        (fp64, one rounding per operation, the bound inclusive).
// It stands for the rejection step of trimesh.sample.sample_surface_even (sample_pointcloud.py:57).
//
//   rounds     keep[i] is the state: -1 undecided, 1 kept, 0 removed.  In a round every undecided i looks at its neighbours j < i
//              within the radius: one of them kept -> removed; else none undecided -> kept; else it waits.  A state only ever moves
//              from undecided to its final value and every decision taken is the sequential one, so whatever a round sees of the
//              states written by its own launch — the L2s of the XCDs are not coherent inside a kernel — the result is the same;
//              a stale read only delays a decision by a round.  The lowest undecided index always decides, so the rounds end.
//              Rounds are launches; a round returns at once when status[1], the undecided left, is zero.
//   grid       private to this file: one uniform grid over the bounding box of all points of the call.  The cell edge is the
//              largest radius times (1 + 2^-20) — the margin covers the rounding of (x - lo) / edge, so that two points within a
//              radius always lie in adjacent cells — and grows by a quarter until the table has at most `cap` cells, cap =
//              min(2^22, max(4096, 8 C)).  Histogram, scan, scatter, all here.  The order of the entries of a cell is whatever the
//              atomics give; the rule goes by index, so it does not matter.  Meshes share the grid; a pair of different meshes
//              is skipped by index range.
//   refusals   status[0]: 1 a coordinate that is not finite, 2 a radius that is negative or not finite, 3 cand_offsets that do
//              not start at 0, descend or do not end at C.  With a status set keep is not written.
#include <math.h>

#include <algorithm>

#include "ogc_common.h"

namespace {

constexpr int ST_THREADS = 256;
constexpr int ST_BBOX_BLOCKS = 256;
constexpr int ST_SCAN_CHUNK = 8192;                // table entries per workgroup of the scan
constexpr int ST_SCAN_PER_THREAD = ST_SCAN_CHUNK / ST_THREADS;
constexpr int ST_MAX_CELLS = 1 << 22;
constexpr int ST_MAX_CHUNKS = ST_MAX_CELLS / ST_SCAN_CHUNK + 1;
constexpr int ST_MAX_POINTS = 1 << 26;
static_assert(ST_MAX_CHUNKS <= 1024 && ST_SCAN_PER_THREAD * ST_THREADS == ST_SCAN_CHUNK, "the chunk sums are scanned by one workgroup");

struct ThinHeader {
    double lo[3];
    double edge;
    int dim[3];
    int ncells;
};

struct ThinLayout { // byte offsets into the workspace
    size_t partial, sums, count, start, cell, sorted, total;
};

int thin_cap(int C) {
    long long cap = 8LL * C;
    if (cap < 4096) cap = 4096;
    if (cap > ST_MAX_CELLS) cap = ST_MAX_CELLS;
    return (int)cap;
}

ThinLayout thin_layout(int C) {
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t cap = (size_t)thin_cap(C);
    ThinLayout l;
    l.partial = up(sizeof(ThinHeader));
    l.sums = l.partial + up((size_t)ST_BBOX_BLOCKS * 8 * sizeof(double));
    l.count = l.sums + up((size_t)(ST_MAX_CHUNKS + 1) * sizeof(int));
    l.start = l.count + up((cap + 1) * sizeof(int));
    l.cell = l.start + up((cap + 1) * sizeof(int));
    l.sorted = l.cell + up((size_t)C * sizeof(int));
    l.total = l.sorted + up((size_t)C * sizeof(int));
    return l;
}

// per workgroup: the bounding box of its points and whether all of them are finite -> partial[block][0..6]
__global__ __launch_bounds__(ST_THREADS) void thin_bbox_kernel(int C, const double *__restrict__ points, double *__restrict__ partial) {
    __shared__ double red[ST_THREADS / OGC_WAVE][7];
    const int tid = threadIdx.x, lane = tid & (OGC_WAVE - 1), wave = tid / OGC_WAVE;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    double bad = 0.0;
    for (int i = blockIdx.x * ST_THREADS + tid; i < C; i += ST_BBOX_BLOCKS * ST_THREADS) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double v = points[(size_t)i * 3 + k];
            if (!isfinite(v)) bad = 1.0;
            lo[k] = fmin(lo[k], v);
            hi[k] = fmax(hi[k], v);
        }
    }
#pragma unroll
    for (int off = OGC_WAVE / 2; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            lo[k] = fmin(lo[k], __shfl_down(lo[k], off, OGC_WAVE));
            hi[k] = fmax(hi[k], __shfl_down(hi[k], off, OGC_WAVE));
        }
        bad = fmax(bad, __shfl_down(bad, off, OGC_WAVE));
    }
    if (lane == 0) {
        for (int k = 0; k < 3; ++k) {
            red[wave][k] = lo[k];
            red[wave][3 + k] = hi[k];
        }
        red[wave][6] = bad;
    }
    __syncthreads();
    if (tid < 7) {
        double v = red[0][tid];
        for (int w = 1; w < ST_THREADS / OGC_WAVE; ++w) v = tid < 3 ? fmin(v, red[w][tid]) : fmax(v, red[w][tid]);
        partial[blockIdx.x * 8 + tid] = v;
    }
}

// one workgroup: the box of the call, the checks of radius and offsets, the cell edge and the table's dimensions
__global__ __launch_bounds__(ST_THREADS) void thin_setup_kernel(int C, int M, int cap, const double *__restrict__ partial,
                                                                const int *__restrict__ cand_offsets, const double *__restrict__ radius,
                                                                ThinHeader *__restrict__ hdr, int *__restrict__ status) {
    __shared__ double red[7][ST_THREADS];
    __shared__ double rmax_s[ST_THREADS];
    __shared__ int bad_s[ST_THREADS];
    const int tid = threadIdx.x;
    static_assert(ST_BBOX_BLOCKS == ST_THREADS, "one partial box per thread");
    for (int k = 0; k < 7; ++k) red[k][tid] = partial[tid * 8 + k];
    double rmax = 0.0;
    int bad = 0; // bit 0: radius, bit 1: offsets
    for (int m = tid; m < M; m += ST_THREADS) {
        const double r = radius[m];
        if (!(r >= 0.0) || !isfinite(r)) bad |= 1;
        rmax = fmax(rmax, r);
        if (cand_offsets[m + 1] < cand_offsets[m]) bad |= 2;
    }
    if (tid == 0 && (cand_offsets[0] != 0 || cand_offsets[M] != C)) bad |= 2;
    rmax_s[tid] = rmax;
    bad_s[tid] = bad;
    __syncthreads();
    for (int s = ST_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
            for (int k = 0; k < 3; ++k) red[k][tid] = fmin(red[k][tid], red[k][tid + s]);
            for (int k = 3; k < 7; ++k) red[k][tid] = fmax(red[k][tid], red[k][tid + s]);
            rmax_s[tid] = fmax(rmax_s[tid], rmax_s[tid + s]);
            bad_s[tid] |= bad_s[tid + s];
        }
        __syncthreads();
    }
    if (tid != 0) return;
    const int code = red[6][0] != 0.0 ? 1 : (bad_s[0] & 1) ? 2 : (bad_s[0] & 2) ? 3 : 0;
    status[0] = code;
    status[1] = code ? 0 : C;
    status[2] = 0;
    if (code) {
        hdr->ncells = 0;
        return;
    }
    double half[3], widest = 0.0; // half extents: finite for any finite box
    for (int k = 0; k < 3; ++k) {
        half[k] = 0.5 * red[3 + k][0] - 0.5 * red[k][0];
        widest = fmax(widest, half[k]);
    }
    double edge = rmax_s[0] * (1.0 + 0x1.0p-20);
    edge = fmax(edge, widest * 0x1.0p-20); // at most 2^21 + 1 cells along an axis
    if (!(edge > 0.0)) edge = 1.0;         // every point the same and no radius: one cell
    int dim[3];
    for (int it = 0; it < 100000; ++it) {
        double cells = 1.0;
        for (int k = 0; k < 3; ++k) {
            const double n = fmin(floor(half[k] / edge * 2.0), 0x1.0p22);
            dim[k] = (int)n + 1;
            cells *= (double)dim[k];
        }
        if (cells <= (double)cap) break;
        edge *= 1.25;
    }
    if ((double)dim[0] * (double)dim[1] * (double)dim[2] > (double)cap) dim[0] = dim[1] = dim[2] = 1; // (an edge beyond the doubles)
    for (int k = 0; k < 3; ++k) {
        hdr->lo[k] = red[k][0];
        hdr->dim[k] = dim[k];
    }
    hdr->edge = edge;
    hdr->ncells = dim[0] * dim[1] * dim[2];
}

__device__ __forceinline__ int thin_axis_cell(double v, double lo, double edge, int dim) {
    const double q = floor((v - lo) / edge); // >= 0: lo is the smallest coordinate
    return q < (double)(dim - 1) ? (int)q : dim - 1; // (a NaN quotient, inf / inf on an absurd box, goes to the last cell)
}

__global__ __launch_bounds__(ST_THREADS) void thin_zero_kernel(const ThinHeader *__restrict__ hdr, const int *__restrict__ status,
                                                               int *__restrict__ count) {
    if (status[0] != 0) return;
    const int n = hdr->ncells + 1;
    for (int c = blockIdx.x * ST_THREADS + threadIdx.x; c < n; c += gridDim.x * ST_THREADS) count[c] = 0;
}

__global__ __launch_bounds__(ST_THREADS) void thin_hist_kernel(int C, const double *__restrict__ points, const ThinHeader *__restrict__ hdr,
                                                               const int *__restrict__ status, int *__restrict__ count,
                                                               int *__restrict__ cell, int *__restrict__ keep) {
    if (status[0] != 0) return;
    const int i = blockIdx.x * ST_THREADS + threadIdx.x;
    if (i >= C) return;
    const double edge = hdr->edge;
    const int cx = thin_axis_cell(points[(size_t)i * 3 + 0], hdr->lo[0], edge, hdr->dim[0]);
    const int cy = thin_axis_cell(points[(size_t)i * 3 + 1], hdr->lo[1], edge, hdr->dim[1]);
    const int cz = thin_axis_cell(points[(size_t)i * 3 + 2], hdr->lo[2], edge, hdr->dim[2]);
    const int c = (cz * hdr->dim[1] + cy) * hdr->dim[0] + cx;
    cell[i] = c;
    keep[i] = -1;
    atomicAdd(&count[c], 1);
}

// exclusive scan of count[0 .. ncells] into start[], three launches: chunk sums, their scan by one workgroup, the chunks
__global__ __launch_bounds__(ST_THREADS) void thin_scan_sums_kernel(const ThinHeader *__restrict__ hdr, const int *__restrict__ status,
                                                                    const int *__restrict__ count, int *__restrict__ sums) {
    __shared__ int part[ST_THREADS / OGC_WAVE];
    if (status[0] != 0) return;
    const int n = hdr->ncells + 1, base = blockIdx.x * ST_SCAN_CHUNK, tid = threadIdx.x;
    int s = 0;
    for (int k = 0; k < ST_SCAN_PER_THREAD; ++k) {
        const int c = base + k * ST_THREADS + tid;
        if (c < n) s += count[c];
    }
#pragma unroll
    for (int off = OGC_WAVE / 2; off > 0; off >>= 1) s += __shfl_down(s, off, OGC_WAVE);
    if ((tid & (OGC_WAVE - 1)) == 0) part[tid / OGC_WAVE] = s;
    __syncthreads();
    if (tid == 0) {
        int t = 0;
        for (int w = 0; w < ST_THREADS / OGC_WAVE; ++w) t += part[w];
        sums[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(1024) void thin_scan_top_kernel(int nchunks, const int *__restrict__ status, int *__restrict__ sums) {
    __shared__ int buf[2][1024];
    if (status[0] != 0) return;
    const int tid = threadIdx.x;
    const int own = tid < nchunks ? sums[tid] : 0;
    int cur = 0;
    buf[0][tid] = own;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) { // inclusive scan, ping-pong
        buf[cur ^ 1][tid] = buf[cur][tid] + (tid >= off ? buf[cur][tid - off] : 0);
        cur ^= 1;
        __syncthreads();
    }
    if (tid < nchunks) sums[tid] = buf[cur][tid] - own; // exclusive
}

__global__ __launch_bounds__(ST_THREADS) void thin_scan_chunks_kernel(const ThinHeader *__restrict__ hdr, const int *__restrict__ status,
                                                                      const int *__restrict__ count, const int *__restrict__ sums,
                                                                      int *__restrict__ start) {
    __shared__ int tot[ST_THREADS];
    if (status[0] != 0) return;
    const int n = hdr->ncells + 1, tid = threadIdx.x;
    const int base = blockIdx.x * ST_SCAN_CHUNK + tid * ST_SCAN_PER_THREAD; // a thread owns consecutive entries
    int v[ST_SCAN_PER_THREAD], s = 0;
#pragma unroll
    for (int k = 0; k < ST_SCAN_PER_THREAD; ++k) {
        v[k] = base + k < n ? count[base + k] : 0;
        s += v[k];
    }
    tot[tid] = s;
    __syncthreads();
    if (tid == 0) { // 256 additions by one thread: this table is scanned once per call
        int run = sums[blockIdx.x];
        for (int t = 0; t < ST_THREADS; ++t) {
            const int x = tot[t];
            tot[t] = run;
            run += x;
        }
    }
    __syncthreads();
    int run = tot[tid];
#pragma unroll
    for (int k = 0; k < ST_SCAN_PER_THREAD; ++k) {
        if (base + k < n) start[base + k] = run;
        run += v[k];
    }
}

__global__ __launch_bounds__(ST_THREADS) void thin_scatter_kernel(int C, const int *__restrict__ status, const int *__restrict__ cell,
                                                                  const int *__restrict__ start, int *__restrict__ count,
                                                                  int *__restrict__ sorted) {
    if (status[0] != 0) return;
    const int i = blockIdx.x * ST_THREADS + threadIdx.x;
    if (i >= C) return;
    const int c = cell[i];
    const int slot = atomicSub(&count[c], 1) - 1; // count[c] .. 1 -> the cell's slots, in no particular order
    sorted[start[c] + slot] = i;
}

__global__ __launch_bounds__(ST_THREADS) void thin_round_kernel(int C, int M, int round, const double *__restrict__ points,
                                                                const int *__restrict__ cand_offsets, const double *__restrict__ radius,
                                                                const ThinHeader *__restrict__ hdr, const int *__restrict__ cell,
                                                                const int *__restrict__ start, const int *__restrict__ sorted, int *keep,
                                                                int *status) {
#pragma clang fp contract(off)
    if (status[0] != 0 || __hip_atomic_load(&status[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) return;
    const int i = blockIdx.x * ST_THREADS + threadIdx.x;
    bool decided = false;
    if (i < C && keep[i] == -1) { // its own state is written by this thread alone
        int mlo = 0, mhi = M;     // the mesh of i: cand_offsets[mlo] <= i < cand_offsets[mhi]
        while (mhi - mlo > 1) {
            const int mid = (mlo + mhi) >> 1;
            if (cand_offsets[mid] <= i) mlo = mid; else mhi = mid;
        }
        const int first = cand_offsets[mlo];
        const double r = radius[mlo], r2 = r * r;
        const double x = points[(size_t)i * 3 + 0], y = points[(size_t)i * 3 + 1], z = points[(size_t)i * 3 + 2];
        const int nx = hdr->dim[0], ny = hdr->dim[1], nz = hdr->dim[2];
        const int c = cell[i], cx = c % nx, cy = (c / nx) % ny, cz = c / (nx * ny);
        bool removed = false, waiting = false;
        for (int dz = max(cz - 1, 0); dz <= min(cz + 1, nz - 1) && !removed; ++dz)
            for (int dy = max(cy - 1, 0); dy <= min(cy + 1, ny - 1) && !removed; ++dy) {
                // the up to three cells along x are neighbours in the table: one range of entries
                const int row = (dz * ny + dy) * nx;
                const int k0 = start[row + max(cx - 1, 0)], k1 = start[row + min(cx + 1, nx - 1) + 1];
                for (int k = k0; k < k1; ++k) {
                    const int j = sorted[k];
                    if (j >= i || j < first) continue; // later candidates and other meshes have no say
                    const int sj = __hip_atomic_load(&keep[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (sj == 0) continue;             // a removed candidate removes nobody
                    const double ddx = x - points[(size_t)j * 3 + 0], ddy = y - points[(size_t)j * 3 + 1],
                                 ddz = z - points[(size_t)j * 3 + 2];
                    if (((ddx * ddx) + (ddy * ddy)) + (ddz * ddz) <= r2) {
                        if (sj == 1) {
                            removed = true;
                            break;
                        }
                        waiting = true;
                    }
                }
            }
        if (removed || !waiting) {
            __hip_atomic_store(&keep[i], removed ? 0 : 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            decided = true;
        }
    }
    const unsigned long long mask = __builtin_amdgcn_ballot_w64(decided);
    if (mask != 0 && (int)(threadIdx.x & (OGC_WAVE - 1)) == __ffsll((long long)mask) - 1) { // the first lane that decided
        atomicSub(&status[1], __popcll(mask));
        atomicMax(&status[2], round + 1);
    }
}

} // namespace

extern "C" long long ogc_surface_thin_ws_bytes(int C, int M) {
    (void)M;
    if (C < 0 || C > ST_MAX_POINTS) return -1;
    return (long long)thin_layout(C).total;
}

extern "C" int ogc_surface_thin(int C, int M, const double *points, const int *cand_offsets, const double *radius, int rounds,
                                int rounds_done, int *keep, int *status, void *ws, long long ws_bytes, ogc_stream_t stream) {
    const char *name = "ogc_surface_thin";
    OGC_REQUIRE(C >= 0 && M >= 0, "%s: negative size (C = %d, M = %d)", name, C, M);
    OGC_REQUIRE(rounds >= 0 && rounds <= 65536 && rounds_done >= 0 && rounds_done <= 0x7fffffff - 65536,
                "%s: rounds = %d, rounds_done = %d, need 0 <= rounds <= 65536 and rounds_done >= 0", name, rounds, rounds_done);
    if (C > ST_MAX_POINTS) {
        ogc_set_error("%s: C = %d, at most %d candidates per call", name, C, ST_MAX_POINTS);
        return OGC_ERR_UNSUPPORTED;
    }
    if (C == 0) return OGC_OK;
    OGC_REQUIRE(M >= 1, "%s: %d candidates need a mesh (M = %d)", name, C, M);
    OGC_REQUIRE(points && cand_offsets && radius && keep && status && ws, "%s: null pointer (points, cand_offsets, radius, keep, status or ws)", name);
    const ThinLayout l = thin_layout(C);
    OGC_REQUIRE(ws_bytes >= (long long)l.total, "%s: workspace of %lld bytes, ogc_surface_thin_ws_bytes(%d, %d) = %lld", name, ws_bytes, C, M,
                (long long)l.total);
    OGC_REQUIRE(((uintptr_t)ws & 255) == 0, "%s: the workspace must be 256-byte aligned", name);
    hipStream_t s = (hipStream_t)stream;
    char *base = static_cast<char *>(ws);
    ThinHeader *hdr = reinterpret_cast<ThinHeader *>(base);
    double *partial = reinterpret_cast<double *>(base + l.partial);
    int *sums = reinterpret_cast<int *>(base + l.sums), *count = reinterpret_cast<int *>(base + l.count);
    int *start = reinterpret_cast<int *>(base + l.start), *cell = reinterpret_cast<int *>(base + l.cell);
    int *sorted = reinterpret_cast<int *>(base + l.sorted);
    const unsigned blocks = (unsigned)ogc_divup(C, ST_THREADS);
    if (rounds_done == 0) { // a fresh call: the grid; a continuation finds it in the workspace
        const int cap = thin_cap(C), nchunks = ogc_divup((long long)cap + 1, ST_SCAN_CHUNK);
        hipLaunchKernelGGL(thin_bbox_kernel, dim3(ST_BBOX_BLOCKS), dim3(ST_THREADS), 0, s, C, points, partial);
        hipLaunchKernelGGL(thin_setup_kernel, dim3(1), dim3(ST_THREADS), 0, s, C, M, cap, partial, cand_offsets, radius, hdr, status);
        hipLaunchKernelGGL(thin_zero_kernel, dim3((unsigned)std::min(ogc_divup((long long)cap + 1, ST_THREADS), 1024)), dim3(ST_THREADS), 0, s, hdr,
                           status, count);
        hipLaunchKernelGGL(thin_hist_kernel, dim3(blocks), dim3(ST_THREADS), 0, s, C, points, hdr, status, count, cell, keep);
        hipLaunchKernelGGL(thin_scan_sums_kernel, dim3((unsigned)nchunks), dim3(ST_THREADS), 0, s, hdr, status, count, sums);
        hipLaunchKernelGGL(thin_scan_top_kernel, dim3(1), dim3(1024), 0, s, nchunks, status, sums);
        hipLaunchKernelGGL(thin_scan_chunks_kernel, dim3((unsigned)nchunks), dim3(ST_THREADS), 0, s, hdr, status, count, sums, start);
        hipLaunchKernelGGL(thin_scatter_kernel, dim3(blocks), dim3(ST_THREADS), 0, s, C, status, cell, start, count, sorted);
        OGC_CHECK_LAUNCH(name);
    }
    for (int r = 0; r < rounds; ++r)
        hipLaunchKernelGGL(thin_round_kernel, dim3(blocks), dim3(ST_THREADS), 0, s, C, M, rounds_done + r, points, cand_offsets, radius, hdr,
                           cell, start, sorted, keep, status);
    OGC_CHECK_LAUNCH(name);
    return OGC_OK;
}

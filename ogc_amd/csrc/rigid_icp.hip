// rigid_icp.hip — batched classical point-to-point ICP (the reference's utils/icp_util.py:73-124, which runs sklearn's
// nearest-neighbour search and numpy's SVD on the CPU once per iteration), all iterations of a pair inside ONE launch.
//
// One workgroup per pair.  The destination cloud never changes: it sits in LDS as fp32, structure-of-arrays, padded with +inf
// to a multiple of four, and every lane walks it in step, so each ds_read_b128 is a broadcast of four candidates (no bank
// conflicts).  A thread owns the source points tid, tid + blockDim, ... (at most PTS of them) and keeps their running
// homogeneous coordinates in registers as double.  Everything the reference does in float64 is double here — coordinates are
// widened on load; differences, squared distances, sums, the SVD (svd3.h) and the running source — which is what makes the
// discrete results (correspondences, iteration count) reproducible against it.  On exact distance ties the lower index wins.
//
// An iteration: search; block sums of the source, the matched destination points and the distances; block sums of the nine
// centred products; thread 0 sums the wave partials, fits R, t (with the reflection fix) and decides whether the loop ends;
// everybody applies the step to its points.  The sums are taken in a fixed order — a thread's points ascending, a shuffle tree
// inside the wave, the waves ascending through LDS — without atomics, so two runs give the same bits.  The decision to leave
// the loop is one LDS word written by thread 0 and read by every thread after a barrier: all waves leave in the same
// iteration, none can wait at a barrier the others never reach.  After the loop the same fit runs once more, from the ORIGINAL
// source to the moved one: that, not the product of the steps, is the transform the reference returns.
#include "ogc_common.h"
#include "svd3.h"

namespace {

constexpr int ICP_THREADS = 1024;                         // the largest workgroup; smaller clouds get fewer waves
constexpr int PTS = OGC_ICP_MAX_POINTS / ICP_THREADS;     // source points per thread
constexpr int ICP_WAVES = ICP_THREADS / OGC_WAVE;
static_assert(OGC_ICP_MAX_POINTS % ICP_THREADS == 0, "points per thread");

struct IcpShared {                 // behind the destination cloud in the dynamic LDS region, 16-byte aligned
    double part[ICP_WAVES][9];     // wave partials of the current block sum
    double step[12];               // R (row-major) and t of the fit thread 0 made last
    int done;                      // the loop-exit word
    int iters;
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = OGC_WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, OGC_WAVE);
    return v; // lane 0 holds the sum
}

// Sums of NV values per thread over the workgroup, in the fixed order described above.  Every thread receives the totals.
// Two barriers: the partials are complete before anyone reads them, and read by all before the next call overwrites them.
template <int NV>
__device__ __forceinline__ void block_sums(double (&v)[NV], IcpShared *sh) {
    const int lane = threadIdx.x & (OGC_WAVE - 1), wave = threadIdx.x / OGC_WAVE, nwaves = blockDim.x / OGC_WAVE;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const double s = wave_sum(v[k]);
        if (lane == 0) sh->part[wave][k] = s;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        double s = sh->part[0][k];
        for (int w = 1; w < nwaves; ++w) s += sh->part[w][k];
        v[k] = s;
    }
    __syncthreads();
}

// Least-squares rigid transform from the points a to the corresponding points b (count[k] tells which of a thread's slots
// hold a point): centroids, cross-covariance H = sum (a - ca)(b - cb)^T, R = V diag(1, 1, det) U^T, t = cb - R ca.  Thread 0
// leaves R | t in sh->step; the caller's barrier publishes it.  `dist_sum` (in: this thread's share, out on every thread: the
// block total) rides along with the centroid sums.
__device__ __forceinline__ void fit(const double (&a)[PTS][3], const double (&b)[PTS][3], const bool (&has)[PTS], int n,
                                    double &dist_sum, IcpShared *sh) {
    double s[7] = {0, 0, 0, 0, 0, 0, dist_sum};
#pragma unroll
    for (int k = 0; k < PTS; ++k)
        if (has[k])
            for (int c = 0; c < 3; ++c) {
                s[c] += a[k][c];
                s[3 + c] += b[k][c];
            }
    block_sums(s, sh);
    double ca[3], cb[3];
    for (int c = 0; c < 3; ++c) {
        ca[c] = s[c] / n;
        cb[c] = s[3 + c] / n;
    }
    dist_sum = s[6];
    double h[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < PTS; ++k)
        if (has[k])
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) h[r * 3 + c] += (a[k][r] - ca[r]) * (b[k][c] - cb[c]);
    block_sums(h, sh);
    if (threadIdx.x == 0) {
        double H[3][3], R[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
        double scale = 0.0;
        bool finite = true;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) {
                H[r][c] = h[r * 3 + c];
                finite = finite && isfinite(H[r][c]);
                scale = fmax(scale, fabs(H[r][c]));
            }
        if (finite && scale > 0.0) { // otherwise (NaN input, or all points coincide) no rotation is preferred: identity
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) H[r][c] /= scale;
            ogc_kabsch3(H, R);
        }
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) sh->step[r * 3 + c] = R[r][c];
            sh->step[9 + r] = cb[r] - (R[r][0] * ca[0] + R[r][1] * ca[1] + R[r][2] * ca[2]);
        }
    }
}

__global__ __launch_bounds__(ICP_THREADS) void rigid_icp_kernel(int n, const float *__restrict__ src_all,
                                                                const float *__restrict__ dst_all,
                                                                const double *__restrict__ init_all, int max_iterations,
                                                                double tolerance, double *__restrict__ T_all,
                                                                double *__restrict__ dist_all, int *__restrict__ iters_all) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int np = (n + 3) & ~3; // the cloud padded to whole float4 groups
    float *dx = reinterpret_cast<float *>(smem), *dy = dx + np, *dz = dy + np;
    IcpShared *sh = reinterpret_cast<IcpShared *>(dz + np);
    const int tid = threadIdx.x, nt = blockDim.x;
    const size_t pair = blockIdx.x;
    const float *src = src_all + pair * n * 3, *dst = dst_all + pair * n * 3;

    for (int j = tid; j < np; j += nt) {
        const bool in = j < n;
        dx[j] = in ? dst[(size_t)j * 3 + 0] : INFINITY;
        dy[j] = in ? dst[(size_t)j * 3 + 1] : INFINITY;
        dz[j] = in ? dst[(size_t)j * 3 + 2] : INFINITY;
    }

    // the running source, homogeneous: w stays 1 unless the initial pose has another last row (the reference multiplies 4x4)
    double p[PTS][3], w[PTS], q[PTS][3], d2[PTS];
    bool has[PTS];
#pragma unroll
    for (int k = 0; k < PTS; ++k) {
        const int i = tid + k * nt;
        has[k] = i < n;
        d2[k] = 0.0;
        w[k] = 1.0;
        for (int c = 0; c < 3; ++c) p[k][c] = has[k] ? (double)src[(size_t)i * 3 + c] : 0.0;
        if (has[k] && init_all) {
            const double *M = init_all + pair * 16;
            const double x = p[k][0], y = p[k][1], z = p[k][2];
            for (int c = 0; c < 3; ++c) p[k][c] = M[c * 4 + 0] * x + M[c * 4 + 1] * y + M[c * 4 + 2] * z + M[c * 4 + 3];
            w[k] = M[12] * x + M[13] * y + M[14] * z + M[15];
        }
    }
    __syncthreads();

    double prev_error = 0.0; // thread 0's
    for (int it = 0;; ++it) {
        // nearest destination point of every own source point; strict '<' over ascending j keeps the lower index on ties,
        // and the +inf padding never wins
        double dist_sum = 0.0;
#pragma unroll
        for (int k = 0; k < PTS; ++k) {
            if (!has[k]) continue;
            const double x = p[k][0], y = p[k][1], z = p[k][2];
            double best = INFINITY;
            int bi = 0;
            for (int j = 0; j < np; j += 4) {
                const float4 cx = *reinterpret_cast<const float4 *>(dx + j);
                const float4 cy = *reinterpret_cast<const float4 *>(dy + j);
                const float4 cz = *reinterpret_cast<const float4 *>(dz + j);
                const float gx[4] = {cx.x, cx.y, cx.z, cx.w}, gy[4] = {cy.x, cy.y, cy.z, cy.w},
                            gz[4] = {cz.x, cz.y, cz.z, cz.w};
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const double ex = x - (double)gx[u], ey = y - (double)gy[u], ez = z - (double)gz[u];
                    const double d = ex * ex + ey * ey + ez * ez;
                    if (d < best) {
                        best = d;
                        bi = j + u;
                    }
                }
            }
            d2[k] = sqrt(best);
            dist_sum += d2[k];
            q[k][0] = dx[bi];
            q[k][1] = dy[bi];
            q[k][2] = dz[bi];
        }
        fit(p, q, has, n, dist_sum, sh);
        if (tid == 0) {
            // the reference's order: the step is applied first, then the error of the search above is compared
            const double mean_error = dist_sum / n;
            const bool stop = fabs(prev_error - mean_error) < tolerance || it == max_iterations - 1;
            prev_error = mean_error;
            sh->done = stop ? 1 : 0;
            sh->iters = it;
        }
        __syncthreads(); // step and exit word are published; the next writer of either sits behind block_sums' barriers
        double R[9], t[3];
        for (int c = 0; c < 9; ++c) R[c] = sh->step[c];
        for (int c = 0; c < 3; ++c) t[c] = sh->step[9 + c];
#pragma unroll
        for (int k = 0; k < PTS; ++k) {
            const double x = p[k][0], y = p[k][1], z = p[k][2];
            for (int c = 0; c < 3; ++c) p[k][c] = R[c * 3 + 0] * x + R[c * 3 + 1] * y + R[c * 3 + 2] * z + t[c] * w[k];
        }
        if (sh->done) break; // uniform over the workgroup
    }

    // distances of the last search, then the transform from the original source to where the loop left it
    double *dist = dist_all + pair * n;
#pragma unroll
    for (int k = 0; k < PTS; ++k) {
        const int i = tid + k * nt;
        if (has[k]) {
            dist[i] = d2[k];
            for (int c = 0; c < 3; ++c) q[k][c] = (double)src[(size_t)i * 3 + c];
        }
    }
    double unused = 0.0;
    fit(q, p, has, n, unused, sh);
    __syncthreads();
    if (tid < 16) {
        const int r = tid >> 2, c = tid & 3;
        T_all[pair * 16 + tid] = r == 3 ? (c == 3 ? 1.0 : 0.0) : (c == 3 ? sh->step[9 + r] : sh->step[r * 3 + c]);
    }
    if (tid == 0) iters_all[pair] = sh->iters;
}

} // namespace

extern "C" int ogc_rigid_icp(int B, int n, const float *src, const float *dst, const double *init_pose, int max_iterations,
                             double tolerance, double *T, double *distances, int *iters, ogc_stream_t stream) {
    OGC_REQUIRE(B >= 0, "ogc_rigid_icp: negative batch");
    if (B == 0) return OGC_OK;
    OGC_REQUIRE(n >= 3, "ogc_rigid_icp: a rigid fit needs at least 3 points per cloud, got n = %d", n);
    OGC_REQUIRE(n <= OGC_ICP_MAX_POINTS, "ogc_rigid_icp: n = %d exceeds OGC_ICP_MAX_POINTS = %d (the destination cloud stays in LDS)",
                n, OGC_ICP_MAX_POINTS);
    OGC_REQUIRE(max_iterations >= 1, "ogc_rigid_icp: max_iterations = %d, need at least 1", max_iterations);
    OGC_REQUIRE(src && dst && T && distances && iters, "ogc_rigid_icp: null pointer");
    const int threads = min(ICP_THREADS, ogc_divup(n, OGC_WAVE) * OGC_WAVE);
    const size_t lds = (size_t)((n + 3) & ~3) * 3 * sizeof(float) + sizeof(IcpShared);
    hipLaunchKernelGGL(rigid_icp_kernel, dim3(B), dim3(threads), lds, (hipStream_t)stream, n, src, dst, init_pose,
                       max_iterations, tolerance, T, distances, iters);
    OGC_CHECK_LAUNCH("ogc_rigid_icp");
    return OGC_OK;
}

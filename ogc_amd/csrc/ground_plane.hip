// ground_plane.hip — batched ground-plane fitting (the reference's utils/gpf_util.py:45-66, numpy + scikit-spatial on the CPU,
// twice per scene pair of the Waymo flow-prediction stage), seed, every fit, every retry of a cloud inside ONE launch.
//
// One workgroup per cloud.  A thread owns the points tid, tid + blockDim, ... (at most PTS of them) and keeps their coordinates
// in registers as double, widened on load, next to the order-preserving 32-bit key of their fp32 height; everything the
// float64 statement of the algorithm does in double is double here.  LDS holds no point data at all: a histogram of 256
// counters, the wave partials of the block sums and what thread 0 publishes.
//
//   seed height   lpr = mean of the n_lpr smallest heights.  A 4 x 8-bit radix select finds the n_lpr-th smallest KEY (integer
//                 histogram atomics in LDS, wave 0 scans the 256 counters with shuffles); the mean is the fp64 block sum of the
//                 heights whose key lies below it plus (n_lpr - their number) x that height — the same value whichever of
//                 several tied heights a partition would have taken.  -0 is folded into +0 before the key is made.
//   fit           count and coordinate sums, then the six centred products of the selected points, as block sums in a fixed
//                 order — a thread's points ascending, a shuffle tree inside the wave, the waves ascending through LDS — without
//                 floating-point atomics, so two runs give the same bits.  Thread 0 solves the symmetric 3x3 eigen-problem
//                 (svd3.h, ogc_sym_eig3); the normal is the eigenvector of the smallest eigenvalue, unit length, signed so that
//                 its vertical component is >= 0.
//   failure       fewer than 3 points selected; a count, centre or scatter that is not finite; or a selection of rank below 2.
//                 COLLINEARITY RULE: with l1 >= l2 >= l3 the eigenvalues of the scatter (the squared singular values of the
//                 centred selection) the fit is refused unless  l2 > l1 * count * DBL_EPSILON.  numpy.linalg.matrix_rank of the
//                 centred points refuses sigma2 <= sigma1 * count * eps; a scatter matrix carries its small eigenvalues only to
//                 about count * eps * l1, so sigma2 / sigma1 = sqrt(count * eps) (1.3e-6 at 8192 points) is the finest line
//                 that can be drawn from it: an exactly collinear selection (l2 == 0) and every selection the float64 SVD
//                 would also call a plane down to that ratio are decided as numpy decides them.
//   retry         thread 0 adds 0.05 to the seed threshold — repeated addition in double, as the reference's `thresh_seed +=
//                 0.05` — and gives up when the sum exceeds 0.8.
//
// Every decision that ends a loop (fit failed, give up) is ONE LDS word written by thread 0 and read by every thread after a
// barrier: all waves leave in the same iteration, none can wait at a barrier the others never reach.  Every loop is bounded:
// four select passes, n_iter fits, and an attempt cap the host computes from thresh_seed with the same additions.
#include <float.h>

#include "ogc_common.h"
#include "svd3.h"

namespace {

constexpr int GPF_THREADS = 1024;                            // the largest workgroup; smaller clouds get fewer waves
constexpr int GPF_MAX_PTS = OGC_GPF_MAX_POINTS / GPF_THREADS; // points per thread at the size limit
constexpr int GPF_WAVES = GPF_THREADS / OGC_WAVE;
constexpr int GPF_ATTEMPT_LIMIT = 4096;                      // thresh_seed so far below 0.8 that more fits were needed is refused
constexpr double GPF_SEED_STEP = 0.05, GPF_SEED_GIVE_UP = 0.8;
static_assert(OGC_GPF_MAX_POINTS % GPF_THREADS == 0 && GPF_MAX_PTS == 8, "points per thread");

enum { GPF_FIT_OK = 0, GPF_RETRY = 1, GPF_GIVE_UP = 2 };

struct GpfShared {
    alignas(16) int hist[256];     // digit counts of the current select pass
    double part[GPF_WAVES][6];     // wave partials of the current block sum
    double plane[6];               // centre and unit normal of the fit thread 0 made last
    double thresh_seed;            // the raised seed threshold after a failed fit
    unsigned prefix;               // select: the leading bits found so far
    int rank;                      // select: 1-based rank still to find among the keys that share `prefix`
    int state;                     // GPF_FIT_OK / GPF_RETRY / GPF_GIVE_UP of the last fit: the loop-exit word
};

__device__ __forceinline__ double gpf_wave_sum(double v) {
#pragma unroll
    for (int off = OGC_WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, OGC_WAVE);
    return v; // lane 0 holds the sum
}

// Sums of NV values per thread over the workgroup in the fixed order described above; every thread receives the totals.
// Two barriers: the partials are complete before anyone reads them, and read by all before the next call overwrites them.
template <int NV>
__device__ __forceinline__ void gpf_block_sums(double (&v)[NV], GpfShared *sh) {
    const int lane = threadIdx.x & (OGC_WAVE - 1), wave = threadIdx.x / OGC_WAVE, nwaves = blockDim.x / OGC_WAVE;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const double s = gpf_wave_sum(v[k]);
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

// fp32 -> a 32-bit key that orders as the floats do (negative floats reversed below the positive ones), and back
__device__ __forceinline__ unsigned gpf_height_key(float h) {
    const unsigned u = __float_as_uint(h + 0.0f); // -0 -> +0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float gpf_key_height(unsigned key) {
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

// a point's height by selects: indexing registers with a run-time axis would move the points out of them
__device__ __forceinline__ double gpf_height(const double (&p)[3], int vertical_axis) {
    return vertical_axis == 0 ? p[0] : vertical_axis == 1 ? p[1] : p[2];
}

// The key of 1-based rank `rank` among the workgroup's keys (1 <= rank <= number of keys), most significant byte first.
// Returns it on every thread, with `rank_in_ties` its rank among the keys equal to it (>= 1): rank - rank_in_ties keys are
// smaller.  Three barriers per pass: counters zeroed | counted | the chosen digit published.
template <int PTS>
__device__ __forceinline__ unsigned gpf_select(const unsigned (&key)[PTS], const bool (&has)[PTS], int rank, GpfShared *sh,
                                               int &rank_in_ties) {
    const int tid = threadIdx.x, nt = blockDim.x;
    unsigned prefix = 0u;
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        const unsigned known = pass == 0 ? 0u : 0xffffffffu << (shift + 8); // the bits `prefix` already fixes
        for (int i = tid; i < 256; i += nt) sh->hist[i] = 0;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PTS; ++k)
            if (has[k] && (key[k] & known) == prefix) atomicAdd(&sh->hist[(key[k] >> shift) & 255u], 1);
        __syncthreads();
        if (tid < OGC_WAVE) { // wave 0 exists in every launch: lane l takes the digits 4l .. 4l + 3
            const int4 c4 = reinterpret_cast<const int4 *>(sh->hist)[tid];
            const int c[4] = {c4.x, c4.y, c4.z, c4.w};
            const int own = c[0] + c[1] + c[2] + c[3];
            int incl = own;
#pragma unroll
            for (int off = 1; off < OGC_WAVE; off <<= 1) {
                const int below = __shfl_up(incl, off, OGC_WAVE);
                if (tid >= off) incl += below;
            }
            const int excl = incl - own;
            if (excl < rank && rank <= incl) { // exactly one lane: the counters add up to the keys in play, at least `rank`
                int r = rank - excl, d = 0;
                for (; d < 3; ++d) {
                    if (r <= c[d]) break;
                    r -= c[d];
                }
                sh->prefix = prefix | ((unsigned)(4 * tid + d) << shift);
                sh->rank = r;
            }
        }
        __syncthreads();
        prefix = sh->prefix; // the next writers sit behind the next pass's two barriers (or gpf_block_sums')
        rank = sh->rank;
    }
    rank_in_ties = rank;
    return prefix;
}

// Plane through the selected points: thread 0 leaves centre | normal and GPF_FIT_OK in `sh`, or GPF_RETRY / GPF_GIVE_UP and
// the raised seed threshold.  The caller's barrier publishes it.
template <int PTS>
__device__ __forceinline__ void gpf_fit(const double (&p)[PTS][3], const bool (&sel)[PTS], int vertical_axis, double thresh_seed,
                                        GpfShared *sh) {
    double s[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < PTS; ++k)
        if (sel[k]) {
            s[0] += 1.0;
            for (int c = 0; c < 3; ++c) s[1 + c] += p[k][c];
        }
    gpf_block_sums(s, sh);
    const double count = s[0]; // a sum of ones below 2^53: exact
    const double c[3] = {s[1] / count, s[2] / count, s[3] / count};
    double m[6] = {0, 0, 0, 0, 0, 0}; // xx xy xz yy yz zz of the centred selection
#pragma unroll
    for (int k = 0; k < PTS; ++k)
        if (sel[k]) {
            const double x = p[k][0] - c[0], y = p[k][1] - c[1], z = p[k][2] - c[2];
            m[0] += x * x;
            m[1] += x * y;
            m[2] += x * z;
            m[3] += y * y;
            m[4] += y * z;
            m[5] += z * z;
        }
    gpf_block_sums(m, sh);
    if (threadIdx.x == 0) {
        double scale = 0.0, normal[3] = {0, 0, 0};
        bool ok = count >= 3.0;
        for (int k = 0; k < 6; ++k) {
            ok = ok && isfinite(m[k]);
            scale = fmax(scale, fabs(m[k]));
        }
        ok = ok && isfinite(c[0]) && isfinite(c[1]) && isfinite(c[2]) && scale > 0.0; // scale == 0: all points coincide
        if (ok) {
            const double S[3][3] = {{m[0] / scale, m[1] / scale, m[2] / scale},
                                    {m[1] / scale, m[3] / scale, m[4] / scale},
                                    {m[2] / scale, m[4] / scale, m[5] / scale}};
            double lam[3], V[3][3];
            ogc_sym_eig3(S, lam, V);
            ok = lam[1] > lam[0] * count * DBL_EPSILON; // the collinearity rule (head of this file)
            const double nrm = sqrt(V[0][2] * V[0][2] + V[1][2] * V[1][2] + V[2][2] * V[2][2]);
            ok = ok && nrm > 0.0;
            if (ok) {
                // (selects, not V[vertical_axis]: a dynamically indexed private array would be placed in LDS, 72 bytes per thread)
                const double vertical = vertical_axis == 0 ? V[0][2] : vertical_axis == 1 ? V[1][2] : V[2][2];
                const double sign = vertical < 0.0 ? -1.0 : 1.0;
                for (int r = 0; r < 3; ++r) normal[r] = sign * V[r][2] / nrm;
            }
        }
        int state = GPF_FIT_OK;
        if (!ok) { // the reference: `thresh_seed += 0.05`, give up `if thresh_seed > 0.8`
            const double raised = thresh_seed + GPF_SEED_STEP;
            state = raised > GPF_SEED_GIVE_UP ? GPF_GIVE_UP : GPF_RETRY;
            sh->thresh_seed = raised;
        }
        for (int r = 0; r < 3; ++r) {
            sh->plane[r] = c[r];
            sh->plane[3 + r] = normal[r];
        }
        sh->state = state;
    }
}

template <int PTS>
__global__ __launch_bounds__(GPF_THREADS) void ground_plane_fit_kernel(int n, const float *__restrict__ pc_all, int n_iter,
                                                                       int n_lpr, double thresh_seed, double thresh_dist,
                                                                       int vertical_axis, int max_attempts,
                                                                       double *__restrict__ plane_all,
                                                                       int *__restrict__ ground_all,
                                                                       int *__restrict__ attempts_all) {
    __shared__ GpfShared shared;
    GpfShared *sh = &shared;
    const int tid = threadIdx.x, nt = blockDim.x;
    const size_t cloud = blockIdx.x;
    const float *pc = pc_all + cloud * n * 3;

    double p[PTS][3];
    unsigned key[PTS];
    bool has[PTS], sel[PTS];
#pragma unroll
    for (int k = 0; k < PTS; ++k) {
        const int i = tid + k * nt;
        has[k] = i < n;
        for (int c = 0; c < 3; ++c) p[k][c] = has[k] ? (double)pc[(size_t)i * 3 + c] : 0.0;
        key[k] = gpf_height_key((float)gpf_height(p[k], vertical_axis)); // the double holds an fp32 value: the cast is exact
    }

    // seed height: the mean of the n_lpr smallest heights
    int rank_in_ties;
    const unsigned kth = gpf_select(key, has, n_lpr, sh, rank_in_ties);
    double below[1] = {0.0};
#pragma unroll
    for (int k = 0; k < PTS; ++k)
        if (has[k] && key[k] < kth) below[0] += gpf_height(p[k], vertical_axis);
    gpf_block_sums(below, sh);
    const double lpr = (below[0] + (double)rank_in_ties * (double)gpf_key_height(kth)) / (double)n_lpr;

    bool success = false;
    int attempts = 0;
    for (int a = 0; a < max_attempts; ++a) {
        attempts = a + 1;
#pragma unroll
        for (int k = 0; k < PTS; ++k) sel[k] = has[k] && gpf_height(p[k], vertical_axis) < lpr + thresh_seed;
        int state = GPF_FIT_OK;
        for (int it = 0; it < n_iter; ++it) {
            gpf_fit(p, sel, vertical_axis, thresh_seed, sh);
            __syncthreads(); // plane and state are published; their next writer sits behind gpf_block_sums' barriers
            state = sh->state;
            if (state != GPF_FIT_OK) break; // uniform over the workgroup
            double c[3], nrm[3];
            for (int r = 0; r < 3; ++r) {
                c[r] = sh->plane[r];
                nrm[r] = sh->plane[3 + r];
            }
#pragma unroll
            for (int k = 0; k < PTS; ++k) {
                const double d = (p[k][0] - c[0]) * nrm[0] + (p[k][1] - c[1]) * nrm[1] + (p[k][2] - c[2]) * nrm[2];
                sel[k] = has[k] && fabs(d) < thresh_dist;
            }
        }
        if (state == GPF_FIT_OK) {
            success = true;
            break;
        }
        if (state == GPF_GIVE_UP) break;
        thresh_seed = sh->thresh_seed;
    }

    int *ground = ground_all + cloud * n;
#pragma unroll
    for (int k = 0; k < PTS; ++k) {
        const int i = tid + k * nt;
        if (has[k]) ground[i] = success && sel[k] ? 1 : 0;
    }
    if (tid < 6) plane_all[cloud * 6 + tid] = success ? sh->plane[tid] : 0.0;
    if (tid == 0) attempts_all[cloud] = attempts;
}

} // namespace

extern "C" int ogc_ground_plane_fit(int B, int n, const float *pc, int n_iter, int n_lpr, double thresh_seed, double thresh_dist,
                                    int vertical_axis, double *plane, int *is_ground, int *attempts, ogc_stream_t stream) {
    OGC_REQUIRE(B >= 0, "ogc_ground_plane_fit: negative batch");
    if (B == 0) return OGC_OK;
    OGC_REQUIRE(n >= 3, "ogc_ground_plane_fit: a plane needs at least 3 points per cloud, got n = %d", n);
    OGC_REQUIRE(n <= OGC_GPF_MAX_POINTS,
                "ogc_ground_plane_fit: n = %d exceeds OGC_GPF_MAX_POINTS = %d (a thread keeps its points in registers)", n,
                OGC_GPF_MAX_POINTS);
    OGC_REQUIRE(n_lpr >= 1 && n_lpr < n, "ogc_ground_plane_fit: n_lpr = %d, need 1 <= n_lpr < n = %d", n_lpr, n);
    OGC_REQUIRE(n_iter >= 1, "ogc_ground_plane_fit: n_iter = %d, need at least 1", n_iter);
    OGC_REQUIRE(vertical_axis >= 0 && vertical_axis <= 2, "ogc_ground_plane_fit: vertical_axis = %d, need 0, 1 or 2", vertical_axis);
    OGC_REQUIRE(pc && plane && is_ground && attempts, "ogc_ground_plane_fit: null pointer");
    // the fits a cloud can start: the kernel's own additions, counted here so that its attempt loop has a fixed bound
    int max_attempts = 1;
    for (double raised = thresh_seed + GPF_SEED_STEP; !(raised > GPF_SEED_GIVE_UP) && max_attempts <= GPF_ATTEMPT_LIMIT;
         raised += GPF_SEED_STEP)
        ++max_attempts;
    OGC_REQUIRE(max_attempts <= GPF_ATTEMPT_LIMIT,
                "ogc_ground_plane_fit: thresh_seed = %g does not reach %g within %d steps of %g", thresh_seed, GPF_SEED_GIVE_UP,
                GPF_ATTEMPT_LIMIT, GPF_SEED_STEP);
    const int threads = min(GPF_THREADS, ogc_divup(n, OGC_WAVE) * OGC_WAVE);
    const int pts = ogc_divup(n, threads);
#define OGC_GPF_LAUNCH(PTS)                                                                                                      \
    hipLaunchKernelGGL(ground_plane_fit_kernel<PTS>, dim3(B), dim3(threads), 0, (hipStream_t)stream, n, pc, n_iter, n_lpr,       \
                       thresh_seed, thresh_dist, vertical_axis, max_attempts, plane, is_ground, attempts)
    if (pts <= 1) OGC_GPF_LAUNCH(1);
    else if (pts <= 2) OGC_GPF_LAUNCH(2);
    else if (pts <= 4) OGC_GPF_LAUNCH(4);
    else OGC_GPF_LAUNCH(GPF_MAX_PTS);
#undef OGC_GPF_LAUNCH
    OGC_CHECK_LAUNCH("ogc_ground_plane_fit");
    return OGC_OK;
}

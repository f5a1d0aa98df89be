// sup_loss.hip — the supervised mask loss (the reference's losses/seg_loss_sup.py) without its (B, N, K, K) tensors: all the
// loss needs from the points is, per sample, a K x K table of sums for the matching cost and a K-vector of sums for the loss.
//
//   e(p, t)     F.binary_cross_entropy(p, t, reduction='none') in float32: (t - 1) * max(log1p(-p), -100) - t * max(log(p), -100)
//               (the maximum as `a < b ? b : a`, which keeps a NaN), with use_focal times (1 - p_t)^gamma and alpha_t in the
//               order of FocalLoss.forward; one rounding per operation (the library is built with -ffp-contract=off).  A p that
//               is NaN or outside [0, 1] is replaced by NaN before anything is formed from it.
//   match cost  ceil(n / 64) workgroups per sample, each owning 64 points.  The workgroup stages p, the two clamped logarithms
//               (once per (point, slot), not once per pair), t and valid in LDS; thread (i, j) then walks the tile's points in
//               ascending order and adds e * v and (p * t) * v in fp64; 2k more threads add p * v and t * v.  The partial
//               tables go to the caller's scratch buffer; a second launch (one workgroup per sample) adds them in chunk order
//               and forms the two (k, k) costs in fp64, rounded once.
//   loss fwd    the same chunks; thread (slot i, slice s) adds the four terms of its points s, s + S, ... against the label column
//               col4row[b, i] (gathered, the permuted labels are never written), the slices are added in slice order, the chunks
//               in chunk order by the finishing launch (one workgroup), which also forms the two means.
//   loss bwd    one thread per element of the mask, fp64 arithmetic on the widened inputs, no reduction.
// No floating-point atomics, no static device memory (calls on different streams are independent), nothing allocated or
// zero-filled, no synchronisation: every sum has a fixed order, and two calls give identical bits.
#include <math.h>

#include "ogc_common.h"

namespace {

constexpr int SL_THREADS = 256;
constexpr int SL_TILE = OGC_SUP_LOSS_TILE;
constexpr int SL_K = OGC_SUP_LOSS_MAX_K;
constexpr int SL_FIN_THREADS = 1024;

struct SupElem {
    int focal, square, has_alpha;
    float alpha, one_m_alpha, gamma;
};

__device__ __forceinline__ float sl_checked(float p) { return (p >= 0.f && p <= 1.f) ? p : NAN; }
__device__ __forceinline__ float sl_floor100(float l) { return l < -100.f ? -100.f : l; } // std::max(l, -100): a NaN stays

__device__ __forceinline__ float sl_elem(float p, float lp, float lq, float t, const SupElem &f) {
    const float ce = (t - 1.f) * lq - t * lp;
    if (!f.focal) return ce;
    const float p_t = t * p + (1.f - t) * (1.f - p);
    const float base = 1.f - p_t;
    float loss = ce * (f.square ? base * base : powf(base, f.gamma));
    if (f.has_alpha) loss = (f.alpha * t + f.one_m_alpha * (1.f - t)) * loss;
    return loss;
}

__global__ __launch_bounds__(SL_THREADS) void sup_cost_partial_kernel(int n, int k, int chunks, const float *__restrict__ mask_all,
                                                                      const float *__restrict__ gt_all,
                                                                      const float *__restrict__ valid_all, SupElem f,
                                                                      double *__restrict__ part) {
    __shared__ float s_p[SL_TILE * SL_K], s_lp[SL_TILE * SL_K], s_lq[SL_TILE * SL_K], s_t[SL_TILE * SL_K], s_v[SL_TILE];
    const int tid = threadIdx.x;
    const int chunk = (int)(blockIdx.x % (unsigned)chunks);
    const size_t b = blockIdx.x / (unsigned)chunks;
    const int n0 = chunk * SL_TILE;
    const int cnt = min(SL_TILE, n - n0);
    const size_t row0 = b * (size_t)n + n0;
    const float *mask = mask_all + row0 * k, *gt = gt_all + row0 * k;
    for (int e = tid; e < cnt * k; e += SL_THREADS) {
        const float p = sl_checked(mask[e]);
        s_p[e] = p;
        s_lp[e] = sl_floor100(logf(p));
        s_lq[e] = sl_floor100(log1pf(-p));
        s_t[e] = gt[e];
    }
    for (int q = tid; q < cnt; q += SL_THREADS) s_v[q] = valid_all ? valid_all[row0 + q] : 1.f;
    __syncthreads();

    const int kk = k * k;
    double *out = part + (b * chunks + chunk) * (size_t)(2 * kk + 2 * k);
    for (int pair = tid; pair < kk; pair += SL_THREADS) {
        const int i = pair / k, j = pair % k;
        double ce = 0.0, pt = 0.0;
        for (int q = 0; q < cnt; ++q) {
            const float p = s_p[q * k + i], t = s_t[q * k + j], v = s_v[q];
            ce += (double)(sl_elem(p, s_lp[q * k + i], s_lq[q * k + i], t, f) * v);
            pt += (double)((p * t) * v);
        }
        out[pair] = ce;
        out[kk + pair] = pt;
    }
    for (int c = tid; c < 2 * k; c += SL_THREADS) {
        const float *src = c < k ? s_p + c : s_t + (c - k);
        double s = 0.0;
        for (int q = 0; q < cnt; ++q) s += (double)(src[q * k] * s_v[q]);
        out[2 * kk + c] = s; // [0, k): sum of p v per predicted slot; [k, 2k): sum of t v per GT slot
    }
}

__global__ __launch_bounds__(SL_THREADS) void sup_cost_finish_kernel(int n, int k, int chunks, const double *__restrict__ part,
                                                                     float *__restrict__ cost_ce, float *__restrict__ cost_dice) {
    __shared__ double tot[2 * SL_K * SL_K + 2 * SL_K];
    const int tid = threadIdx.x, kk = k * k, entries = 2 * kk + 2 * k;
    const size_t b = blockIdx.x;
    const double *src = part + b * chunks * (size_t)entries;
    for (int e = tid; e < entries; e += SL_THREADS) {
        double s = 0.0;
        for (int c = 0; c < chunks; ++c) s += src[(size_t)c * entries + e];
        tot[e] = s;
    }
    __syncthreads();
    for (int pair = tid; pair < kk; pair += SL_THREADS) {
        const int i = pair / k, j = pair % k;
        cost_ce[b * kk + pair] = (float)(tot[pair] / (double)n);
        cost_dice[b * kk + pair] = (float)(1.0 - (2.0 * tot[kk + pair] + 1.0) / (tot[2 * kk + i] + tot[2 * kk + k + j] + 1.0));
    }
}

__global__ __launch_bounds__(SL_THREADS) void sup_loss_partial_kernel(int n, int k, int chunks, const float *__restrict__ mask_all,
                                                                      const float *__restrict__ gt_all,
                                                                      const float *__restrict__ valid_all,
                                                                      const int *__restrict__ col_all, SupElem f,
                                                                      double *__restrict__ part) {
    __shared__ double s_part[SL_THREADS][4];
    const int tid = threadIdx.x;
    const int chunk = (int)(blockIdx.x % (unsigned)chunks);
    const size_t b = blockIdx.x / (unsigned)chunks;
    const int n0 = chunk * SL_TILE;
    const int cnt = min(SL_TILE, n - n0);
    const size_t row0 = b * (size_t)n + n0;
    const int S = SL_THREADS / k, i = tid % k, s = tid / k;
    if (s < S) {
        const int col = col_all[b * k + i];
        const bool matched = col >= 0 && col < k; // nothing is indexed with an entry outside [0, k)
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        for (int q = s; q < cnt; q += S) {
            const size_t row = row0 + q;
            const float p = matched ? sl_checked(mask_all[row * k + i]) : NAN; // an unmatched slot: all four sums NaN
            const float t = matched ? gt_all[row * k + col] : NAN;
            const float v = valid_all ? valid_all[row] : 1.f;
            a0 += (double)(sl_elem(p, sl_floor100(logf(p)), sl_floor100(log1pf(-p)), t, f) * v);
            a1 += (double)((p * t) * v);
            a2 += (double)(p * v);
            a3 += (double)(t * v);
        }
        s_part[tid][0] = a0;
        s_part[tid][1] = a1;
        s_part[tid][2] = a2;
        s_part[tid][3] = a3;
    }
    __syncthreads();
    if (tid < 4 * k) {
        const int slot = tid >> 2, c = tid & 3;
        double total = 0.0;
        for (int u = 0; u < S; ++u) total += s_part[u * k + slot][c];
        part[(b * chunks + chunk) * (size_t)(4 * k) + tid] = total;
    }
}

// one workgroup: sums (B, k, 4) in chunk order, then the two means in a fixed order
__global__ __launch_bounds__(SL_FIN_THREADS) void sup_loss_finish_kernel(int B, int n, int k, int chunks,
                                                                         const double *__restrict__ part, double *sums,
                                                                         float *__restrict__ terms) {
    __shared__ double red[2][SL_FIN_THREADS];
    const int tid = threadIdx.x;
    const long long rows = (long long)B * k, entries = rows * 4;
    const int per = 4 * k;
    for (long long e = tid; e < entries; e += SL_FIN_THREADS) {
        const size_t b = (size_t)(e / per);
        const double *src = part + b * chunks * (size_t)per + (e % per);
        double s = 0.0;
        for (int c = 0; c < chunks; ++c) s += src[(size_t)c * per];
        sums[e] = s;
    }
    __syncthreads(); // the workgroup reads back its own stores
    double ce = 0.0, dice = 0.0;
    for (long long r = tid; r < rows; r += SL_FIN_THREADS) {
        const double *q = sums + r * 4;
        ce += q[0];
        dice += 1.0 - (2.0 * q[1] + 1.0) / (q[2] + q[3] + 1.0);
    }
    red[0][tid] = ce;
    red[1][tid] = dice;
    __syncthreads();
    for (int off = SL_FIN_THREADS / 2; off > 0; off >>= 1) {
        if (tid < off) {
            red[0][tid] += red[0][tid + off];
            red[1][tid] += red[1][tid + off];
        }
        __syncthreads();
    }
    if (tid == 0) {
        terms[0] = (float)(red[0][0] / ((double)B * (double)n * (double)k));
        terms[1] = (float)(red[1][0] / (double)rows);
    }
}

struct SupElemD {
    int focal, has_alpha;
    double alpha, gamma;
};

__device__ __forceinline__ double sl_floor100d(double l) { return l < -100.0 ? -100.0 : l; }

__global__ __launch_bounds__(SL_THREADS) void sup_loss_bwd_kernel(long long total, int B, int n, int k,
                                                                  const float *__restrict__ mask, const float *__restrict__ gt,
                                                                  const float *__restrict__ valid, const int *__restrict__ col_all,
                                                                  const double *__restrict__ sums, SupElemD f, double w_ce,
                                                                  double w_dice, const float *__restrict__ grad_out,
                                                                  float *__restrict__ grad_mask) {
    const long long e = (long long)blockIdx.x * SL_THREADS + threadIdx.x;
    if (e >= total) return;
    const long long row = e / k;
    const int i = (int)(e % k);
    const long long r = (row / n) * k + i; // b * k + i
    const int col = col_all[r];
    if (col < 0 || col >= k) {
        grad_mask[e] = NAN;
        return;
    }
    const double p = (double)sl_checked(mask[e]), t = (double)gt[row * k + col], v = valid ? (double)valid[row] : 1.0;
    const double den = (1.0 - p) * p;
    double d = (p - t) / (den < 1e-12 ? 1e-12 : den); // torch's binary_cross_entropy_backward
    if (f.focal) {
        const double ce = (t - 1.0) * sl_floor100d(log1p(-p)) - t * sl_floor100d(log(p));
        const double base = 1.0 - (t * p + (1.0 - t) * (1.0 - p)); // d base / d p = 1 - 2 t
        d = d * pow(base, f.gamma) + ce * (f.gamma * pow(base, f.gamma - 1.0) * (1.0 - 2.0 * t));
        if (f.has_alpha) d *= f.alpha * t + (1.0 - f.alpha) * (1.0 - t);
    }
    const double *q = sums + r * 4;
    const double D = q[2] + q[3] + 1.0;
    const double dd = ((2.0 * q[1] + 1.0) * v - 2.0 * t * v * D) / (D * D) / ((double)B * (double)k);
    const double g = (double)grad_out[0];
    grad_mask[e] = (float)(g * (w_ce * (d * v / ((double)B * (double)n * (double)k)) + w_dice * dd));
}

int sl_check(const char *name, int B, int n, int k, double alpha, double gamma) {
    OGC_REQUIRE(n >= 1, "%s: n = %d, need at least one point per sample", name, n);
    OGC_REQUIRE(k >= 1 && k <= SL_K, "%s: k = %d, need 1 <= k <= %d slots", name, k, SL_K);
    OGC_REQUIRE(isfinite(gamma) && gamma >= 1.0, "%s: gamma = %g, need a finite value >= 1", name, gamma);
    OGC_REQUIRE(!isnan(alpha), "%s: alpha is NaN", name);
    OGC_REQUIRE((long long)B * ogc_divup(n, SL_TILE) < (1ll << 31), "%s: B = %d, n = %d: too many workgroups", name, B, n);
    return OGC_OK;
}

SupElem sl_elem_params(int use_focal, double alpha, double gamma) {
    SupElem f;
    f.focal = use_focal != 0;
    f.square = gamma == 2.0;
    f.has_alpha = alpha >= 0.0;
    f.alpha = (float)alpha;
    f.one_m_alpha = (float)(1.0 - alpha);
    f.gamma = (float)gamma;
    return f;
}

} // namespace

extern "C" long long ogc_sup_loss_ws_doubles(int B, int n, int k) {
    if (B < 1 || n < 1 || k < 1 || k > SL_K) return 0;
    return (long long)B * ogc_divup(n, SL_TILE) * (2ll * k * k + 2ll * k); // >= the 4k per chunk of the loss itself
}

extern "C" int ogc_sup_match_cost(int B, int n, int k, const float *mask, const float *gt_mask, const float *valid,
                                  int use_focal, double alpha, double gamma, double *ws, float *cost_ce, float *cost_dice,
                                  ogc_stream_t stream) {
    OGC_REQUIRE(B >= 0, "ogc_sup_match_cost: negative batch");
    if (B == 0) return OGC_OK;
    if (int rc = sl_check("ogc_sup_match_cost", B, n, k, alpha, gamma)) return rc;
    OGC_REQUIRE(mask && gt_mask && ws && cost_ce && cost_dice, "ogc_sup_match_cost: null pointer");
    const int chunks = ogc_divup(n, SL_TILE);
    hipLaunchKernelGGL(sup_cost_partial_kernel, dim3((unsigned)(B * chunks)), dim3(SL_THREADS), 0, (hipStream_t)stream, n, k,
                       chunks, mask, gt_mask, valid, sl_elem_params(use_focal, alpha, gamma), ws);
    OGC_CHECK_LAUNCH("ogc_sup_match_cost");
    hipLaunchKernelGGL(sup_cost_finish_kernel, dim3(B), dim3(SL_THREADS), 0, (hipStream_t)stream, n, k, chunks, ws, cost_ce,
                       cost_dice);
    OGC_CHECK_LAUNCH("ogc_sup_match_cost");
    return OGC_OK;
}

extern "C" int ogc_sup_mask_loss_fwd(int B, int n, int k, const float *mask, const float *gt_mask, const float *valid,
                                     const int *col4row, int use_focal, double alpha, double gamma, double *ws, double *sums,
                                     float *terms, ogc_stream_t stream) {
    OGC_REQUIRE(B >= 0, "ogc_sup_mask_loss_fwd: negative batch");
    if (B == 0) return OGC_OK;
    if (int rc = sl_check("ogc_sup_mask_loss_fwd", B, n, k, alpha, gamma)) return rc;
    OGC_REQUIRE(mask && gt_mask && col4row && ws && sums && terms, "ogc_sup_mask_loss_fwd: null pointer");
    const int chunks = ogc_divup(n, SL_TILE);
    hipLaunchKernelGGL(sup_loss_partial_kernel, dim3((unsigned)(B * chunks)), dim3(SL_THREADS), 0, (hipStream_t)stream, n, k,
                       chunks, mask, gt_mask, valid, col4row, sl_elem_params(use_focal, alpha, gamma), ws);
    OGC_CHECK_LAUNCH("ogc_sup_mask_loss_fwd");
    hipLaunchKernelGGL(sup_loss_finish_kernel, dim3(1), dim3(SL_FIN_THREADS), 0, (hipStream_t)stream, B, n, k, chunks, ws, sums,
                       terms);
    OGC_CHECK_LAUNCH("ogc_sup_mask_loss_fwd");
    return OGC_OK;
}

extern "C" int ogc_sup_mask_loss_bwd(int B, int n, int k, const float *mask, const float *gt_mask, const float *valid,
                                     const int *col4row, int use_focal, double alpha, double gamma, const double *sums,
                                     double w_ce, double w_dice, const float *grad_out, float *grad_mask, ogc_stream_t stream) {
    OGC_REQUIRE(B >= 0, "ogc_sup_mask_loss_bwd: negative batch");
    if (B == 0) return OGC_OK;
    if (int rc = sl_check("ogc_sup_mask_loss_bwd", B, n, k, alpha, gamma)) return rc;
    OGC_REQUIRE(mask && gt_mask && col4row && sums && grad_out && grad_mask, "ogc_sup_mask_loss_bwd: null pointer");
    const long long total = (long long)B * n * k;
    const long long blocks = (total + SL_THREADS - 1) / SL_THREADS;
    OGC_REQUIRE(blocks < (1ll << 31), "ogc_sup_mask_loss_bwd: B * n * k = %lld: too many workgroups", total);
    SupElemD f;
    f.focal = use_focal != 0;
    f.has_alpha = alpha >= 0.0;
    f.alpha = alpha;
    f.gamma = gamma;
    hipLaunchKernelGGL(sup_loss_bwd_kernel, dim3((unsigned)blocks), dim3(SL_THREADS), 0, (hipStream_t)stream, total, B, n, k, mask,
                       gt_mask, valid, col4row, sums, f, w_ce, w_dice, grad_out, grad_mask);
    OGC_CHECK_LAUNCH("ogc_sup_mask_loss_bwd");
    return OGC_OK;
}

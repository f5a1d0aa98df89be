// batch_norm.hip — fused BatchNorm2d (+ ReLU) (+ max over the neighbourhood), forward and backward, for the per-point
// MLPs of the FlowStep3D nets.
//
// Replaces the `F.relu(bn(conv(x)))` chains and the trailing `.max(dim=-1)` of FlowEmbedding / PointNetSetAbstraction
// (reference: utils/flowstep3d_util.py:57-66, :126-138; nn.BatchNorm2d in its default configuration).  MIOpen runs
// BatchNorm on these (B, C, N, nsample) tensors as separate statistics / normalise / backward kernels around NCHW
// transposes, ReLU and the max as further full passes (BatchNorm + max-reduce ≈ 25 % of a FlowStep3D training step).
// Same plan as group_norm.hip with per-channel rows over the whole batch:
//   forward : stats   per channel over (B, HW), fp64 partials          1 read   (skipped when the producing
//                                                                                convolution delivers them)
//             finalize mean, rstd per channel; running statistics        tiny
//             apply   y = relu(a_c x + b_c)      [or max over nsample]   1 read + 1 write  [1 read]
//   backward: sums    ds = sum dy'*x, db = sum dy' per channel           2 reads      (dy' = dy * [y > 0])
//             params  dgamma, dbeta, c2, c3 per channel                  tiny
//             dx      = dy' * gamma_c * rstd_c + c2 * x + c3             2 reads + 1 write
// Semantics of nn.BatchNorm2d: training = batch statistics with biased variance for the normalisation, running
// statistics updated with `momentum` and the UNBIASED variance; evaluation = running statistics, whose gradient is
// the plain affine map (c2 = c3 = 0).
#include <stdlib.h>

#include "norm_dev.h"

namespace {

// ---- finalize folded into the consumers (round 6) ---------------------------------------------------------------------------------
// A training-mode BatchNorm used to be stats -> finalize -> apply forwards and sums -> params -> dx backwards: the two middle
// launches are one thread per channel, ~4.5 us each plus a dependent kernel boundary, 210 of them per FlowStep3D training step
// whose launch thread is as busy as its GPU.  Every workgroup of the apply / dx kernel now derives ITS channel's coefficients from
// the channel's sums itself (the same double-precision expressions, so the same values bit for bit), and the workgroup
// (chunk 0, sample 0) of a channel also writes what the middle launch wrote: mean / rstd / running statistics, dgamma / dbeta.
struct BnFin {   // stats == nullptr: not folded (the coefficients come from mean / rstd / var as before)
    const double *stats;
    int slots;
    double count;
    float momentum;
    float *running_mean, *running_var, *mean_out, *rstd_out;
};

__device__ __forceinline__ void bn_fin(const BnFin &f, int c, int ch, float eps, bool writer, float &mean, float &rstd) {
    double sum = 0.0, sumsq = 0.0;
    for (int sl = 0; sl < f.slots; ++sl) {
        sum += f.stats[((size_t)sl * c + ch) * 2];
        sumsq += f.stats[((size_t)sl * c + ch) * 2 + 1];
    }
    const double m = sum / f.count;
    const double var = fmax(sumsq / f.count - m * m, 0.0);
    mean = (float)m;
    rstd = (float)(1.0 / sqrt(var + (double)eps));
    if (writer) {
        f.mean_out[ch] = mean;
        f.rstd_out[ch] = rstd;
        if (f.running_mean && f.running_var) {
            const double unbiased = f.count > 1.0 ? var * f.count / (f.count - 1.0) : var;
            f.running_mean[ch] = (float)((1.0 - (double)f.momentum) * (double)f.running_mean[ch] + (double)f.momentum * m);
            f.running_var[ch] = (float)((1.0 - (double)f.momentum) * (double)f.running_var[ch] + (double)f.momentum * unbiased);
        }
    }
}

struct BnBwdFin {   // dsdb == nullptr: not folded (c2, c3 come from the c2c3 buffer)
    const double *dsdb;
    double count;
    int training;
    float *dgamma, *dbeta;
};

// The two halves of the params step from a channel's sums ds, db (m = mean, r = rstd, g = gamma in double): the coefficients of
// dx = a dy' + c2 x + c3 (evaluation: the plain affine map, both zero), and the parameter gradients.  The folded dx kernels and
// bn_bwd_params_kernel both go through them, so the two routes give the same bits.
__device__ __forceinline__ void bn_c2c3(double ds, double db, double m, double r, double g, double count, int training, float &c2f,
                                        float &c3f) {
    double c2 = 0.0, c3 = 0.0;
    if (training) {
        c2 = g * (db * m - ds) * r * r * r / count;
        c3 = -c2 * m - g * db * r / count;
    }
    c2f = (float)c2;
    c3f = (float)c3;
}
__device__ __forceinline__ void bn_dparams(double ds, double db, double m, double r, float &dgamma, float &dbeta) {
    dgamma = (float)((ds - m * db) * r);
    dbeta = (float)db;
}

__device__ __forceinline__ void bn_bwd_fin(const BnBwdFin &f, int ch, float gamma, float mean, float rstd, bool writer, float &c2f,
                                           float &c3f) {
    const double ds = f.dsdb[(size_t)ch * 2], db = f.dsdb[(size_t)ch * 2 + 1];
    bn_c2c3(ds, db, mean, rstd, gamma, f.count, f.training, c2f, c3f);
    if (writer) bn_dparams(ds, db, mean, rstd, f.dgamma[ch], f.dbeta[ch]);
}

// a, bb of y = a x + bb for channel ch: from the channel's sums (folded finalize), from the running statistics (var != nullptr:
// evaluation with mean = running_mean, no finalize launch) or from mean / rstd
__device__ __forceinline__ void bn_fwd_coeffs(const BnFin &fin, int c, int ch, float eps, const float *__restrict__ gamma,
                                              const float *__restrict__ beta, const float *__restrict__ mean,
                                              const float *__restrict__ rstd, const float *__restrict__ var, float &a, float &bb) {
    float mu, rs;
    if (fin.stats) bn_fin(fin, c, ch, eps, blockIdx.x == 0 && blockIdx.z == 0 && threadIdx.x == 0, mu, rs);
    else { mu = mean[ch]; rs = var ? (float)(1.0 / sqrt((double)var[ch] + (double)eps)) : rstd[ch]; }
    a = rs * gamma[ch];
    bb = beta[ch] - mu * a;
}

// thread 0's pair of sums for channel ch -> acc[ch][0..1] (fp64 atomics); part (deterministic mode, else null): the workgroup's
// pair goes to slab (sample, chunk) of part instead — summed in slab order by ogc_det_reduce_f64
__device__ __forceinline__ void bn_emit_pair(int c, int ch, double s0, double s1, double *acc, double *part) {
    if (threadIdx.x == 0) {
        if (part) {
            double *slab = part + ((size_t)blockIdx.z * gridDim.x + blockIdx.x) * 2 * c;
            slab[(size_t)ch * 2] = s0;
            slab[(size_t)ch * 2 + 1] = s1;
        } else {
            atomicAdd(acc + (size_t)ch * 2, s0);
            atomicAdd(acc + (size_t)ch * 2 + 1, s1);
        }
    }
}

// grid (chunks, C, B): partial sum / sum of squares of one (sample, channel) segment -> ws (bn_emit_pair)
__global__ __launch_bounds__(NORM_THREADS) void bn_stats_kernel(int c, int hw, const float *__restrict__ x,
                                                                double *__restrict__ ws, double *__restrict__ part) {
    __shared__ double smem[2 * NORM_THREADS / 64];
    const int b = blockIdx.z, ch = blockIdx.y;
    const float *p = x + ((size_t)b * c + ch) * hw;
    double s = 0.0, ss = 0.0;
    if ((hw & 3) == 0 && ((uintptr_t)p & 15) == 0) {
        for (int i = (blockIdx.x * NORM_THREADS + threadIdx.x) * 4; i < hw; i += gridDim.x * NORM_THREADS * 4) {
            const float4 v = *reinterpret_cast<const float4 *>(p + i);
            s += (double)((v.x + v.y) + (v.z + v.w));
            ss += (double)((v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w));
        }
    } else {
        for (int i = blockIdx.x * NORM_THREADS + threadIdx.x; i < hw; i += gridDim.x * NORM_THREADS) {
            const float v = p[i];
            s += v;
            ss += (double)v * v;
        }
    }
    norm_block_sum2(s, ss, smem);
    bn_emit_pair(c, ch, s, ss, ws, part);
}

// one thread per channel: the finalize step as a launch of its own (evaluation mode, or OGC_BN_FOLD=0)
__global__ void bn_finalize_kernel(int c, double count, float eps, int training, float momentum,
                                   const double *__restrict__ stats, int slots, float *__restrict__ running_mean,
                                   float *__restrict__ running_var, float *__restrict__ mean_out,
                                   float *__restrict__ rstd_out) {
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= c) return;
    if (!training) {
        mean_out[ch] = running_mean[ch];
        rstd_out[ch] = (float)(1.0 / sqrt((double)running_var[ch] + (double)eps));
        return;
    }
    float mean, rstd;
    bn_fin(BnFin{stats, slots, count, momentum, running_mean, running_var, mean_out, rstd_out}, c, ch, eps, true, mean, rstd);
}

template <bool RELU>
__global__ __launch_bounds__(NORM_THREADS) void bn_apply_kernel(int c, int hw, const float *__restrict__ x,
                                                                const float *__restrict__ gamma,
                                                                const float *__restrict__ beta,
                                                                const float *__restrict__ mean,
                                                                const float *__restrict__ rstd,
                                                                const float *__restrict__ var, float eps,
                                                                float *__restrict__ y, BnFin fin) {
    const int b = blockIdx.z, ch = blockIdx.y;
    float a, bb;
    bn_fwd_coeffs(fin, c, ch, eps, gamma, beta, mean, rstd, var, a, bb);
    const size_t base = ((size_t)b * c + ch) * hw;
    norm_apply_row<RELU>(a, bb, hw, x + base, y + base);
}

// x (B, C, P, S) -> out (B, C, P) = max_s act(a_c x + b_c), argmax (first index on ties); L = S/4 lanes per row
template <bool RELU>
__global__ __launch_bounds__(NORM_THREADS) void bn_apply_maxpool_kernel(int c, int p, int s,
                                                                        const float *__restrict__ x,
                                                                        const float *__restrict__ gamma,
                                                                        const float *__restrict__ beta,
                                                                        const float *__restrict__ mean,
                                                                        const float *__restrict__ rstd,
                                                                        const float *__restrict__ var, float eps,
                                                                        float *__restrict__ out, int *__restrict__ arg, BnFin fin) {
    const int b = blockIdx.z, ch = blockIdx.y;
    float a, bb;
    bn_fwd_coeffs(fin, c, ch, eps, gamma, beta, mean, rstd, var, a, bb);
    norm_apply_maxpool_rows<RELU>(a, bb, p, s, ((size_t)b * c + ch) * p, x, out, arg);
}

// ---- backward ------------------------------------------------------------------------------------------------
template <bool RELU>
__global__ __launch_bounds__(NORM_THREADS) void bn_bwd_sums_kernel(int c, int hw, const float *__restrict__ x,
                                                                   const float *__restrict__ gamma,
                                                                   const float *__restrict__ beta,
                                                                   const float *__restrict__ mean,
                                                                   const float *__restrict__ rstd,
                                                                   const float *__restrict__ dy,
                                                                   double *__restrict__ dsdb, double *__restrict__ part) {
    __shared__ double smem[2 * NORM_THREADS / 64];
    const int b = blockIdx.z, ch = blockIdx.y;
    const float a = rstd[ch] * gamma[ch];
    const float bb = beta[ch] - mean[ch] * a;
    const size_t base = ((size_t)b * c + ch) * hw;
    double s = 0.0, sb = 0.0;
    norm_bwd_sums_row<RELU, float>(a, bb, hw, x + base, dy + base, s, sb);
    norm_block_sum2(s, sb, smem);
    bn_emit_pair(c, ch, s, sb, dsdb, part);
}

// one thread per channel: dgamma, dbeta, and the coefficients of dx = a dy' + c2 x + c3, as a launch of its own (OGC_BN_FOLD=0)
__global__ void bn_bwd_params_kernel(int c, double count, int training, const float *__restrict__ gamma,
                                     const float *__restrict__ mean, const float *__restrict__ rstd,
                                     const double *__restrict__ dsdb, float *__restrict__ dgamma,
                                     float *__restrict__ dbeta, float *__restrict__ c2c3) {
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= c) return;
    const double ds = dsdb[(size_t)ch * 2], db = dsdb[(size_t)ch * 2 + 1];
    bn_dparams(ds, db, mean[ch], rstd[ch], dgamma[ch], dbeta[ch]);
    bn_c2c3(ds, db, mean[ch], rstd[ch], gamma[ch], count, training, c2c3[ch * 2], c2c3[ch * 2 + 1]);
}

template <bool RELU>
__global__ __launch_bounds__(NORM_THREADS) void bn_bwd_dx_kernel(int c, int hw, const float *__restrict__ x,
                                                                 const float *__restrict__ gamma,
                                                                 const float *__restrict__ beta,
                                                                 const float *__restrict__ mean,
                                                                 const float *__restrict__ rstd,
                                                                 const float *__restrict__ c2c3,
                                                                 const float *__restrict__ dy, float *__restrict__ dx, BnBwdFin fin) {
    const int b = blockIdx.z, ch = blockIdx.y;
    const float a = rstd[ch] * gamma[ch];
    const float bb = beta[ch] - mean[ch] * a;
    float c2, c3;
    if (fin.dsdb) bn_bwd_fin(fin, ch, gamma[ch], mean[ch], rstd[ch], blockIdx.x == 0 && b == 0 && threadIdx.x == 0, c2, c3);
    else { c2 = c2c3[ch * 2]; c3 = c2c3[ch * 2 + 1]; }
    const size_t base = ((size_t)b * c + ch) * hw;
    const float *px = x + base, *pd = dy + base;
    float *po = dx + base;
    if ((hw & 3) == 0 && (((uintptr_t)px | (uintptr_t)pd | (uintptr_t)po) & 15) == 0) {
        for (int i = (blockIdx.x * NORM_THREADS + threadIdx.x) * 4; i < hw; i += gridDim.x * NORM_THREADS * 4) {
            const float4 v = *reinterpret_cast<const float4 *>(px + i);
            float4 d = *reinterpret_cast<const float4 *>(pd + i);
            if (RELU) norm_relu_gate(a, bb, v, d);
            *reinterpret_cast<float4 *>(po + i) = norm_dx(a, c2, c3, v, d);
        }
    } else {
        for (int i = blockIdx.x * NORM_THREADS + threadIdx.x; i < hw; i += gridDim.x * NORM_THREADS) {
            const float v = px[i];
            float d = pd[i];
            if (RELU) d = norm_relu_gate(a, bb, v, d);
            po[i] = norm_dx(a, c2, c3, v, d);
        }
    }
}

// sparse gradient of the max: non-zero only at the arg-max element of each row
template <bool RELU>
__global__ __launch_bounds__(NORM_THREADS) void bn_maxpool_bwd_sums_kernel(int c, int p, int s,
                                                                           const float *__restrict__ x,
                                                                           const float *__restrict__ out,
                                                                           const int *__restrict__ arg,
                                                                           const float *__restrict__ gout,
                                                                           double *__restrict__ dsdb, double *__restrict__ part) {
    __shared__ double smem[2 * NORM_THREADS / 64];
    const int b = blockIdx.z, ch = blockIdx.y;
    double ds = 0.0, db = 0.0;
    norm_maxpool_sums_rows<RELU, float>(p, s, ((size_t)b * c + ch) * p, x, out, arg, gout, nullptr, ds, db);
    norm_block_sum2(ds, db, smem);
    bn_emit_pair(c, ch, ds, db, dsdb, part);
}

template <bool RELU>
__global__ __launch_bounds__(NORM_THREADS) void bn_maxpool_bwd_dx_kernel(int c, int p, int s,
                                                                         const float *__restrict__ x,
                                                                         const float *__restrict__ gamma,
                                                                         const float *__restrict__ rstd,
                                                                         const float *__restrict__ c2c3,
                                                                         const float *__restrict__ out,
                                                                         const int *__restrict__ arg,
                                                                         const float *__restrict__ gout,
                                                                         float *__restrict__ dx, const float *__restrict__ mean,
                                                                         BnBwdFin fin) {
    const int b = blockIdx.z, ch = blockIdx.y;
    const float a = rstd[ch] * gamma[ch];
    float c2, c3;
    if (fin.dsdb) bn_bwd_fin(fin, ch, gamma[ch], mean[ch], rstd[ch], blockIdx.x == 0 && b == 0 && threadIdx.x == 0, c2, c3);
    else { c2 = c2c3[ch * 2]; c3 = c2c3[ch * 2 + 1]; }
    norm_maxpool_dx_rows<RELU>(a, c2, c3, p, s, ((size_t)b * c + ch) * p, x, out, arg, gout, dx);
}

int bn_chunks(int b, int c, int hw) {
    int chunks = 1;
    while ((long long)b * c * chunks < 2048 && hw / (chunks * 2) >= 4096) chunks *= 2;
    return chunks;
}

// OGC_BN_FOLD=0 in the environment: the finalize / params launches of their own, as until round 5 (A/B runs, tests of both)
bool bn_fold_finalize() {
    static const bool on = [] { const char *e = getenv("OGC_BN_FOLD"); return !(e && e[0] == '0'); }();
    return on;
}

// deterministic mode: one slab of 2 c doubles per workgroup of the split (grid.x chunks x grid.z samples), every entry written
double *bn_partials(const char *name, dim3 grid, int c, hipStream_t s) {
    if (!ogc_deterministic()) return nullptr;
    double *part = static_cast<double *>(ogc_det_scratch(s, sizeof(double) * 2 * (size_t)c * grid.x * grid.z));
    if (!part) ogc_set_error("%s (deterministic): no scratch memory", name);
    return part;
}

// statistics (unless supplied) + finalize; leaves mean / rstd per channel
// fin: training mode — the finalize step is left to the apply kernel (see BnFin); evaluation mode keeps the finalize launch
int bn_prepare(const char *name, int b, int c, int hw, float eps, int training, float momentum, const float *x,
               float *running_mean, float *running_var, float *mean, float *rstd, double *ws, const double *stats,
               int slots, hipStream_t s, BnFin *fin) {
    *fin = BnFin{nullptr, 0, 0.0, 0.f, nullptr, nullptr, nullptr, nullptr};
    if (training && !stats) {
        OGC_REQUIRE(ws, "%s: null workspace", name);
        if (ogc_zero_async(ws, sizeof(double) * 2 * c, s) != hipSuccess) {
            ogc_set_error("%s: memset failed", name);
            return OGC_ERR_LAUNCH;
        }
        const dim3 grid(bn_chunks(b, c, hw), c, b);
        double *part = bn_partials(name, grid, c, s);
        if (ogc_deterministic() && !part) return OGC_ERR_LAUNCH;
        hipLaunchKernelGGL(bn_stats_kernel, grid, dim3(NORM_THREADS), 0, s, c, hw, x, ws, part);
        if (part && ogc_det_reduce_f64(ws, part, (int)(grid.x * grid.z), 2ll * c, 0, s) != hipSuccess) return OGC_ERR_LAUNCH;
        stats = ws;
        slots = 1;
    }
    if (!training) OGC_REQUIRE(running_mean && running_var, "%s: evaluation mode needs running statistics", name);
    if (training && bn_fold_finalize()) {
        *fin = BnFin{stats, slots, (double)b * (double)hw, momentum, running_mean, running_var, mean, rstd};
        return OGC_OK;
    }
    hipLaunchKernelGGL(bn_finalize_kernel, dim3(ogc_divup(c, 256)), dim3(256), 0, s, c, (double)b * (double)hw, eps,
                       training, momentum, stats, slots, running_mean, running_var, mean, rstd);
    return OGC_OK;
}

} // namespace

extern "C" int ogc_batch_norm_fwd(int b, int c, int hw, float eps, int relu, int training, float momentum,
                                  const float *x, const float *gamma, const float *beta, float *running_mean,
                                  float *running_var, float *y, float *mean, float *rstd, double *ws,
                                  const double *stats, int slots, ogc_stream_t stream) {
    OGC_REQUIRE(b >= 0 && c >= 1 && hw >= 1, "ogc_batch_norm_fwd: bad shape");
    if (b == 0) return OGC_OK;
    // evaluation without mean / rstd outputs (nothing will be back-propagated): the affine map is formed from the running
    // statistics inside the apply kernel — one launch
    const bool inline_eval = !training && !mean && !rstd;
    OGC_REQUIRE(x && gamma && beta && y && (inline_eval || (mean && rstd)), "ogc_batch_norm_fwd: null pointer");
    OGC_REQUIRE((long long)c * hw < (1ll << 31) && b <= 65535, "ogc_batch_norm_fwd: one sample exceeds 32-bit indexing");
    hipStream_t s = (hipStream_t)stream;
    const float *var = nullptr;
    BnFin fin{nullptr, 0, 0.0, 0.f, nullptr, nullptr, nullptr, nullptr};
    if (inline_eval) {
        OGC_REQUIRE(running_mean && running_var, "ogc_batch_norm_fwd: evaluation mode needs running statistics");
        mean = running_mean;
        var = running_var;
    } else {
        const int rc = bn_prepare("ogc_batch_norm_fwd", b, c, hw, eps, training, momentum, x, running_mean, running_var,
                                  mean, rstd, ws, stats, slots, s, &fin);
        if (rc != OGC_OK) return rc;
    }
    dim3 grid(bn_chunks(b, c, hw), c, b);
    norm_relu_dispatch(relu, [&](auto r) {
        hipLaunchKernelGGL(bn_apply_kernel<r.value>, grid, dim3(NORM_THREADS), 0, s, c, hw, x, gamma, beta, mean, rstd, var, eps,
                           y, fin);
    });
    OGC_CHECK_LAUNCH("ogc_batch_norm_fwd");
    return OGC_OK;
}

extern "C" int ogc_batch_norm_bwd(int b, int c, int hw, int relu, int training, const float *x, const float *gamma,
                                  const float *beta, const float *mean, const float *rstd, const float *grad_y,
                                  float *grad_x, float *grad_gamma, float *grad_beta, double *ws,
                                  ogc_stream_t stream) {
    OGC_REQUIRE(b >= 0 && c >= 1 && hw >= 1, "ogc_batch_norm_bwd: bad shape");
    if (b == 0) return OGC_OK;
    // before the pointers are looked at: b is a grid dimension, c * hw the span of the kernels' int offsets
    OGC_REQUIRE((long long)c * hw < (1ll << 31) && b <= 65535, "ogc_batch_norm_bwd: one sample exceeds 32-bit indexing");
    OGC_REQUIRE(x && gamma && beta && mean && rstd && grad_y && grad_x && grad_gamma && grad_beta && ws,
                "ogc_batch_norm_bwd: null pointer");
    hipStream_t s = (hipStream_t)stream;
    double *dsdb = ws; // [c][2] fp64, then c2c3 [c][2] fp32
    float *c2c3 = reinterpret_cast<float *>(ws + (size_t)2 * c);
    if (ogc_zero_async(dsdb, sizeof(double) * 2 * c, s) != hipSuccess) {
        ogc_set_error("ogc_batch_norm_bwd: memset failed");
        return OGC_ERR_LAUNCH;
    }
    dim3 grid(bn_chunks(b, c, hw), c, b);
    double *part = bn_partials("ogc_batch_norm_bwd", grid, c, s);
    if (ogc_deterministic() && !part) return OGC_ERR_LAUNCH;
    norm_relu_dispatch(relu, [&](auto r) {
        hipLaunchKernelGGL(bn_bwd_sums_kernel<r.value>, grid, dim3(NORM_THREADS), 0, s, c, hw, x, gamma, beta, mean, rstd,
                           grad_y, dsdb, part);
    });
    if (part && ogc_det_reduce_f64(dsdb, part, (int)(grid.x * grid.z), 2ll * c, 0, s) != hipSuccess) return OGC_ERR_LAUNCH;
    BnBwdFin bfin{nullptr, 0.0, 0, nullptr, nullptr};
    if (bn_fold_finalize()) bfin = BnBwdFin{dsdb, (double)b * (double)hw, training, grad_gamma, grad_beta};
    else
        hipLaunchKernelGGL(bn_bwd_params_kernel, dim3(ogc_divup(c, 256)), dim3(256), 0, s, c, (double)b * (double)hw,
                           training, gamma, mean, rstd, dsdb, grad_gamma, grad_beta, c2c3);
    norm_relu_dispatch(relu, [&](auto r) {
        hipLaunchKernelGGL(bn_bwd_dx_kernel<r.value>, grid, dim3(NORM_THREADS), 0, s, c, hw, x, gamma, beta, mean, rstd, c2c3,
                           grad_y, grad_x, bfin);
    });
    OGC_CHECK_LAUNCH("ogc_batch_norm_bwd");
    return OGC_OK;
}

extern "C" int ogc_batch_norm_maxpool_fwd(int b, int c, int p, int s, float eps, int relu, int training, float momentum,
                                          const float *x, const float *gamma, const float *beta, float *running_mean,
                                          float *running_var, float *out, int *argmax, float *mean, float *rstd,
                                          double *ws, const double *stats, int slots, ogc_stream_t stream) {
    OGC_REQUIRE(b >= 0 && c >= 1 && p >= 1, "ogc_batch_norm_maxpool_fwd: bad shape");
    if (!norm_pool_shape_ok(s) || ((uintptr_t)x & 15) != 0) {
        ogc_set_error("ogc_batch_norm_maxpool_fwd: nsample=%d must be a power of two in [4,256] and x 16-byte aligned", s);
        return OGC_ERR_UNSUPPORTED;
    }
    if (b == 0) return OGC_OK;
    const bool inline_eval = !training && !mean && !rstd; // as in ogc_batch_norm_fwd
    OGC_REQUIRE(x && gamma && beta && out && argmax && (inline_eval || (mean && rstd)),
                "ogc_batch_norm_maxpool_fwd: null pointer");
    OGC_REQUIRE((long long)c * p * s < (1ll << 31) && b <= 65535,
                "ogc_batch_norm_maxpool_fwd: one sample exceeds 32-bit indexing");
    hipStream_t st = (hipStream_t)stream;
    const float *var = nullptr;
    BnFin fin{nullptr, 0, 0.0, 0.f, nullptr, nullptr, nullptr, nullptr};
    if (inline_eval) {
        OGC_REQUIRE(running_mean && running_var, "ogc_batch_norm_maxpool_fwd: evaluation mode needs running statistics");
        mean = running_mean;
        var = running_var;
    } else {
        const int rc = bn_prepare("ogc_batch_norm_maxpool_fwd", b, c, p * s, eps, training, momentum, x, running_mean,
                                  running_var, mean, rstd, ws, stats, slots, st, &fin);
        if (rc != OGC_OK) return rc;
    }
    dim3 grid(norm_pool_blocks(b, c, p, s), c, b);
    norm_relu_dispatch(relu, [&](auto r) {
        hipLaunchKernelGGL(bn_apply_maxpool_kernel<r.value>, grid, dim3(NORM_THREADS), 0, st, c, p, s, x, gamma, beta, mean,
                           rstd, var, eps, out, argmax, fin);
    });
    OGC_CHECK_LAUNCH("ogc_batch_norm_maxpool_fwd");
    return OGC_OK;
}

extern "C" int ogc_batch_norm_maxpool_bwd(int b, int c, int p, int s, int relu, int training, const float *x,
                                          const float *gamma, const float *mean, const float *rstd, const float *out,
                                          const int *argmax, const float *grad_out, float *grad_x, float *grad_gamma,
                                          float *grad_beta, double *ws, ogc_stream_t stream) {
    OGC_REQUIRE(b >= 0 && c >= 1 && p >= 1, "ogc_batch_norm_maxpool_bwd: bad shape");
    if (!norm_pool_shape_ok(s) || (((uintptr_t)x | (uintptr_t)grad_x) & 15) != 0) {
        ogc_set_error("ogc_batch_norm_maxpool_bwd: nsample=%d must be a power of two in [4,256], tensors 16-byte aligned",
                      s);
        return OGC_ERR_UNSUPPORTED;
    }
    if (b == 0) return OGC_OK;
    OGC_REQUIRE((long long)c * p * s < (1ll << 31) && b <= 65535,
                "ogc_batch_norm_maxpool_bwd: one sample exceeds 32-bit indexing");
    OGC_REQUIRE(x && gamma && mean && rstd && out && argmax && grad_out && grad_x && grad_gamma && grad_beta && ws,
                "ogc_batch_norm_maxpool_bwd: null pointer");
    hipStream_t st = (hipStream_t)stream;
    double *dsdb = ws;
    float *c2c3 = reinterpret_cast<float *>(ws + (size_t)2 * c);
    if (ogc_zero_async(dsdb, sizeof(double) * 2 * c, st) != hipSuccess) {
        ogc_set_error("ogc_batch_norm_maxpool_bwd: memset failed");
        return OGC_ERR_LAUNCH;
    }
    int bs = ogc_divup(p, NORM_THREADS);
    while (bs > 1 && (long long)bs * c * b > 4096) bs = (bs + 1) / 2;
    dim3 gsum(bs, c, b);
    double *part = bn_partials("ogc_batch_norm_maxpool_bwd", gsum, c, st);
    if (ogc_deterministic() && !part) return OGC_ERR_LAUNCH;
    norm_relu_dispatch(relu, [&](auto r) {
        hipLaunchKernelGGL(bn_maxpool_bwd_sums_kernel<r.value>, gsum, dim3(NORM_THREADS), 0, st, c, p, s, x, out, argmax,
                           grad_out, dsdb, part);
    });
    if (part && ogc_det_reduce_f64(dsdb, part, (int)(gsum.x * gsum.z), 2ll * c, 0, st) != hipSuccess) return OGC_ERR_LAUNCH;
    BnBwdFin bfin{nullptr, 0.0, 0, nullptr, nullptr};
    if (bn_fold_finalize()) bfin = BnBwdFin{dsdb, (double)b * (double)p * (double)s, training, grad_gamma, grad_beta};
    else
        hipLaunchKernelGGL(bn_bwd_params_kernel, dim3(ogc_divup(c, 256)), dim3(256), 0, st, c,
                           (double)b * (double)p * (double)s, training, gamma, mean, rstd, dsdb, grad_gamma, grad_beta, c2c3);
    dim3 grid(norm_pool_blocks(b, c, p, s), c, b);
    norm_relu_dispatch(relu, [&](auto r) {
        hipLaunchKernelGGL(bn_maxpool_bwd_dx_kernel<r.value>, grid, dim3(NORM_THREADS), 0, st, c, p, s, x, gamma, rstd, c2c3,
                           out, argmax, grad_out, grad_x, mean, bfin);
    });
    OGC_CHECK_LAUNCH("ogc_batch_norm_maxpool_bwd");
    return OGC_OK;
}

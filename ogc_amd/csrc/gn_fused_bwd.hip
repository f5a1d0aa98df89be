// gn_fused_bwd.hip — backward of  y = conv( relu( GroupNorm(y_prev) ) )  without the GroupNorm backward passes.
//
// Inside a SharedMLP (reference utils/nn_util.py:45-85: Conv2d 1x1 -> GroupNorm -> ReLU, repeated) the normalised
// activation z = relu(a y_prev + bb) (a, bb per sample and channel: the GroupNorm folded into an affine map) is never
// stored: the convolution and its weight gradient recompute it while loading y_prev (conv1x1.hip).  The backward pass
// of one such layer used to be
//     dW   = g_y z^T                      (weight gradient, reads y_prev and g_y)
//     g_z  = W^T g_y                      (input gradient, writes g_z)
//     S1, S2 per (sample, group)          (GroupNorm sums, reads y_prev and g_z)
//     g_prev = alpha mask g_z + c2 y_prev + c3      (GroupNorm adjoint, reads y_prev and g_z, writes g_prev)
// — nine passes over a tensor of the activation's size, five of them in the two GroupNorm kernels (3.1 ms of a 14 ms
// C4 step, all of it re-reading).  Both GroupNorm sums follow from two MOMENT MATRICES the weight-gradient kernel can
// accumulate next to each other:   with mask = [a y_prev + bb > 0],
//     H  = g_y mask^T,   H2 = g_y (mask . y_prev)^T              (cout x cin each, per sample)
//     dW = sum_b  H2 diag(a_b) + H diag(bb_b)
//     T1[k] = sum_pos g_z[k] mask[k]          = sum_m W[m,k] H[m,k]
//     T2[k] = sum_pos g_z[k] mask[k] y_prev[k] = sum_m W[m,k] H2[m,k]
// so the sums are known BEFORE the input gradient is formed, and the input-gradient GEMM applies the adjoint in its
// epilogue (it holds the g_z tile; it reads the matching y_prev tile) and writes g_prev directly: g_z never exists.
// Five passes instead of nine: weight gradient 2 reads, input gradient 2 reads + 1 write.
//   ogc_conv1x1_wgrad_moments   H, H2          (v_mfma_f32_16x16x4_f32, two accumulator sets)
//   ogc_gn_moments_combine      dW, dgamma, dbeta, and alpha / c2 / c3 per (sample, channel)
//   ogc_conv1x1_dgrad_adjoint   g_prev
#include "conv1x1_shared.h" // v4f, WG_WAVES, ogc_pooled_grad, the operand precision switch ogc_g_matmul_bf16 (conv1x1.hip)
#include "act_io.h"
#include "first_conv.h"
#include "live_steps.h" // LiveIn, live_check (the lists are made in live_steps.hip)
#include <type_traits>

namespace {

// ---- moment matrices ------------------------------------------------------------------------------------------------
// Same operand layout as conv1x1_wgrad_kernel: for a step of 16 positions lane (i = l & 15, k = l >> 4) loads ONE float4 =
// row (c0 + i), positions pb + 4k .. 4k+3; MFMA k-slot k of sub-step s is position pb + 4k + s for both operands.
// A workgroup stays inside one sample (blockIdx.x = sample * chunks + chunk): H / H2 are per sample.
// POOLED: g_y is the gradient of a max-pooled GroupNorm in sparse form (ogc_group_norm_maxpool_bwd_sparse): `dy` is the
// convolution's OUTPUT y, and g_y[row, pos] = fmaf(c2, y, c3) + (pos % S == arg ? ag : 0) is rebuilt from coef2[b, row] =
// (c2, c3) and inj[b, row, pos / S] = (ag, arg) — a step's 16 positions lie inside one neighbourhood (S = 16, 32, 64).
// AT: element type of x and dy (float / ogc_bf16: act_io.h).
// FIRST (0: off, else the CP of first_conv.h): x is the output of a first convolution that was never stored; a lane rebuilds its
// CIB float4 of it from the x0 values at its four positions (loaded in x's place) and the rows of W1 it holds in registers.
// LIST: the wave walks entries of the sample's live-step list (LiveIn: live_steps.h) instead of consecutive steps, its share derived
// from the list's length so that the live steps spread over all workgroups of the sample; the g_y operand of an entry's last
// position is multiplied by the entry's weight (the skipped repeats of that column).
// The body both moment kernels share is moments_body.inc + moments_walk.inc.  What they differ in: the STEP — positions per step
// (1 << SHIFT) and per lane (PER), what a lane loads, where its positions lie inside a neighbourhood — and `fma`, the transform
// from the loaded dy / x to the MFMA operands with the products into acc1 (H) and acc2 (H2), which each kernel spells itself.
struct MomentStep16 { // fp32 tensors, 16 positions per step
    static constexpr int SHIFT = 4, PER = 4;
    typedef float4 Raw;
    template <typename T>
    static __device__ inline void ld(const T *p, Raw &r) { r = ogc_ld4(p); }
    // (the step lies inside one neighbourhood: pb is a multiple of 16)
    static __device__ inline int centre(int pb, int k, int s_shift) { return pb >> s_shift; }
    static __device__ inline int inside(int pb, int k, int smask) { return (pb & smask) + 4 * k; }
};

template <int COB, int CIB, bool POOLED, typename AT = float, int FIRST = 0, bool LIST = false>
__global__ __launch_bounds__(WG_WAVES *OGC_WAVE) void wgrad_moments_kernel(int cin, int cout, int hw, int chunks,
                                                                           int steps_per_wave, int relu,
                                                                           const AT *__restrict__ x,   // y_prev (B, cin, hw)
                                                                           const AT *__restrict__ dy,  // g_y (B, cout, hw)
                                                                           const float *__restrict__ aff_a,
                                                                           const float *__restrict__ aff_b,
                                                                           const float2 *__restrict__ coef2, // (B, cout)
                                                                           const float2 *__restrict__ inj,   // (B, cout, hw >> s_shift)
                                                                           int s_shift,
                                                                           float *__restrict__ hm,        // (B, 2, cout, cin)
                                                                           FirstIn first = FirstIn(), LiveIn ls = LiveIn()) {
    typedef MomentStep16 STEP;
#include "moments_body.inc"
    // the transform: g_y rebuilt (POOLED) and weighted (LIST), x rebuilt (FIRST), then the mask and mask . x as fp32 operands
    auto fma = [&](float4(&yv)[COB], const float4(&xraw)[XN], const float2(&jv)[COB], int jpos, int went) {
        if (POOLED) {
#pragma unroll
            for (int a = 0; a < COB; ++a) ogc_pooled_grad(yv[a], pc2[a], pc3[a], jv[a], jpos); // (gn_maxpool_bwd_dx_kernel's expression)
        }
        if constexpr (LIST) { // the step's last position: lane group k == 3, component .w
            const float wl = k == 3 ? (float)(1 + 16 * (went >> LIVE_SHIFT)) : 1.f;
#pragma unroll
            for (int a = 0; a < COB; ++a) yv[a].w *= wl;
        }
        float4 x0v[FIRST ? FIRST : 1];
        if constexpr (FIRST > 0) {
#pragma unroll
            for (int e = 0; e < FIRST; ++e) x0v[e] = xraw[e];
            ogc_first_mask<FIRST>(x0v, first.c0, true);
        }
        float4 m1[CIB], m2[CIB];
#pragma unroll
        for (int c = 0; c < CIB; ++c) {
            float4 v;
            if constexpr (FIRST > 0) v = ogc_first_row<FIRST>(x0v, w1r[c]);
            else v = xraw[c];
            // mask = [a y + bb > 0] (relu); without relu: all ones
            const bool bx = relu ? fmaf(ca[c], v.x, cb[c]) > 0.f : true;
            const bool by = relu ? fmaf(ca[c], v.y, cb[c]) > 0.f : true;
            const bool bz = relu ? fmaf(ca[c], v.z, cb[c]) > 0.f : true;
            const bool bw = relu ? fmaf(ca[c], v.w, cb[c]) > 0.f : true;
            m1[c] = make_float4(bx ? 1.f : 0.f, by ? 1.f : 0.f, bz ? 1.f : 0.f, bw ? 1.f : 0.f);
            m2[c] = make_float4(bx ? v.x : 0.f, by ? v.y : 0.f, bz ? v.z : 0.f, bw ? v.w : 0.f);
        }
#pragma unroll
        for (int a = 0; a < COB; ++a)
#pragma unroll
            for (int c = 0; c < CIB; ++c) {
                acc1[a][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(yv[a].x, m1[c].x, acc1[a][c], 0, 0, 0);
                acc2[a][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(yv[a].x, m2[c].x, acc2[a][c], 0, 0, 0);
                acc1[a][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(yv[a].y, m1[c].y, acc1[a][c], 0, 0, 0);
                acc2[a][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(yv[a].y, m2[c].y, acc2[a][c], 0, 0, 0);
                acc1[a][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(yv[a].z, m1[c].z, acc1[a][c], 0, 0, 0);
                acc2[a][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(yv[a].z, m2[c].z, acc2[a][c], 0, 0, 0);
                acc1[a][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(yv[a].w, m1[c].w, acc1[a][c], 0, 0, 0);
                acc2[a][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(yv[a].w, m2[c].w, acc2[a][c], 0, 0, 0);
            }
    };
#include "moments_walk.inc"
}

// ---- the moment matrices from 16-bit tensors --------------------------------------------------------------------------------
// With x and dy stored as bf16 the kernel above moves half the bytes and is no faster: per 16 positions it still issues one load
// per row block (16 rows x 32 bytes each: the vector memory pipe works per row, not per byte) and 128 fp32 MFMAs (0.44 ms of
// matrix time for the 64 x 64 layers of C2's first level, twice what the halved bytes cost).  Here a step is 32 positions — lane
// (i, k) loads SIXTEEN bytes: row i, positions pb + 8 k .. 8 k + 7 — and the products run on gfx950's v_mfma_f32_16x16x32_bf16: a
// lane's eight consecutive positions are its eight k-slots (one MFMA per lane load and accumulator; ogc_mfma_bf16_k32, act_io.h).
// Nothing is rounded that was not already: dy (dense form) is used as loaded, the mask is 0 / 1, mask . x is x or 0; only the
// POOLED form rebuilds g_y in fp32 and rounds it (bf16 operands, as everywhere under ogc_set_matmul_precision(1)).
typedef short v4s16 __attribute__((ext_vector_type(4)));

struct MomentStep32 { // bf16 tensors, 32 positions per step
    static constexpr int SHIFT = 5, PER = 8;
    typedef uint4 Raw;
    static __device__ inline void ld(const ogc_bf16 *p, Raw &r) { r = *reinterpret_cast<const uint4 *>(p); }
    // (a lane's eight positions lie inside one neighbourhood, the step's 32 need not: S >= 16)
    static __device__ inline int centre(int pb, int k, int s_shift) { return (pb + 8 * k) >> s_shift; }
    static __device__ inline int inside(int pb, int k, int smask) { return (pb + 8 * k) & smask; }
};

template <int COB, int CIB, bool POOLED>
__global__ __launch_bounds__(WG_WAVES *OGC_WAVE) void wgrad_moments16_kernel(int cin, int cout, int hw, int chunks,
                                                                             int steps_per_wave, int relu,
                                                                             const ogc_bf16 *__restrict__ x,   // y_prev (B, cin, hw)
                                                                             const ogc_bf16 *__restrict__ dy,  // g_y or y (B, cout, hw)
                                                                             const float *__restrict__ aff_a,
                                                                             const float *__restrict__ aff_b,
                                                                             const float2 *__restrict__ coef2, // (B, cout)
                                                                             const float2 *__restrict__ inj,   // (B, cout, hw >> s_shift)
                                                                             int s_shift,
                                                                             float *__restrict__ hm) {         // (B, 2, cout, cin)
    // What the body asks for by name and this kernel does not take: the first-layer and list forms exist for fp32 tensors only
    // (a step of 32 positions fits neither the x0 rebuild nor the 16-position entries of a list).
    typedef ogc_bf16 AT;
    constexpr int FIRST = 0;
    constexpr bool LIST = false;
    static_assert(FIRST == 0 && !LIST, "wgrad_moments16_kernel: no first-layer form and no list form");
    const FirstIn first = FirstIn();
    const LiveIn ls = LiveIn();
    typedef MomentStep32 STEP;
#include "moments_body.inc"
    // the transform: dy as loaded (POOLED: rebuilt in fp32 and rounded), the mask and mask . x as bit masks on the packed x
    auto fma = [&](const uint4(&yraw)[COB], const uint4(&xraw)[CIB], const float2(&jv)[COB], int jpos, int) {
        v4s16 y0[COB], y1[COB];
#pragma unroll
        for (int a = 0; a < COB; ++a) {
            if (POOLED) { // the expression of gn_maxpool_bwd_dx_kernel on the stored y, rounded to the operand precision
                float f[8];
                ogc_unpack8(yraw[a], f);
                ogc_pooled_grad(f, pc2[a], pc3[a], jv[a], jpos);
                y0[a] = ogc_pack_bf16_rr(f[0], f[1], f[2], f[3]);
                y1[a] = ogc_pack_bf16_rr(f[4], f[5], f[6], f[7]);
            } else {
                y0[a] = __builtin_bit_cast(v4s16, make_uint2(yraw[a].x, yraw[a].y));
                y1[a] = __builtin_bit_cast(v4s16, make_uint2(yraw[a].z, yraw[a].w));
            }
        }
        v4s16 m1a[CIB], m1b[CIB], m2a[CIB], m2b[CIB];
#pragma unroll
        for (int c = 0; c < CIB; ++c) {
            float f[8];
            ogc_unpack8(xraw[c], f);
            unsigned keep[4]; // 0xFFFF per 16-bit half whose position passes the ReLU
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool lo = relu ? fmaf(ca[c], f[2 * e], cb[c]) > 0.f : true;
                const bool hi = relu ? fmaf(ca[c], f[2 * e + 1], cb[c]) > 0.f : true;
                keep[e] = (lo ? 0x0000FFFFu : 0u) | (hi ? 0xFFFF0000u : 0u);
            }
            const unsigned xs[4] = {xraw[c].x, xraw[c].y, xraw[c].z, xraw[c].w};
            m1a[c] = __builtin_bit_cast(v4s16, make_uint2(keep[0] & 0x3F803F80u, keep[1] & 0x3F803F80u)); // bf16 1.0 = 0x3F80
            m1b[c] = __builtin_bit_cast(v4s16, make_uint2(keep[2] & 0x3F803F80u, keep[3] & 0x3F803F80u));
            m2a[c] = __builtin_bit_cast(v4s16, make_uint2(keep[0] & xs[0], keep[1] & xs[1]));
            m2b[c] = __builtin_bit_cast(v4s16, make_uint2(keep[2] & xs[2], keep[3] & xs[3]));
        }
#pragma unroll
        for (int a = 0; a < COB; ++a)
#pragma unroll
            for (int c = 0; c < CIB; ++c) {
                // one v_mfma_f32_16x16x32_bf16 per accumulator: the lane's eight positions are its eight k-slots
                acc1[a][c] = ogc_mfma_bf16_k32(y0[a], y1[a], m1a[c], m1b[c], acc1[a][c]);
                acc2[a][c] = ogc_mfma_bf16_k32(y0[a], y1[a], m2a[c], m2b[c], acc2[a][c]);
            }
    };
#include "moments_walk.inc"
}

// One tile of the ladder below: the launch geometry, then the kernel — the list form wherever a list came along (fp32 only).
template <int COB, int CIB, typename AT, int FIRST, bool POOLED>
void moments_launch(int b, int cin, int cout, int hw, int relu, const AT *x, const AT *dy, const float *pa,
                    const float *pb, const float *coef2, const float *inj, int s_shift, float *hm, hipStream_t s,
                    const FirstIn &first, const LiveIn &ls) {
    const int steps_per_img = sizeof(AT) == 2 ? hw >> 5 : hw >> 4; // (16-bit tensors: 32 positions per step)
    const int tiles = ogc_divup(cout, 16 * COB) * ogc_divup(cin, 16 * CIB);
    long long waves = (2048 / tiles) / b;            // wavefronts per sample and tile pair: ~2048 over the chip
    if (waves < 4) waves = 4;
    int spw = (int)((steps_per_img + waves - 1) / waves);
    if (spw < 8) spw = 8;
    spw = (spw + 1) / 2 * 2;
    const int chunks = ogc_divup(steps_per_img, spw * WG_WAVES);
    dim3 grid(b * chunks, ogc_divup(cout, 16 * COB), ogc_divup(cin, 16 * CIB));
    const float2 *c2 = reinterpret_cast<const float2 *>(coef2), *ij = reinterpret_cast<const float2 *>(inj);
    auto go = [&](auto kernel, auto... tail) {
        hipLaunchKernelGGL(kernel, grid, dim3(WG_WAVES * OGC_WAVE), 0, s, cin, cout, hw, chunks, spw, relu, x, dy, pa, pb, c2, ij,
                           s_shift, hm, tail...);
    };
    if constexpr (sizeof(AT) == 2) go(wgrad_moments16_kernel<COB, CIB, POOLED>);
    else if (ls.steps) // (grid of the worst case: every step live; the kernel derives its share from the list's length)
        go(wgrad_moments_kernel<COB, CIB, POOLED, AT, FIRST, true>, first, ls);
    else go(wgrad_moments_kernel<COB, CIB, POOLED, AT, FIRST>, first, ls);
}

// The tile ladder: (COB, CIB) row and column blocks of 16 per workgroup, by the channel counts; launch(COB, CIB) takes them as
// integral constants.  MAXC: column blocks at most — 2 for the first-layer forms, where beyond 32 channels of y1 the grid's z
// dimension walks the column tiles (the recomputed operand costs registers the <.., 4> forms do not have).  WIDE: the widest
// tile is <4, 4>; without it <4, 2> — the pooled fp32 <4, 4> runs out of registers (256 + 34) and is not compiled.
template <int N>
using TileC = std::integral_constant<int, N>;
template <int MAXC, bool WIDE, typename F>
void moments_ladder(int cin, int cout, F launch) {
    if (cout <= 16 && cin <= 16) launch(TileC<1>(), TileC<1>());
    else if (cout <= 32 && cin <= 16) launch(TileC<2>(), TileC<1>());
    else if (cout <= 32 && (cin <= 32 || MAXC == 2)) launch(TileC<2>(), TileC<2>());
    else if (cin <= 16) launch(TileC<4>(), TileC<1>());
    else if (cin <= 32 || MAXC == 2) launch(TileC<4>(), TileC<2>());
    else if constexpr (MAXC == 4) {
        if (cout <= 32) launch(TileC<2>(), TileC<4>());
        else if constexpr (WIDE) launch(TileC<4>(), TileC<4>());
        else launch(TileC<4>(), TileC<2>());
    }
}

// What every moment entry point ends in, its own checks done: H, H2 zeroed (the kernels add into them), the ladder, the launch.
template <typename AT, int FIRST, bool POOLED>
int moments_run(const char *name, int b, int cin, int cout, int hw, int relu, const AT *x, const AT *dy, const float *pa,
                const float *pb, const float *coef2, const float *inj, int s_shift, float *moments, hipStream_t s,
                const FirstIn &first, const LiveIn &ls) {
    if (ogc_zero_async(moments, sizeof(float) * 2 * (size_t)b * cin * cout, s) != hipSuccess) {
        ogc_set_error("%s: memset failed", name);
        return OGC_ERR_LAUNCH;
    }
    moments_ladder<FIRST ? 2 : 4, !(POOLED && sizeof(AT) == 4)>(cin, cout, [&](auto cob, auto cib) {
        moments_launch<decltype(cob)::value, decltype(cib)::value, AT, FIRST, POOLED>(b, cin, cout, hw, relu, x, dy, pa, pb, coef2, inj,
                                                                                     s_shift, moments, s, first, ls);
    });
    OGC_CHECK_LAUNCH(name);
    return OGC_OK;
}

// ---- dW, the GroupNorm parameter gradients and the coefficients of the adjoint ----------------------------------------------
// blocks [0, b): one per sample — T1, T2 per channel, the two sums per group, alpha / c2 / c3 per channel, and the sample's
// share of dgamma / dbeta; the other blocks: one element of dW per thread.
__global__ __launch_bounds__(256) void moments_combine_kernel(int b, int cin, int cout, int hw, int groups,
                                                              const float *__restrict__ hm, const float *__restrict__ w,
                                                              const float *__restrict__ pa, const float *__restrict__ pb,
                                                              const float *__restrict__ mean, const float *__restrict__ rstd,
                                                              const float *__restrict__ gamma, float *__restrict__ dw,
                                                              float *__restrict__ coef, // (b, cin, 3): alpha, c2, c3
                                                              float *__restrict__ dgamma, float *__restrict__ dbeta) {
    __shared__ double s1[32], s2[32];
    const int cpg = cin / groups;
    if ((int)blockIdx.x < b) {
        const int img = blockIdx.x;
        __shared__ double tt1[512], tt2[512]; // T1, T2 per channel (cin <= 512, checked by the entry point)
        for (int t = threadIdx.x; t < 512; t += blockDim.x) { tt1[t] = 0.0; tt2[t] = 0.0; }
        if (threadIdx.x < 32) { s1[threadIdx.x] = 0.0; s2[threadIdx.x] = 0.0; }
        __syncthreads();
        const float *h1 = hm + (size_t)img * 2 * cout * cin, *h2 = h1 + (size_t)cout * cin;
        // work item = (channel k, row lane ml of 8): consecutive threads take consecutive channels (coalesced rows of H)
        for (int it = threadIdx.x; it < cin * 8; it += blockDim.x) {
            const int ml = it / cin, k = it - ml * cin;
            double t1 = 0.0, t2 = 0.0;
            for (int m = ml; m < cout; m += 8) {
                const double wv = w[(size_t)m * cin + k];
                t1 += wv * h1[(size_t)m * cin + k];
                t2 += wv * h2[(size_t)m * cin + k];
            }
            atomicAdd(&tt1[k], t1);
            atomicAdd(&tt2[k], t2);
        }
        __syncthreads();
        for (int k = threadIdx.x; k < cin; k += blockDim.x) {
            const int g = k / cpg;
            const double mu = mean[img * groups + g], r = rstd[img * groups + g], gm = gamma[k];
            atomicAdd(&s1[g], gm * tt1[k]);                       // S1 = sum_c gamma_c sum_pos g'
            atomicAdd(&s2[g], gm * (tt2[k] - mu * tt1[k]) * r);   // S2 = sum_c gamma_c sum_pos g' xhat
        }
        __syncthreads();
        const double n = (double)cpg * (double)hw;
        for (int k = threadIdx.x; k < cin; k += blockDim.x) {
            const int g = k / cpg;
            const double mu = mean[img * groups + g], r = rstd[img * groups + g];
            const double c2 = -r * r * s2[g] / n;
            const double c3 = -r * s1[g] / n - c2 * mu;
            float *o = coef + ((size_t)img * cin + k) * 3;
            o[0] = (float)((double)gamma[k] * r);
            o[1] = (float)c2;
            o[2] = (float)c3;
        }
        // this sample's share of the GroupNorm parameter gradients (fp32 atomics over the b samples; zeroed by the entry point)
        for (int k = threadIdx.x; k < cin; k += blockDim.x) {
            const int g = k / cpg;
            const double mu = mean[img * groups + g], r = rstd[img * groups + g];
            unsafeAtomicAdd(dgamma + k, (float)((tt2[k] - mu * tt1[k]) * r));
            unsafeAtomicAdd(dbeta + k, (float)tt1[k]);
        }
    } else {
        // one element of dW per thread, summed over the samples in a fixed order
        const long long e = ((long long)blockIdx.x - b) * blockDim.x + threadIdx.x;
        if (e < (long long)cout * cin) {
            const int k = (int)(e % cin);
            float acc = 0.f;
            for (int img = 0; img < b; ++img) {
                const float *h1 = hm + (size_t)img * 2 * cout * cin, *h2 = h1 + (size_t)cout * cin;
                acc += pa[(size_t)img * cin + k] * h2[e] + pb[(size_t)img * cin + k] * h1[e];
            }
            dw[e] = acc;
        }
    }
}

// ---- input gradient with the GroupNorm adjoint in the epilogue -----------------------------------------------------------------
// g_prev[b, m, p] = alpha[b, m] mask (sum_k w[k, m] g_y[b, k, p]) + c2[b, m] y_prev[b, m, p] + c3[b, m]
// The GEMM of conv1x1_gemm_kernel<TRANSPOSE_A = true> (M = cin, K = cout): a wave owns 64 positions, the whole K x 64 tile
// of g_y in registers, A = w^T staged through LDS 64 rows at a time; the epilogue holds four consecutive positions of
// an output row per lane and reads the same four of y_prev.
// POOLED: g_y in the sparse form of ogc_group_norm_maxpool_bwd_sparse, rebuilt from the convolution's output (`gy` = y) as
// in wgrad_moments_kernel; a lane's four positions lie inside one neighbourhood (S >= 4).
// AT: element type of gy, yprev and out (float / ogc_bf16: act_io.h).
// BF: operands rounded to bf16 on v_mfma_f32_16x16x16_bf16, staged as in conv1x1_gemm_kernel (the 16-bit instantiation: at 64 x 64
// channels the fp32 MFMAs of a tile take 3.4 us per wavefront, twice what its halved bytes cost).
// FIRST (0: off, else the CP of first_conv.h): y_prev is the output y1 = conv(x0, W1) of a first convolution that was never
// stored (M = c1 <= 64): its rows are rebuilt from the lane's x0 values, and g_prev is not stored either — nothing reads it but
// the weight gradient of that convolution, dW1[m][c] = sum_p g_prev[m][p] x0[c][p], which the epilogue forms from the four
// positions it holds: summed over the 16 lanes of a DPP row, then over the workgroup's run of first.run position tiles in LDS,
// then one fp32 atomic per element and workgroup into first.dw1.
// LIST (fp32): a wave's tile is FOUR ENTRIES of the sample's live-step list (LiveIn: live_steps.h) instead of 64
// consecutive positions — lane j holds positions 4 (j & 3) .. + 3 of entry 4 tile + (j >> 2); the geometry of S = 16, four
// neighbourhoods per tile, and the pooled table is sized for it (its per-row pair (c2, c3) apart from the per-entry pair (ag, arg):
// at K = 128 the weight tile and a table of whole float4 would not fit 64 KiB).  POOLED writes g_prev at live positions only; FIRST
// multiplies the term of an entry's last position by the entry's weight and derives the workgroup's run of tiles from the list's
// length.  Neither (the plain form, a middle layer between a pooled tail and a layer that reads its gradient densely) reads g_y and
// y_prev at live positions only and writes g_prev DENSELY: the steps an entry skips (s_shift: log2 of the neighbourhood size,
// which bounds them) repeat the entry's last position bit for bit, so the four lanes that hold the entry store that value there.
// The pooled forms' table: (c2, c3, ag, arg) of the wave's K rows x (64 >> s_shift) neighbourhoods through wave-private LDS, read
// back one entry per row right where it is used (held in registers next to the K x 64 tile they cost a wavefront per SIMD).
// Dense: one float4 per row and neighbourhood (cpw columns per row).  LIST: one column per entry of the tile, (ag, arg) per row
// and entry in tabj, then (c2, c3) per row in tabc — 40 bytes per row and wave instead of 64.
// This is the read-back, (c2, c3, ag, arg) of `row` in the lane's neighbourhood (LIST: entry) `mine` of the tile.  The fill is
// text in the kernel: as a function next to this one — five shapes of it: with the table as a struct or as pointers, scalars by
// value or by reference, always_inline or not — it moved the spilled SGPRs of dgrad_adjoint_kernel<33 / 40, true, bf16, true>
// (8 -> 16 and 30 -> 28; <8 / 16 / 25, .., LIST> by one SGPR in the first shape), and with the kernel's own text they stay.
template <bool LIST>
__device__ inline float4 pooled_table_row(const float4 *tab, const float2 *tabj, const float2 *tabc, int cpw, int row, int mine) {
    if constexpr (LIST) {
        const float2 cc = tabc[row], jj = tabj[row * 4 + mine];
        return make_float4(cc.x, cc.y, jj.x, jj.y);
    } else {
        return tab[row * cpw + mine];
    }
}

template <int KQ, bool POOLED, typename AT = float, bool BF = false, int FIRST = 0, bool LIST = false>
__global__ __launch_bounds__(WG_WAVES *OGC_WAVE) void dgrad_adjoint_kernel(int M, int K, int hw, int relu,
                                                                           const float *__restrict__ w,     // (K, M)
                                                                           const AT *__restrict__ gy,    // (B, K, hw)
                                                                           const AT *__restrict__ yprev, // (B, M, hw)
                                                                           const float *__restrict__ pa,
                                                                           const float *__restrict__ pb,
                                                                           const float *__restrict__ coef,  // (B, M, 3)
                                                                           const float2 *__restrict__ coef2, // (B, K)
                                                                           const float2 *__restrict__ inj,   // (B, K, hw >> s_shift)
                                                                           int s_shift,
                                                                           AT *__restrict__ out,         // (B, M, hw)
                                                                           FirstIn first = FirstIn(), LiveIn ls = LiveIn()) {
    extern __shared__ __attribute__((aligned(16))) float a_lds[]; // [64][ogc_a_ld(Kq)] weights (conv_stage.h), then [64][5] coefficients
    __shared__ __attribute__((aligned(16))) float s_w1[FIRST ? FC_MAX_ROWS * FC_MAX_C0 : 4]; // FIRST: W1, zero-padded
    __shared__ float s_dw[FIRST ? FC_MAX_ROWS * FC_MAX_C0 : 4];                              // FIRST: the workgroup's share of dW1
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 15, kk = lane >> 4;
    const int b = blockIdx.y;
    const int Kq = (K + 3) >> 2;
    const AT *inb = gy + (size_t)b * K * hw;
    AT *outb = out + (size_t)b * M * hw;
    const AT *yb = yprev + (size_t)b * M * hw;
    const int a_ld = ogc_a_ld(Kq);
    float *cf = a_lds + (size_t)64 * a_ld;
    int run = FIRST ? first.run : 1; // position tiles of 256 a workgroup walks (one, unless FIRST)
    int n_lv = 0;
    const int *lv_ = nullptr;
    if constexpr (LIST) {
        static_assert(!BF && sizeof(AT) == 4, "list form: fp32");
        n_lv = min(ls.n[b], ls.cap);
        lv_ = ls.steps + (size_t)b * ls.cap;
        const int tiles = (n_lv + 4 * WG_WAVES - 1) / (4 * WG_WAVES); // a workgroup's tile: 16 entries
        if (FIRST) run = (tiles + (int)gridDim.x - 1) / (int)gridDim.x;
        if ((int)blockIdx.x * run >= tiles) return; // (the whole workgroup, ahead of every barrier)
    }
    if constexpr (FIRST > 0) { // (visible to all after the barriers in front of the first tile's MFMAs)
        static_assert(!POOLED && !BF && sizeof(AT) == 4, "first-layer form: dense, fp32");
        ogc_first_stage_w1<WG_WAVES * OGC_WAVE>(s_w1, first.w1, M, first.c0);
        for (int t = threadIdx.x; t < FC_MAX_ROWS * FC_MAX_C0; t += WG_WAVES * OGC_WAVE) s_dw[t] = 0.f;
    }
    for (int it = 0; it < run; ++it) {
        const int tw = (blockIdx.x * run + it) * WG_WAVES + wave; // the wave's tile
        const int p0 = tw * 64;
        const bool live = LIST ? 4 * tw < n_lv : p0 < hw;
        int pos = p0 + 4 * j; // the lane's first position
        bool mine_ok = true;  // LIST: the lane's entry exists (the last tile of a list may hold fewer than four)
        float wl = 1.f;       // LIST: the weight of the lane's LAST position (.w)
        int skipped = 0;      // LIST, plain form: the steps behind the lane's entry that repeat its last position
        if constexpr (LIST) {
            const int q = 4 * tw + (j >> 2);
            mine_ok = q < n_lv;
            const int ent = lv_[min(q, n_lv - 1)];
            const int step = min(ent & LIVE_MASK, (hw >> 4) - 1);
            pos = step * 16 + 4 * (j & 3);
            wl = (j & 3) == 3 ? (float)(1 + 16 * (ent >> LIVE_SHIFT)) : 1.f;
            if constexpr (!POOLED && FIRST == 0) { // (clamped to the steps left in the centre, as the step is clamped to the sample)
                const int tmask = (1 << (s_shift - 4)) - 1;
                skipped = mine_ok ? min(max(ent >> LIVE_SHIFT, 0), tmask - (step & tmask)) : 0;
            }
        }
        const bool lane_live = live && mine_ok;
        float4 x0v[FIRST ? FIRST : 1];
        if constexpr (FIRST > 0) {
            ogc_first_load_raw<FIRST>(x0v, first.x0 + (size_t)b * first.c0 * hw + (live ? pos : 0), first.c0, hw);
            ogc_first_mask<FIRST>(x0v, first.c0, lane_live);
        }

        float4 xin[KQ];
#pragma unroll
        for (int q = 0; q < KQ; ++q) {
            const int row = q * 4 + kk;
            xin[q] = (lane_live && row < K) ? ogc_ld4(inb + (size_t)row * hw + pos) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if (POOLED) { // g_y rebuilt from y through the wave's table (pooled_table_row above)
            const int centres = hw >> s_shift, cpw = LIST ? 4 : 64 >> s_shift; // LIST: one table column per entry of the tile
            float4 *tab = reinterpret_cast<float4 *>(cf + 64 * 5) + (size_t)wave * K * cpw;
            float2 *tabj = reinterpret_cast<float2 *>(cf + 64 * 5) + (size_t)wave * K * 5, *tabc = tabj + K * 4;
            if constexpr (LIST) {
                for (int e = lane; e < K; e += OGC_WAVE) tabc[e] = coef2[(size_t)b * K + e];
            }
            for (int e = lane; e < K * cpw; e += OGC_WAVE) {
                const int row = e / cpw;
                int centre = (p0 >> s_shift) + (e - row * cpw);
                if constexpr (LIST) {
                    const int q = 4 * tw + (e - row * cpw);
                    const int step = min(lv_[min(q, n_lv - 1)] & LIVE_MASK, (hw >> 4) - 1);
                    centre = q < n_lv ? (step * 16) >> s_shift : centres;
                }
                const float2 cc = coef2[(size_t)b * K + row];
                const float2 jj = (live && centre < centres) ? inj[((size_t)b * K + row) * centres + centre]
                                                             : make_float2(0.f, __int_as_float(-1));
                if constexpr (LIST) tabj[e] = jj;
                else tab[e] = make_float4(cc.x, cc.y, jj.x, jj.y);
            }
            __syncthreads();
            const int mine = LIST ? j >> 2 : (4 * j) >> s_shift, jpos = pos & ((1 << s_shift) - 1);
#pragma unroll
            for (int q = 0; q < KQ; ++q) { // the expression of gn_maxpool_bwd_dx_kernel, bit for bit (rows beyond K stay zero)
                const int row = q * 4 + kk;
                if (row < K) { // (implies q < Kq; one predicate per row keeps the masks of 33 rows out of spilled SGPRs)
                    const float4 t = pooled_table_row<LIST>(tab, tabj, tabc, cpw, row, mine);
                    ogc_pooled_grad(xin[q], t.x, t.y, make_float2(t.z, t.w), jpos);
                }
            }
        }
        typedef short v4s __attribute__((ext_vector_type(4)));
        constexpr int GQ = (KQ + 3) / 4;
        v4s xb[BF ? GQ : 1][4]; // BF: the tile as packed bf16 operands (k-slot i of lane group kk = row 4 (4 g + i) + kk)
        if constexpr (BF) {
#pragma unroll
            for (int g = 0; g < GQ; ++g) {
                float4 r[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) r[i] = 4 * g + i < KQ ? xin[4 * g + i] : make_float4(0.f, 0.f, 0.f, 0.f);
                xb[g][0] = ogc_pack_bf16_rr(r[0].x, r[1].x, r[2].x, r[3].x);
                xb[g][1] = ogc_pack_bf16_rr(r[0].y, r[1].y, r[2].y, r[3].y);
                xb[g][2] = ogc_pack_bf16_rr(r[0].z, r[1].z, r[2].z, r[3].z);
                xb[g][3] = ogc_pack_bf16_rr(r[0].w, r[1].w, r[2].w, r[3].w);
            }
        }
        for (int m0 = 0; m0 < M; m0 += 64) {
            // FIRST: M <= 64 — the one row tile and the sample's coefficients are staged for the first position tile of the run and
            // stay; the later tiles of the run meet no barrier and no dependent round trip besides their own loads
            if (FIRST == 0 || it == 0) {
                __syncthreads(); // previous tile fully consumed
                if constexpr (BF) {
                    ogc_stage_weight_tile_bf16<true, WG_WAVES, GQ>(a_lds, w, m0, M, K, Kq); // packed operands of w^T (conv_stage.h)
                } else {
                    ogc_stage_weight_tile<true, WG_WAVES>(a_lds, w, m0, M, K, Kq);
                }
                for (int t = threadIdx.x; t < 64; t += WG_WAVES * OGC_WAVE) {
                    const int m = m0 + t;
                    const bool in = m < M;
                    cf[t * 5 + 0] = in ? pa[(size_t)b * M + m] : 0.f;
                    cf[t * 5 + 1] = in ? pb[(size_t)b * M + m] : 0.f;
                    cf[t * 5 + 2] = in ? coef[((size_t)b * M + m) * 3] : 0.f;
                    cf[t * 5 + 3] = in ? coef[((size_t)b * M + m) * 3 + 1] : 0.f;
                    cf[t * 5 + 4] = in ? coef[((size_t)b * M + m) * 3 + 2] : 0.f;
                }
                __syncthreads();
            }
            const int nblk = min(4, (M - m0 + 15) >> 4);
            // One 16-row block of the tile at a time (unlike conv1x1_gemm_kernel, which runs the four blocks side by side): the
            // block's accumulators are 16 registers instead of 64, its y_prev values (requested before its MFMA loop, consumed
            // after it) another 16 — the epilogue needs both in VGPRs, and holding the whole tile there costs two wavefronts
            // per SIMD.  Four independent accumulators (the four column blocks) keep the MFMA pipe issuing back to back.
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                if (a < nblk) {
                    float4 yv[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int m = m0 + a * 16 + kk * 4 + r;
                        if constexpr (FIRST > 0) { // (rows beyond M meet zero weights, a wave that is not live zero x0 values)
                            float w1r[FIRST];
                            ogc_first_w1_row<FIRST>(w1r, s_w1, m);
                            yv[r] = ogc_first_row<FIRST>(x0v, w1r);
                        } else {
                            yv[r] = (live && m < M) ? ogc_ld4(yb + (size_t)m * hw + pos) : make_float4(0.f, 0.f, 0.f, 0.f);
                        }
                    }
                    v4f acc[4];
#pragma unroll
                    for (int c = 0; c < 4; ++c) acc[c] = (v4f){0.f, 0.f, 0.f, 0.f};
                    if constexpr (BF) {
                        // pairs of groups on v_mfma_f32_16x16x32_bf16, a single last group on the 16x16x16 form — the order of
                        // conv1x1_gemm16_kernel's adjoint form (conv1x1_h.hip), so that the two kernels agree bit for bit
                        const v4s *a_bf = reinterpret_cast<const v4s *>(a_lds);
#pragma unroll
                        for (int g = 0; g + 1 < GQ; g += 2) {
                            if (4 * (g + 1) < Kq) {
                                const v4s av0 = a_bf[(g * 64 + a * 16 + j) * 4 + kk], av1 = a_bf[((g + 1) * 64 + a * 16 + j) * 4 + kk];
#pragma unroll
                                for (int c = 0; c < 4; ++c) acc[c] = ogc_mfma_bf16_k32(av0, av1, xb[g][c], xb[g + 1][c], acc[c]);
                            } else if (4 * g < Kq) {
                                const v4s av = a_bf[(g * 64 + a * 16 + j) * 4 + kk];
#pragma unroll
                                for (int c = 0; c < 4; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(av, xb[g][c], acc[c], 0, 0, 0);
                            }
                        }
                        if constexpr (GQ % 2 == 1) {
                            constexpr int g = GQ - 1;
                            if (4 * g < Kq) {
                                const v4s av = a_bf[(g * 64 + a * 16 + j) * 4 + kk];
#pragma unroll
                                for (int c = 0; c < 4; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(av, xb[g][c], acc[c], 0, 0, 0);
                            }
                        }
                    } else {
#pragma unroll
                        for (int q = 0; q < KQ; ++q) {
                            if (q < Kq) {
                                const float av = a_lds[(a * 16 + j) * a_ld + q * 4 + kk]; // A[m0+16a+j][4q+kk]
                                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xin[q].x, acc[0], 0, 0, 0);
                                acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xin[q].y, acc[1], 0, 0, 0);
                                acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xin[q].z, acc[2], 0, 0, 0);
                                acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xin[q].w, acc[3], 0, 0, 0);
                            }
                        }
                    }
                    if (live) { // (wave-uniform; m is uniform over the 16 lanes of a DPP row)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int mi = a * 16 + kk * 4 + r, m = m0 + mi; // C/D layout: row (l >> 4) * 4 + r, column l & 15
                            if (m < M) {
                                const float fa = cf[mi * 5], fb = cf[mi * 5 + 1], al = cf[mi * 5 + 2], c2 = cf[mi * 5 + 3], c3 = cf[mi * 5 + 4];
                                float4 o = make_float4(acc[0][r], acc[1][r], acc[2][r], acc[3][r]);
                                ogc_gn_adjoint(o, yv[r], fa, fb, al, c2, c3, relu);
                                if constexpr (FIRST > 0) {
                                    float mine = 0.f; // lane j < c0 of the row keeps channel j's sum (every lane of the row holds them all)
                                    if constexpr (LIST) o.w *= wl; // (a lane without an entry holds zeros in x0v)
#pragma unroll
                                    for (int c = 0; c < FIRST; ++c) {
                                        float d = fmaf(o.w, x0v[c].w, fmaf(o.z, x0v[c].z, fmaf(o.y, x0v[c].y, o.x * x0v[c].x)));
                                        d += ogc_dpp_f32<0xB1>(d);
                                        d += ogc_dpp_f32<0x4E>(d);
                                        d += ogc_dpp_f32<0x141>(d);
                                        d += ogc_dpp_f32<0x140>(d);
                                        mine = j == c ? d : mine;
                                    }
                                    if (j < first.c0) atomicAdd(&s_dw[m * FC_MAX_C0 + j], mine);
                                } else {
                                    if (mine_ok) ogc_st4(outb + (size_t)m * hw + pos, o);
                                    if constexpr (LIST && !POOLED) { // the skipped steps: the value of the entry's last position
                                        const float v = ogc_dpp_f32<0xFF>(o.w); // (lane 3 of the quad of lanes that holds the entry)
#pragma unroll
                                        for (int t = 1; t <= 3; ++t)
                                            if (t <= skipped) ogc_st4(outb + (size_t)m * hw + pos + 16 * t, make_float4(v, v, v, v));
                                    }
                                }
                            }
                        }
                    }
                }
            }
        }
    }
    if constexpr (FIRST > 0) {
        __syncthreads();
        for (int t = threadIdx.x; t < M * first.c0; t += WG_WAVES * OGC_WAVE) {
            const float v = s_dw[(t / first.c0) * FC_MAX_C0 + t % first.c0];
            if (v != 0.0f) unsafeAtomicAdd(first.dw1 + t, v);
        }
    }
}

} // namespace

namespace {
int nsample_shift(int nsample) { return nsample == 16 ? 4 : nsample == 32 ? 5 : nsample == 64 ? 6 : -1; }

// The pooled forms' own preconditions (grad_y in the sparse form of ogc_group_norm_maxpool_bwd_sparse: y (B, cout, hw) is the
// convolution's output, hw = centres * nsample); sh: log2 nsample.
int pooled_check(const char *name, int b, int hw, int nsample, const float *coef2, const float *inj, int &sh) {
    sh = nsample_shift(nsample);
    if (sh < 0 || hw % nsample != 0 || (((uintptr_t)coef2 | (uintptr_t)inj) & 7) != 0) {
        ogc_set_error("%s: nsample=%d must be 16, 32 or 64 and divide hw=%d", name, nsample, hw);
        return OGC_ERR_UNSUPPORTED;
    }
    OGC_REQUIRE(b == 0 || (coef2 && inj), "%s: null pointer", name);
    return OGC_OK;
}

// The list forms' entry: the list checked (live_steps.h) ahead of everything else, then run(name, list).
template <typename F>
int with_live(const char *name, const int *live, const int *n_live, int live_cap, int hw, int nsample, F run) {
    LiveIn ls;
    const int rc = live_check(name, live, n_live, live_cap, hw, nsample, ls);
    return rc != OGC_OK ? rc : run(name, ls);
}

template <typename AT>
int wgrad_moments_impl(const char *name, int b, int cin, int cout, int hw, int relu, const AT *y_prev, const float *pa,
                       const float *pb, const AT *grad_y, const float *coef2, const float *inj, int s_shift,
                       float *moments, ogc_stream_t stream, LiveIn ls = LiveIn()) {
    OGC_REQUIRE(b >= 0 && cin >= 1 && cout >= 1 && hw >= 1, "%s: bad shape", name);
    OGC_REQUIRE(y_prev && pa && pb && grad_y && moments, "%s: null pointer", name);
    if ((hw & (sizeof(AT) == 2 ? 31 : 15)) != 0 || (((uintptr_t)y_prev | (uintptr_t)grad_y) & 15) != 0) {
        ogc_set_error("%s: hw=%d must be a multiple of 16 (32 for 16-bit tensors) and the tensors 16-byte aligned", name, hw);
        return OGC_ERR_UNSUPPORTED;
    }
    if (sizeof(AT) == 2 && !ogc_g_matmul_bf16) {
        ogc_set_error("%s: 16-bit activations need ogc_set_matmul_precision(1)", name);
        return OGC_ERR_UNSUPPORTED;
    }
    OGC_REQUIRE((long long)cin * hw < (1ll << 31) && (long long)cout * hw < (1ll << 31) && b <= 32768,
                "%s: one sample exceeds 32-bit indexing", name);
    if (b == 0) return OGC_OK;
    hipStream_t s = (hipStream_t)stream;
    if (inj) return moments_run<AT, 0, true>(name, b, cin, cout, hw, relu, y_prev, grad_y, pa, pb, coef2, inj, s_shift, moments, s, FirstIn(), ls);
    return moments_run<AT, 0, false>(name, b, cin, cout, hw, relu, y_prev, grad_y, pa, pb, coef2, inj, s_shift, moments, s, FirstIn(), ls);
}

template <typename AT>
int wgrad_moments_pooled_impl(const char *name, int b, int cin, int cout, int hw, int relu, int nsample, const AT *y_prev,
                              const float *pa, const float *pb, const AT *y, const float *coef2, const float *inj,
                              float *moments, ogc_stream_t stream, LiveIn ls = LiveIn()) {
    int sh;
    const int rc = pooled_check(name, b, hw, nsample, coef2, inj, sh);
    if (rc != OGC_OK) return rc;
    return wgrad_moments_impl<AT>(name, b, cin, cout, hw, relu, y_prev, pa, pb, y, coef2, inj, sh, moments, stream, ls);
}
} // namespace

extern "C" int ogc_conv1x1_wgrad_moments(int b, int cin, int cout, int hw, int relu, const float *y_prev, const float *pa,
                                         const float *pb, const float *grad_y, float *moments, ogc_stream_t stream) {
    return wgrad_moments_impl<float>("ogc_conv1x1_wgrad_moments", b, cin, cout, hw, relu, y_prev, pa, pb, grad_y, nullptr, nullptr, 0,
                                     moments, stream);
}

extern "C" int ogc_conv1x1_wgrad_moments_h(int b, int cin, int cout, int hw, int relu, const ogc_bf16_t *y_prev, const float *pa,
                                           const float *pb, const ogc_bf16_t *grad_y, float *moments, ogc_stream_t stream) {
    return wgrad_moments_impl<ogc_bf16>("ogc_conv1x1_wgrad_moments_h", b, cin, cout, hw, relu, y_prev, pa, pb, grad_y, nullptr,
                                        nullptr, 0, moments, stream);
}

// The same with grad_y in the sparse form (pooled_check above); nsample 16, 32 or 64.
extern "C" int ogc_conv1x1_wgrad_moments_pooled(int b, int cin, int cout, int hw, int relu, int nsample, const float *y_prev,
                                                const float *pa, const float *pb, const float *y, const float *coef2,
                                                const float *inj, float *moments, ogc_stream_t stream) {
    return wgrad_moments_pooled_impl<float>("ogc_conv1x1_wgrad_moments_pooled", b, cin, cout, hw, relu, nsample, y_prev, pa, pb, y,
                                            coef2, inj, moments, stream);
}

extern "C" int ogc_conv1x1_wgrad_moments_pooled_live(int b, int cin, int cout, int hw, int relu, int nsample, const float *y_prev,
                                                     const float *pa, const float *pb, const float *y, const float *coef2,
                                                     const float *inj, const int *live, const int *n_live, int live_cap,
                                                     float *moments, ogc_stream_t stream) {
    return with_live("ogc_conv1x1_wgrad_moments_pooled_live", live, n_live, live_cap, hw, nsample, [&](const char *name, const LiveIn &ls) {
        return wgrad_moments_pooled_impl<float>(name, b, cin, cout, hw, relu, nsample, y_prev, pa, pb, y, coef2, inj, moments, stream, ls);
    });
}

extern "C" int ogc_conv1x1_wgrad_moments_pooled_h(int b, int cin, int cout, int hw, int relu, int nsample,
                                                  const ogc_bf16_t *y_prev, const float *pa, const float *pb, const ogc_bf16_t *y,
                                                  const float *coef2, const float *inj, float *moments, ogc_stream_t stream) {
    return wgrad_moments_pooled_impl<ogc_bf16>("ogc_conv1x1_wgrad_moments_pooled_h", b, cin, cout, hw, relu, nsample, y_prev, pa,
                                               pb, y, coef2, inj, moments, stream);
}

extern "C" int ogc_gn_moments_combine(int b, int cin, int cout, int hw, int groups, const float *moments, const float *w,
                                      const float *pa, const float *pb, const float *mean, const float *rstd,
                                      const float *gamma, float *grad_w, float *coef, float *grad_gamma,
                                      float *grad_beta, ogc_stream_t stream) {
    OGC_REQUIRE(b >= 1 && cin >= 1 && cin <= 512 && cout >= 1 && hw >= 1 && groups >= 1 && groups <= 32 && cin % groups == 0,
                "ogc_gn_moments_combine: bad shape (cin <= 512, groups <= 32 dividing cin)");
    OGC_REQUIRE(moments && w && pa && pb && mean && rstd && gamma && grad_w && coef && grad_gamma && grad_beta,
                "ogc_gn_moments_combine: null pointer");
    OGC_REQUIRE(grad_beta == grad_gamma + cin, "ogc_gn_moments_combine: grad_beta must follow grad_gamma (one 2 x cin buffer)");
    if (ogc_zero_async(grad_gamma, sizeof(float) * 2 * (size_t)cin, (hipStream_t)stream) != hipSuccess) {
        ogc_set_error("ogc_gn_moments_combine: memset failed");
        return OGC_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(moments_combine_kernel, dim3(b + ogc_divup((long long)cout * cin, 256)), dim3(256), 0,
                       (hipStream_t)stream, b, cin, cout, hw, groups, moments, w, pa, pb, mean, rstd, gamma, grad_w, coef,
                       grad_gamma, grad_beta);
    OGC_CHECK_LAUNCH("ogc_gn_moments_combine");
    return OGC_OK;
}

namespace {
// One launch of dgrad_adjoint_kernel: KQ by the width of g_y, then the form by what came along — a first convolution (FIRST), a
// live-step list (fp32 only), the sparse gradient (inj).
template <typename AT, int FIRST>
void dgrad_launch(dim3 grid, size_t lds, hipStream_t s, int M, int K, int hw, int relu, const float *w, const AT *gy, const AT *yprev,
                  const float *pa, const float *pb, const float *coef, const float *coef2, const float *inj, int s_shift, AT *out,
                  const FirstIn &first, const LiveIn &ls) {
    constexpr bool BF = sizeof(AT) == 2;
    const float2 *c2 = reinterpret_cast<const float2 *>(coef2), *ij = reinterpret_cast<const float2 *>(inj);
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(WG_WAVES * OGC_WAVE), lds, s, M, K, hw, relu, w, gy, yprev, pa, pb, coef, c2, ij, s_shift,
                           out, first, ls);
    };
    auto form = [&](auto kq) {
        constexpr int KQ = decltype(kq)::value;
        if constexpr (FIRST > 0) { // (list form: the run of tiles derived on the device)
            if (ls.steps) go(dgrad_adjoint_kernel<KQ, false, AT, false, FIRST, true>);
            else go(dgrad_adjoint_kernel<KQ, false, AT, false, FIRST>);
        } else {
            if constexpr (!BF) {
                if (ls.steps) { // (grid of the worst case; workgroups beyond the list leave at once)
                    if (inj) go(dgrad_adjoint_kernel<KQ, true, AT, false, 0, true>);
                    else go(dgrad_adjoint_kernel<KQ, false, AT, false, 0, true>); // (the plain list form: dense output, s_shift bounds the filled steps)
                    return;
                }
            }
            if (inj) go(dgrad_adjoint_kernel<KQ, true, AT, BF>);
            else go(dgrad_adjoint_kernel<KQ, false, AT, BF>);
        }
    };
    const int Kq = (K + 3) / 4;
    if (Kq <= 8) form(TileC<8>());
    else if (Kq <= 16 || FIRST > 0) form(TileC<16>()); // (FIRST: K <= 64, checked by the entry point)
    else if constexpr (FIRST == 0) {
        if (Kq <= 25) form(TileC<25>());
        else if (Kq <= 33) form(TileC<33>());
        else form(TileC<40>());
    }
}

template <typename AT>
int dgrad_adjoint_impl(const char *name, int b, int cin, int cout, int hw, int relu, const float *w, const AT *grad_y,
                       const AT *y_prev, const float *pa, const float *pb, const float *coef, const float *coef2,
                       const float *inj, int s_shift, AT *grad_prev, ogc_stream_t stream, LiveIn ls = LiveIn()) {
    OGC_REQUIRE(b >= 0 && cin >= 1 && cout >= 1 && hw >= 1, "%s: bad shape", name);
    OGC_REQUIRE(w && grad_y && y_prev && pa && pb && coef && grad_prev, "%s: null pointer", name);
    if ((hw & 63) != 0 || cout > 160 || (((uintptr_t)grad_y | (uintptr_t)y_prev | (uintptr_t)grad_prev) & ogc_act_mask<AT>()) != 0) {
        ogc_set_error("%s: needs hw %% 64 == 0, cout <= 160 and 16-byte aligned tensors (hw=%d, cout=%d)", name, hw, cout);
        return OGC_ERR_UNSUPPORTED;
    }
    OGC_REQUIRE((long long)cin * hw < (1ll << 31) && (long long)cout * hw < (1ll << 31) && b <= 65535,
                "%s: one sample exceeds 32-bit indexing", name);
    if (b == 0) return OGC_OK;
    const int M = cin, K = cout, Kq = (K + 3) / 4;
    const size_t lds = ((size_t)64 * ogc_a_ld(Kq) + 64 * 5) * sizeof(float) +
                       (!inj ? 0 : ls.steps ? (size_t)WG_WAVES * K * 5 * sizeof(float2) // (list form: the table's two parts)
                                            : (size_t)WG_WAVES * K * (64 >> s_shift) * sizeof(float4));
    if (sizeof(AT) == 2 && !ogc_g_matmul_bf16) {
        ogc_set_error("%s: 16-bit activations need ogc_set_matmul_precision(1)", name);
        return OGC_ERR_UNSUPPORTED;
    }
    if (lds > 64 * 1024) { // (the kernels keep the default dynamic-LDS limit)
        ogc_set_error("%s: the weight tile and the pooled table need %zu bytes of LDS (> 64 KiB) at cout=%d, nsample=%d", name,
                      lds, cout, 64 >> (6 - s_shift));
        return OGC_ERR_UNSUPPORTED;
    }
    dim3 grid(ogc_divup(hw, 64 * WG_WAVES), b);
    hipStream_t s = (hipStream_t)stream;
    if constexpr (sizeof(AT) == 2) { // dense form, enough tiles: the persistent kernel (the same expressions)
        if (!inj && ogc_gemm16_adjoint_launch(b, M, K, hw, relu, w, grad_y, y_prev, pa, pb, coef, grad_prev, s)) {
            OGC_CHECK_LAUNCH(name);
            return OGC_OK;
        }
    }
    dgrad_launch<AT, 0>(grid, lds, s, M, K, hw, relu, w, grad_y, y_prev, pa, pb, coef, coef2, inj, s_shift, grad_prev, FirstIn(), ls);
    OGC_CHECK_LAUNCH(name);
    return OGC_OK;
}

template <typename AT>
int dgrad_adjoint_pooled_impl(const char *name, int b, int cin, int cout, int hw, int relu, int nsample, const float *w,
                              const AT *y, const float *coef2, const float *inj, const AT *y_prev, const float *pa,
                              const float *pb, const float *coef, AT *grad_prev, ogc_stream_t stream, LiveIn ls = LiveIn()) {
    int sh;
    const int rc = pooled_check(name, b, hw, nsample, coef2, inj, sh);
    if (rc != OGC_OK) return rc;
    return dgrad_adjoint_impl<AT>(name, b, cin, cout, hw, relu, w, y, y_prev, pa, pb, coef, coef2, inj, sh, grad_prev, stream, ls);
}
} // namespace

extern "C" int ogc_conv1x1_dgrad_adjoint(int b, int cin, int cout, int hw, int relu, const float *w, const float *grad_y,
                                         const float *y_prev, const float *pa, const float *pb, const float *coef,
                                         float *grad_prev, ogc_stream_t stream) {
    return dgrad_adjoint_impl<float>("ogc_conv1x1_dgrad_adjoint", b, cin, cout, hw, relu, w, grad_y, y_prev, pa, pb, coef, nullptr,
                                     nullptr, 0, grad_prev, stream);
}

extern "C" int ogc_conv1x1_dgrad_adjoint_h(int b, int cin, int cout, int hw, int relu, const float *w, const ogc_bf16_t *grad_y,
                                           const ogc_bf16_t *y_prev, const float *pa, const float *pb, const float *coef,
                                           ogc_bf16_t *grad_prev, ogc_stream_t stream) {
    return dgrad_adjoint_impl<ogc_bf16>("ogc_conv1x1_dgrad_adjoint_h", b, cin, cout, hw, relu, w, grad_y, y_prev, pa, pb, coef,
                                        nullptr, nullptr, 0, grad_prev, stream);
}

// The same with grad_y in the sparse form (y: the convolution's output).
extern "C" int ogc_conv1x1_dgrad_adjoint_pooled(int b, int cin, int cout, int hw, int relu, int nsample, const float *w,
                                                const float *y, const float *coef2, const float *inj, const float *y_prev,
                                                const float *pa, const float *pb, const float *coef, float *grad_prev,
                                                ogc_stream_t stream) {
    return dgrad_adjoint_pooled_impl<float>("ogc_conv1x1_dgrad_adjoint_pooled", b, cin, cout, hw, relu, nsample, w, y, coef2, inj,
                                            y_prev, pa, pb, coef, grad_prev, stream);
}

extern "C" int ogc_conv1x1_dgrad_adjoint_pooled_live(int b, int cin, int cout, int hw, int relu, int nsample, const float *w,
                                                     const float *y, const float *coef2, const float *inj, const float *y_prev,
                                                     const float *pa, const float *pb, const float *coef, const int *live,
                                                     const int *n_live, int live_cap, float *grad_prev, ogc_stream_t stream) {
    return with_live("ogc_conv1x1_dgrad_adjoint_pooled_live", live, n_live, live_cap, hw, nsample, [&](const char *name, const LiveIn &ls) {
        return dgrad_adjoint_pooled_impl<float>(name, b, cin, cout, hw, relu, nsample, w, y, coef2, inj, y_prev, pa, pb, coef, grad_prev,
                                                stream, ls);
    });
}

extern "C" int ogc_conv1x1_dgrad_adjoint_pooled_h(int b, int cin, int cout, int hw, int relu, int nsample, const float *w,
                                                  const ogc_bf16_t *y, const float *coef2, const float *inj,
                                                  const ogc_bf16_t *y_prev, const float *pa, const float *pb, const float *coef,
                                                  ogc_bf16_t *grad_prev, ogc_stream_t stream) {
    return dgrad_adjoint_pooled_impl<ogc_bf16>("ogc_conv1x1_dgrad_adjoint_pooled_h", b, cin, cout, hw, relu, nsample, w, y, coef2,
                                               inj, y_prev, pa, pb, coef, grad_prev, stream);
}

// ---- the same two kernels behind a first convolution whose output was never stored (first_conv.h) ---------------------------
namespace {
int wgrad_moments_first_impl(const char *name, int b, int cin, int cout, int hw, int relu, int c0, const float *x0, const float *w1,
                             const float *pa, const float *pb, const float *grad_y, float *moments, ogc_stream_t stream,
                             LiveIn ls = LiveIn()) {
    const int rc = ogc_first_check(name, b, cin, c0, hw, x0, w1);
    if (rc != OGC_OK) return rc;
    OGC_REQUIRE(cout >= 1 && pa && pb && grad_y && moments, "%s: bad shape or null pointer", name);
    if (((uintptr_t)grad_y & 15) != 0) {
        ogc_set_error("%s: grad_y must be 16-byte aligned", name);
        return OGC_ERR_UNSUPPORTED;
    }
    OGC_REQUIRE((long long)cout * hw < (1ll << 31), "%s: one sample exceeds 32-bit indexing", name);
    if (b == 0) return OGC_OK;
    hipStream_t s = (hipStream_t)stream;
    FirstIn first;
    first.x0 = x0; first.w1 = w1; first.c0 = c0;
    const int cp = ogc_first_cp(c0);
    const float *none = nullptr;
    if (cp == 3) return moments_run<float, 3, false>(name, b, cin, cout, hw, relu, none, grad_y, pa, pb, none, none, 0, moments, s, first, ls);
    if (cp == 6) return moments_run<float, 6, false>(name, b, cin, cout, hw, relu, none, grad_y, pa, pb, none, none, 0, moments, s, first, ls);
    return moments_run<float, 8, false>(name, b, cin, cout, hw, relu, none, grad_y, pa, pb, none, none, 0, moments, s, first, ls);
}

int dgrad_adjoint_first_impl(const char *name, int b, int cin, int cout, int hw, int relu, int c0, const float *w,
                             const float *grad_y, const float *x0, const float *w1, const float *pa, const float *pb,
                             const float *coef, float *grad_w1, ogc_stream_t stream, LiveIn ls = LiveIn()) {
    const int rc = ogc_first_check(name, b, cin, c0, hw, x0, w1);
    if (rc != OGC_OK) return rc;
    OGC_REQUIRE(cout >= 1 && w && grad_y && pa && pb && coef && grad_w1, "%s: bad shape or null pointer", name);
    if (cout > 64 || ((uintptr_t)grad_y & 15) != 0) {
        ogc_set_error("%s: needs cout <= 64 and a 16-byte aligned grad_y (cout=%d)", name, cout);
        return OGC_ERR_UNSUPPORTED;
    }
    OGC_REQUIRE((long long)cout * hw < (1ll << 31) && b <= 65535, "%s: one sample exceeds 32-bit indexing", name);
    hipStream_t s = (hipStream_t)stream;
    if (ogc_zero_async(grad_w1, sizeof(float) * (size_t)cin * c0, s) != hipSuccess) {
        ogc_set_error("%s: memset failed", name);
        return OGC_ERR_LAUNCH;
    }
    if (b == 0) return OGC_OK;
    const int M = cin, K = cout, Kq = (K + 3) / 4;
    const size_t lds = ((size_t)64 * ogc_a_ld(Kq) + 64 * 5) * sizeof(float);
    // ~768 workgroups over the chip (three per CU are resident: one round), each walking a run of consecutive 256-position tiles
    // of one sample: the atomics per element of dW1 stay in the hundreds
    const int tiles = ogc_divup(hw, 64 * WG_WAVES);
    int chunks = 768 / b;
    if (chunks < 1) chunks = 1;
    if (chunks > tiles) chunks = tiles;
    FirstIn first;
    first.x0 = x0; first.w1 = w1; first.c0 = c0; first.dw1 = grad_w1;
    first.run = ogc_divup(tiles, chunks);
    dim3 grid(ogc_divup(tiles, first.run), b); // (list form: the same grid — the worst case, every step live, is as many tiles)
    const int cp = ogc_first_cp(c0);
    const float *none = nullptr;
    if (cp == 3) dgrad_launch<float, 3>(grid, lds, s, M, K, hw, relu, w, grad_y, none, pa, pb, coef, none, none, 0, (float *)nullptr, first, ls);
    else if (cp == 6) dgrad_launch<float, 6>(grid, lds, s, M, K, hw, relu, w, grad_y, none, pa, pb, coef, none, none, 0, (float *)nullptr, first, ls);
    else dgrad_launch<float, 8>(grid, lds, s, M, K, hw, relu, w, grad_y, none, pa, pb, coef, none, none, 0, (float *)nullptr, first, ls);
    OGC_CHECK_LAUNCH(name);
    return OGC_OK;
}
} // namespace

extern "C" int ogc_conv1x1_wgrad_moments_first(int b, int cin, int cout, int hw, int relu, int c0, const float *x0, const float *w1,
                                               const float *pa, const float *pb, const float *grad_y, float *moments,
                                               ogc_stream_t stream) {
    return wgrad_moments_first_impl("ogc_conv1x1_wgrad_moments_first", b, cin, cout, hw, relu, c0, x0, w1, pa, pb, grad_y, moments,
                                    stream);
}

extern "C" int ogc_conv1x1_dgrad_adjoint_first(int b, int cin, int cout, int hw, int relu, int c0, const float *w,
                                               const float *grad_y, const float *x0, const float *w1, const float *pa,
                                               const float *pb, const float *coef, float *grad_w1, ogc_stream_t stream) {
    return dgrad_adjoint_first_impl("ogc_conv1x1_dgrad_adjoint_first", b, cin, cout, hw, relu, c0, w, grad_y, x0, w1, pa, pb, coef,
                                    grad_w1, stream);
}

// The list forms: grad_y needs values at the positions of live steps only (what ogc_conv1x1_dgrad_adjoint_pooled_live writes).
extern "C" int ogc_conv1x1_wgrad_moments_first_live(int b, int cin, int cout, int hw, int relu, int c0, int nsample, const float *x0,
                                                    const float *w1, const float *pa, const float *pb, const float *grad_y,
                                                    const int *live, const int *n_live, int live_cap, float *moments,
                                                    ogc_stream_t stream) {
    return with_live("ogc_conv1x1_wgrad_moments_first_live", live, n_live, live_cap, hw, nsample, [&](const char *name, const LiveIn &ls) {
        return wgrad_moments_first_impl(name, b, cin, cout, hw, relu, c0, x0, w1, pa, pb, grad_y, moments, stream, ls);
    });
}

extern "C" int ogc_conv1x1_dgrad_adjoint_first_live(int b, int cin, int cout, int hw, int relu, int c0, int nsample, const float *w,
                                                    const float *grad_y, const float *x0, const float *w1, const float *pa,
                                                    const float *pb, const float *coef, const int *live, const int *n_live,
                                                    int live_cap, float *grad_w1, ogc_stream_t stream) {
    return with_live("ogc_conv1x1_dgrad_adjoint_first_live", live, n_live, live_cap, hw, nsample, [&](const char *name, const LiveIn &ls) {
        return dgrad_adjoint_first_impl(name, b, cin, cout, hw, relu, c0, w, grad_y, x0, w1, pa, pb, coef, grad_w1, stream, ls);
    });
}

// The plain list forms — a middle layer between a pooled tail in list form and a layer that reads its gradient densely: grad_y and
// y_prev are read at the positions of live steps only, and ogc_conv1x1_dgrad_adjoint_live_fill writes grad_prev densely (a skipped
// step repeats the last position of the entry that skips it).
extern "C" int ogc_conv1x1_wgrad_moments_live(int b, int cin, int cout, int hw, int relu, int nsample, const float *y_prev,
                                              const float *pa, const float *pb, const float *grad_y, const int *live,
                                              const int *n_live, int live_cap, float *moments, ogc_stream_t stream) {
    return with_live("ogc_conv1x1_wgrad_moments_live", live, n_live, live_cap, hw, nsample, [&](const char *name, const LiveIn &ls) {
        return wgrad_moments_impl<float>(name, b, cin, cout, hw, relu, y_prev, pa, pb, grad_y, nullptr, nullptr, 0, moments, stream, ls);
    });
}

extern "C" int ogc_conv1x1_dgrad_adjoint_live_fill(int b, int cin, int cout, int hw, int relu, int nsample, const float *w,
                                                   const float *grad_y, const float *y_prev, const float *pa, const float *pb,
                                                   const float *coef, const int *live, const int *n_live, int live_cap,
                                                   float *grad_prev, ogc_stream_t stream) {
    return with_live("ogc_conv1x1_dgrad_adjoint_live_fill", live, n_live, live_cap, hw, nsample, [&](const char *name, const LiveIn &ls) {
        return dgrad_adjoint_impl<float>(name, b, cin, cout, hw, relu, w, grad_y, y_prev, pa, pb, coef, nullptr, nullptr,
                                         nsample_shift(nsample), grad_prev, stream, ls);
    });
}

// conv1x1_shared.h — what the two translation units of the 1x1 convolution kernels share (conv1x1.hip: forward / input-gradient
// GEMMs; conv1x1_wgrad.hip: weight gradients).  Split in round 5 so that the two halves compile side by side.
#pragma once
#include <stdlib.h>

#include "ogc_common.h"
#include "conv_stage.h"

typedef float v4f __attribute__((ext_vector_type(4)));
typedef short v4s __attribute__((ext_vector_type(4)));  // four bf16 MFMA operand values

constexpr int WG_WAVES = 4;

// Operand precision of the convolution kernels (ogc_set_matmul_precision): 0 = fp32 operands on
// v_mfma_f32_16x16x4_f32 (default; results are exact fp32 FMA chains), 1 = operands rounded to bf16 (nearest even) on
// v_mfma_f32_16x16x16_bf16, fp32 accumulation, tensors in memory stay fp32 — what autocast(bfloat16) gives the
// reference's Conv2d layers (BASELINE config "OGC-DR ..., bf16").  Layers of 128 channels and more sit on the fp32
// MFMA roof (157 TFLOP/s); with bf16 operands (2.5 PFLOP/s) they fall back onto the HBM roof.  (Defined in conv1x1.hip.)
extern int ogc_g_matmul_bf16;
#define g_matmul_bf16 ogc_g_matmul_bf16

// ---- the two maps the weight-gradient kernels apply to what they load, over N = 4 or 8 consecutive positions of one row ------------
// The gradient behind a pooled GroupNorm, rebuilt from the convolution's raw output y (ogc_group_norm_maxpool_bwd_sparse):
//     g_y[row, pos] = fmaf(c2, y, c3) + (pos % S == arg ? ag : 0)        (c2, c3) = coef2[b, row], (ag, arg) = jv = inj[b, row, pos / S]
// — the expression of gn_maxpool_bwd_dx_kernel, bit for bit.  jpos: position of v[0] inside its neighbourhood (the N positions
// lie inside one neighbourhood: S >= 16); arg travels as int bits.
template <int N>
__device__ __forceinline__ void ogc_pooled_grad(float (&v)[N], float c2, float c3, const float2 &jv, int jpos) {
    const int rel = __float_as_int(jv.y) - jpos;
    const float ag = jv.x;
#pragma unroll
    for (int e = 0; e < N; ++e) v[e] = fmaf(c2, v[e], c3) + (rel == e ? ag : 0.f);
}
template <int N>
__device__ __forceinline__ void ogc_affine_act(float (&v)[N], float a, float b, int relu) {
#pragma unroll
    for (int e = 0; e < N; ++e) {
        v[e] = fmaf(a, v[e], b);
        if (relu) v[e] = fmaxf(v[e], 0.f);
    }
}
// The same two on a float4 = four consecutive positions.  Spelled on the components: through a float[4] (and with the ReLU
// as a second loop) the array forms moved the register allocation of 55 of the 134 weight-gradient kernels.
__device__ __forceinline__ void ogc_pooled_grad(float4 &v, float c2, float c3, const float2 &jv, int jpos) {
    const int rel = __float_as_int(jv.y) - jpos;
    const float ag = jv.x;
    v.x = fmaf(c2, v.x, c3) + (rel == 0 ? ag : 0.f);
    v.y = fmaf(c2, v.y, c3) + (rel == 1 ? ag : 0.f);
    v.z = fmaf(c2, v.z, c3) + (rel == 2 ? ag : 0.f);
    v.w = fmaf(c2, v.w, c3) + (rel == 3 ? ag : 0.f);
}
__device__ __forceinline__ void ogc_affine_act(float4 &v, float a, float b, int relu) {
    v.x = fmaf(a, v.x, b); v.y = fmaf(a, v.y, b);
    v.z = fmaf(a, v.z, b); v.w = fmaf(a, v.w, b);
    if (relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
}

// The GroupNorm adjoint on four consecutive positions of one row (gn_fused_bwd.hip): g, the input gradient W^T g_y, becomes
//     alpha mask g + c2 y + c3,      mask = [fa y + fb > 0] (relu) or all ones
// — the epilogue of dgrad_adjoint_kernel and of the adjoint form of conv1x1_gemm16_kernel (conv1x1_h.hip), which have to agree
// bit for bit: the 16-bit entry point sends a shape to either.
__device__ __forceinline__ void ogc_gn_adjoint(float4 &g, const float4 &y, float fa, float fb, float al, float c2, float c3, int relu) {
    if (relu) {
        g.x = fmaf(fa, y.x, fb) > 0.f ? g.x : 0.f; g.y = fmaf(fa, y.y, fb) > 0.f ? g.y : 0.f;
        g.z = fmaf(fa, y.z, fb) > 0.f ? g.z : 0.f; g.w = fmaf(fa, y.w, fb) > 0.f ? g.w : 0.f;
    }
    g.x = fmaf(al, g.x, fmaf(c2, y.x, c3)); g.y = fmaf(al, g.y, fmaf(c2, y.y, c3));
    g.z = fmaf(al, g.z, fmaf(c2, y.z, c3)); g.w = fmaf(al, g.w, fmaf(c2, y.w, c3));
}

__device__ __forceinline__ v4s ogc_pack_bf16(float a, float b, float c, float d) {
    typedef float v2f __attribute__((ext_vector_type(2)));
    typedef __bf16 v2bf __attribute__((ext_vector_type(2)));
    union { v2bf h[2]; v4s s; } u;
    u.h[0] = __builtin_convertvector((v2f){a, b}, v2bf); // one v_cvt_pk_bf16_f32 per pair
    u.h[1] = __builtin_convertvector((v2f){c, d}, v2bf);
    return u.s;
}

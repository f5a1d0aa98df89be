// first_conv.h — the first convolution of a set-abstraction MLP recomputed where its output would have been loaded.
//
// The first level's MLP starts with a c0 -> c1 convolution of the grouped input x0 (c0 <= 8 channels: coordinates and point
// features).  Its output y1 (c1 channels on every (centre, neighbour) pair) costs c0 multiply-adds per element to make and a full
// pass over memory every time it is written or read; the kernels that consume it — the next layer's forward GEMM, its moment
// matrices and its adjoint input gradient (conv1x1.hip, gn_fused_bwd.hip) — therefore take x0 and W1 and rebuild the float4 of
// y1 they would have loaded.  The value is ONE multiply followed by fused multiply-adds over the input channels ascending:
// the order in which v_mfma_f32_16x16x4_f32 walks k, so the result equals what ogc_conv1x1_gemm_gnstats stores, bit for bit
// (group_linear_direct_kernel of group_linear.hip relies on the same fact).
// CP: the channel count a kernel is built for (3, 6 or 8; c0 <= CP).  Channels c0 .. CP - 1 are zeros in the lane's x0 values
// and in the staged weights: fmaf(0, 0, v) leaves v as it is.
#pragma once
#include "ogc_common.h"

constexpr int FC_MAX_C0 = 8;   // input channels of a first convolution (the staged weight rows are FC_MAX_C0 floats apart)
constexpr int FC_MAX_ROWS = 64; // output channels c1 the consumers hold in LDS

// what the first-layer forms of the three kernels get besides their own arguments
struct FirstIn {
    const float *x0 = nullptr; // (B, c0, hw)
    const float *w1 = nullptr; // (c1, c0)
    int c0 = 0;
    float *dw1 = nullptr;      // adjoint form: (c1, c0), zeroed by the entry point
    int run = 1;               // adjoint form: consecutive 256-position groups a workgroup walks
};

// the preconditions the first-layer entry points share (conv1x1.hip): c0 <= FC_MAX_C0, c1 <= FC_MAX_ROWS, hw % 64 == 0, alignment
int ogc_first_check(const char *name, int b, int c1, int c0, int hw, const float *x0, const float *w1);

constexpr int ogc_first_cp(int c0) { return c0 <= 3 ? 3 : c0 <= 6 ? 6 : 8; }

// s_w1[r * FC_MAX_C0 + c] = W1[r][c], zeros beyond c1 rows / c0 columns (all FC_MAX_ROWS rows are written)
template <int THREADS>
__device__ __forceinline__ void ogc_first_stage_w1(float *s_w1, const float *__restrict__ w1, int c1, int c0) {
    for (int t = threadIdx.x; t < FC_MAX_ROWS * FC_MAX_C0; t += THREADS) {
        const int r = t / FC_MAX_C0, c = t % FC_MAX_C0;
        s_w1[t] = (r < c1 && c < c0) ? w1[r * c0 + c] : 0.f;
    }
}

template <int CP>
__device__ __forceinline__ void ogc_first_w1_row(float (&w)[CP], const float *s_w1, int row) {
    const float4 lo = *reinterpret_cast<const float4 *>(s_w1 + row * FC_MAX_C0);
    w[0] = lo.x; w[1] = lo.y; w[2] = lo.z;
    if constexpr (CP > 3) {
        const float4 hi = *reinterpret_cast<const float4 *>(s_w1 + row * FC_MAX_C0 + 4);
        w[3] = lo.w; w[4] = hi.x; w[5] = hi.y;
        if constexpr (CP > 6) { w[6] = hi.z; w[7] = hi.w; }
    }
}

// the lane's x0 values at four consecutive positions: xp = &x0[b][0][p].  One load shape for every channel (channels beyond
// c0 re-read the last one and are zeroed by a select; a wave that is not `live` reads position 0 of its sample and gets zeros).
template <int CP>
__device__ __forceinline__ void ogc_first_load_raw(float4 (&x)[CP], const float *__restrict__ xp, int c0, int hw) {
#pragma unroll
    for (int c = 0; c < CP; ++c) x[c] = *reinterpret_cast<const float4 *>(xp + (size_t)min(c, c0 - 1) * hw);
}
template <int CP>
__device__ __forceinline__ void ogc_first_mask(float4 (&x)[CP], int c0, bool live) {
#pragma unroll
    for (int c = 0; c < CP; ++c)
        if (!(live && c < c0)) x[c] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// y1[row, p .. p + 3] from the lane's x0 values and the row of W1
template <int CP>
__device__ __forceinline__ float4 ogc_first_row(const float4 (&x)[CP], const float (&w)[CP]) {
    float4 v = make_float4(w[0] * x[0].x, w[0] * x[0].y, w[0] * x[0].z, w[0] * x[0].w);
#pragma unroll
    for (int c = 1; c < CP; ++c) {
        v.x = fmaf(w[c], x[c].x, v.x); v.y = fmaf(w[c], x[c].y, v.y);
        v.z = fmaf(w[c], x[c].z, v.z); v.w = fmaf(w[c], x[c].w, v.w);
    }
    return v;
}

// norm_dev.h — the pieces batch_norm.hip and group_norm.hip share: both are "statistics, then y = act(a_c x + b_c) [or its max
// over the neighbourhood]; backwards sums of dy' x and dy', then dx = a_c dy' + c2 x + c3" and differ in what a row is and in
// where a_c, b_c, c2, c3 come from.  Everything here has a caller in each file (or several in one); what only one kernel
// needs stays next to it.  The loops are written for a block (chunk over the row, channel, sample) of NORM_THREADS threads.
#pragma once
#include <type_traits>

#include "ogc_common.h"
#include "act_io.h"

constexpr int NORM_THREADS = 256;

// block-wide sum of two doubles; result valid in thread 0
__device__ __forceinline__ void norm_block_sum2(double &a, double &b, double *smem /* [2*NORM_THREADS/64] */) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_down(a, off, 64);
        b += __shfl_down(b, off, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        smem[wave * 2] = a;
        smem[wave * 2 + 1] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = 0.0;
        b = 0.0;
        for (int w = 0; w < NORM_THREADS / 64; ++w) {
            a += smem[w * 2];
            b += smem[w * 2 + 1];
        }
    }
}

// dy' = dy * [a x + bb > 0]: the gradient behind the ReLU, the gate recomputed from x
__device__ __forceinline__ float norm_relu_gate(float a, float bb, float v, float d) { return fmaf(a, v, bb) > 0.f ? d : 0.f; }
__device__ __forceinline__ void norm_relu_gate(float a, float bb, const float4 &v, float4 &d) {
    d.x = norm_relu_gate(a, bb, v.x, d.x); d.y = norm_relu_gate(a, bb, v.y, d.y);
    d.z = norm_relu_gate(a, bb, v.z, d.z); d.w = norm_relu_gate(a, bb, v.w, d.w);
}

// dx = a dy' + c2 x + c3
__device__ __forceinline__ float norm_dx(float a, float c2, float c3, float v, float d) { return fmaf(a, d, fmaf(c2, v, c3)); }
__device__ __forceinline__ float4 norm_dx(float a, float c2, float c3, const float4 &v, const float4 &d) {
    return make_float4(norm_dx(a, c2, c3, v.x, d.x), norm_dx(a, c2, c3, v.y, d.y), norm_dx(a, c2, c3, v.z, d.z),
                       norm_dx(a, c2, c3, v.w, d.w));
}

// py = act(a px + bb) over the block's share of one channel row of hw elements
template <bool RELU>
__device__ __forceinline__ void norm_apply_row(float a, float bb, int hw, const float *__restrict__ px, float *__restrict__ py) {
    if ((hw & 3) == 0 && (((uintptr_t)px | (uintptr_t)py) & 15) == 0) {
        for (int i = (blockIdx.x * NORM_THREADS + threadIdx.x) * 4; i < hw; i += gridDim.x * NORM_THREADS * 4) {
            float4 v = *reinterpret_cast<const float4 *>(px + i);
            v.x = fmaf(a, v.x, bb); v.y = fmaf(a, v.y, bb); v.z = fmaf(a, v.z, bb); v.w = fmaf(a, v.w, bb);
            if (RELU) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
            *reinterpret_cast<float4 *>(py + i) = v;
        }
    } else {
        for (int i = blockIdx.x * NORM_THREADS + threadIdx.x; i < hw; i += gridDim.x * NORM_THREADS) {
            const float v = fmaf(a, px[i], bb);
            py[i] = RELU ? fmaxf(v, 0.f) : v;
        }
    }
}

// s += dy' x, sb += dy' over the block's share of one channel row; AT: float / ogc_bf16 (act_io.h)
template <bool RELU, typename AT>
__device__ __forceinline__ void norm_bwd_sums_row(float a, float bb, int hw, const AT *__restrict__ px, const AT *__restrict__ pd,
                                                  double &s, double &sb) {
    if ((hw & 3) == 0 && (((uintptr_t)px | (uintptr_t)pd) & ogc_act_mask<AT>()) == 0) {
        for (int i = (blockIdx.x * NORM_THREADS + threadIdx.x) * 4; i < hw; i += gridDim.x * NORM_THREADS * 4) {
            const float4 v = ogc_ld4(px + i);
            float4 d = ogc_ld4(pd + i);
            if (RELU) norm_relu_gate(a, bb, v, d);
            s += (double)((d.x * v.x + d.y * v.y) + (d.z * v.z + d.w * v.w));
            sb += (double)((d.x + d.y) + (d.z + d.w));
        }
    } else {
        for (int i = blockIdx.x * NORM_THREADS + threadIdx.x; i < hw; i += gridDim.x * NORM_THREADS) {
            const float v = ogc_ld1(px + i);
            float d = ogc_ld1(pd + i);
            if (RELU) d = norm_relu_gate(a, bb, v, d);
            s += (double)d * v;
            sb += d;
        }
    }
}

// x (.., P, S) -> out[base + pr] = max_s act(a x + bb), arg = its position (first index on ties), for the block's share of the
// p rows of one channel (base = its first row).  L = S/4 lanes share a row, one float4 each; the row maximum is reduced with
// xor-shuffles inside the L-lane group.
template <bool RELU>
__device__ __forceinline__ void norm_apply_maxpool_rows(float a, float bb, int p, int s, size_t base, const float *__restrict__ x,
                                                        float *__restrict__ out, int *__restrict__ arg) {
    const int L = s >> 2;                         // lanes per row (power of two, <= 64)
    const int rows_per_block = NORM_THREADS / L;
    const int sub = threadIdx.x % L;
    for (int pr = blockIdx.x * rows_per_block + threadIdx.x / L; pr < p + (rows_per_block - 1);
         pr += gridDim.x * rows_per_block) { // uniform trip count for the shuffles; tail rows are clamped
        const int prc = min(pr, p - 1);
        const float4 v = *reinterpret_cast<const float4 *>(x + (base + prc) * s + sub * 4);
        float y0 = fmaf(a, v.x, bb), y1 = fmaf(a, v.y, bb), y2 = fmaf(a, v.z, bb), y3 = fmaf(a, v.w, bb);
        if (RELU) { y0 = fmaxf(y0, 0.f); y1 = fmaxf(y1, 0.f); y2 = fmaxf(y2, 0.f); y3 = fmaxf(y3, 0.f); }
        float best = y0;
        int bi = sub * 4;
        if (y1 > best) { best = y1; bi = sub * 4 + 1; }
        if (y2 > best) { best = y2; bi = sub * 4 + 2; }
        if (y3 > best) { best = y3; bi = sub * 4 + 3; }
        for (int off = 1; off < L; off <<= 1) {
            const float ob = __shfl_xor(best, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
        }
        if (sub == 0 && pr < p) {
            out[base + pr] = best;
            arg[base + pr] = bi;
        }
    }
}

// gradient of the pooled output of row i behind the ReLU: zero where the maximum itself was gated
template <bool RELU>
__device__ __forceinline__ float norm_pool_gate(const float *__restrict__ out, const float *__restrict__ gout, size_t i) {
    float g = gout[i];
    if (RELU && !(out[i] > 0.f)) g = 0.f;
    return g;
}

// ds += g' x[arg], db += g' over the block's share of the p rows of one channel: the gradient of the max is non-zero only at
// the arg-max element of each row.  xext (or null): x at arg, kept by the forward pass.
template <bool RELU, typename XT>
__device__ __forceinline__ void norm_maxpool_sums_rows(int p, int s, size_t base, const XT *__restrict__ x,
                                                       const float *__restrict__ out, const int *__restrict__ arg,
                                                       const float *__restrict__ gout, const float *__restrict__ xext, double &ds,
                                                       double &db) {
    for (int pr = blockIdx.x * NORM_THREADS + threadIdx.x; pr < p; pr += gridDim.x * NORM_THREADS) {
        const float g = norm_pool_gate<RELU>(out, gout, base + pr);
        // (the gather costs a 32-byte sector per element: 50 us at C4's widths against 5 when the forward pass kept the values)
        ds += (double)g * (double)(xext ? xext[base + pr] : ogc_ld1(x + (base + pr) * s + arg[base + pr]));
        db += g;
    }
}

// dx = c2 x + c3 everywhere, + a g' at the arg-max element of each row; lanes and rows as in norm_apply_maxpool_rows
template <bool RELU>
__device__ __forceinline__ void norm_maxpool_dx_rows(float a, float c2, float c3, int p, int s, size_t base,
                                                     const float *__restrict__ x, const float *__restrict__ out,
                                                     const int *__restrict__ arg, const float *__restrict__ gout,
                                                     float *__restrict__ dx) {
    const int L = s >> 2;
    const int rows_per_block = NORM_THREADS / L;
    const int sub = threadIdx.x % L;
    for (int pr = blockIdx.x * rows_per_block + threadIdx.x / L; pr < p; pr += gridDim.x * rows_per_block) {
        const size_t off = (base + pr) * s + sub * 4;
        const float4 v = *reinterpret_cast<const float4 *>(x + off);
        const float g = norm_pool_gate<RELU>(out, gout, base + pr);
        const int rel = arg[base + pr] - sub * 4;
        const float ag = a * g;
        float4 o;
        o.x = fmaf(c2, v.x, c3) + (rel == 0 ? ag : 0.f);
        o.y = fmaf(c2, v.y, c3) + (rel == 1 ? ag : 0.f);
        o.z = fmaf(c2, v.z, c3) + (rel == 2 ? ag : 0.f);
        o.w = fmaf(c2, v.w, c3) + (rel == 3 ? ag : 0.f);
        *reinterpret_cast<float4 *>(dx + off) = o;
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
// launch(std::true_type / std::false_type): a kernel's RELU instantiation is chosen here, its argument list is written once
template <typename F>
static inline void norm_relu_dispatch(int relu, F &&launch) {
    if (relu) launch(std::true_type{});
    else launch(std::false_type{});
}

// nsample the pooled kernels take: a power of two, one float4 per lane, a row within one wavefront's reach
static inline bool norm_pool_shape_ok(int s) { return s >= 4 && s <= 256 && (s & (s - 1)) == 0; }

// grid.x of the pooled apply / dx kernels: NORM_THREADS / (s/4) rows per workgroup, halved while the grid exceeds 8192 workgroups
// (the kernels stride over the rest)
static inline int norm_pool_blocks(int b, int c, int p, int s) {
    int bx = ogc_divup(p, NORM_THREADS / (s / 4));
    while (bx > 1 && (long long)bx * c * b > 8192) bx = (bx + 1) / 2;
    return bx;
}

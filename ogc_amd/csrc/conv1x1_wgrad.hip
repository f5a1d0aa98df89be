// conv1x1_wgrad.hip — weight gradient of the per-point (1x1) convolutions of the shared MLPs, on the fp32 MFMA pipe.
//
//     dW[co, ci] = sum_b sum_p dY[b, co, p] * X[b, ci, p]          X (B, Cin, HW), dY (B, Cout, HW), fp32, NCHW
//
// Replaces the weight-gradient half of the nn.Conv2d(kernel 1x1, bias=False) layers of SharedMLP
// (reference: utils/nn_util.py:45-85, :155-172).  MIOpen serves this shape with an NHWC implicit-GEMM kernel wrapped
// in two full-tensor NCHW->NHWC transposes (x and dy): on the C4 training step that is ~3 ms of transposes plus ~2 ms
// of igemm per step.  Here the tensors are read once, in place:
//   * GEMM view: M = Cout, N = Cin, K = B*HW (millions) — a tiny output and a huge reduction, i.e. a streaming,
//     HBM-bound kernel; v_mfma_f32_16x16x4_f32 (exact fp32 FMA chains, 157 TF peak) keeps the math off the critical path;
//   * operand layout without any shuffle: for a step of 16 positions, lane (i = l & 15, k = l >> 4) loads ONE float4
//     = row (c0 + i), positions pb + 4k .. 4k+3.  MFMA k-slot k of sub-step s is position pb + 4k + s for BOTH
//     operands, so component s of the two float4s are directly the A and B operands of sub-step s;
//   * a wave owns a (16*COB) x (16*CIB) tile of dW in registers and strides over the positions; the next step's
//     loads are issued before the current step's MFMAs; the four waves of a workgroup are reduced through LDS,
//     workgroups through fp32 atomics into dW (zeroed by this entry point).
#include <type_traits>

#include "conv1x1_shared.h"
#include "act_io.h"

namespace {

// PRO: the layer's input was never materialised — x holds the previous layer's raw convolution output and the operand
// is act(pa[b, ci] * x + pb[b, ci]), recomputed while loading (see conv1x1_gemm_kernel; ogc_affine_act).
// POOLED: dy is not stored — `dy` holds y, the convolution's raw output, and the gradient of the pooled GroupNorm behind it is
// rebuilt while y is loaded:  g_y[row, pos] = fmaf(c2, y, c3) + (pos % S == arg ? ag : 0)  with (c2, c3) = coef2[b, row] and
// (ag, arg) = inj[b, row, pos / S] (ogc_group_norm_maxpool_bwd_sparse; a step's 16 positions lie inside one neighbourhood,
// S = 16, 32, 64) — the expression of gn_maxpool_bwd_dx_kernel, bit for bit (ogc_pooled_grad).
// XT / YT: element types of x and dy (float / ogc_bf16: act_io.h).
// A workgroup's share of dW[row][col].  Ordinarily one fp32 atomic per element and workgroup (the workgroups of a tile split the
// positions among them: blockIdx.x); with slab != 0 (the deterministic mode, det.hip) a plain store into slab blockIdx.x of a
// scratch buffer instead — zeros included — and ogc_det_reduce_f32 adds the slabs to dW in blockIdx.x order afterwards.
__device__ __forceinline__ void wgrad_emit(float *__restrict__ dw, long long slab, int row, int col, int cout, int cin, float v) {
    if (row < cout && col < cin) {
        if (slab) dw[(size_t)blockIdx.x * slab + (size_t)row * cin + col] = v;
        else if (v != 0.0f) unsafeAtomicAdd(dw + (size_t)row * cin + col, v);
    }
}

// ---- a step of the register-tile kernels: what differs between 16 and 32 positions ----------------------------------------------
// SHIFT: log2 of the positions per step, of which lane (i, k) holds PER consecutive ones of row i; Raw: those as loaded; ld: the
// load; mfma: one raw step -> PRO / POOLED maps -> MFMA operands -> the tile's MFMAs.
// The members of this struct and of the stage structs below are `inline`, NOT __forceinline__: they are called from the bodies'
// lambdas and have to be inlined with them, in the ordinary inliner's order.  Forced, they were inlined before anything was
// simplified and the bf16 packing (ogc_pack_bf16) and the two maps then cost other registers in 57 of 134 kernels (compare the
// caveat at ogc_pack_bf16_rr, act_io.h).
// 16 positions: a float4 per lane and row, four v_mfma_f32_16x16x4_f32 per accumulator or (BF) one v_mfma_f32_16x16x16_bf16.
template <bool BF>
struct WgradStep16 {
    static constexpr int SHIFT = 4, PER = 4;
    typedef float4 Raw;
    template <typename T>
    static __device__ inline void ld(const T *p, Raw &r) { r = ogc_ld4(p); }
    template <bool PRO, bool POOLED, typename XT, int COB, int CIB, int NP>
    static __device__ inline void mfma(v4f (&acc)[COB][CIB], const Raw (&yraw)[COB], const Raw (&xraw)[CIB],
                                       const float (&fa)[CIB], const float (&fb)[CIB], const float2 (&cc)[NP],
                                       const float2 (&jv)[NP], int jpos, int pro_relu) {
        float4 yv[COB], xv[CIB];
#pragma unroll
        for (int a = 0; a < COB; ++a) {
            yv[a] = yraw[a];
            if constexpr (POOLED) ogc_pooled_grad(yv[a], cc[a].x, cc[a].y, jv[a], jpos);
        }
#pragma unroll
        for (int c = 0; c < CIB; ++c) {
            xv[c] = xraw[c];
            if (PRO) ogc_affine_act(xv[c], fa[c], fb[c], pro_relu);
        }
        if constexpr (BF) {
            // the lane's four consecutive positions are the four k-slots 4k .. 4k+3 of ONE 16x16x16 MFMA
            v4s yb16[COB], xb16[CIB];
#pragma unroll
            for (int a = 0; a < COB; ++a) yb16[a] = ogc_pack_bf16(yv[a].x, yv[a].y, yv[a].z, yv[a].w);
#pragma unroll
            for (int c = 0; c < CIB; ++c) xb16[c] = ogc_pack_bf16(xv[c].x, xv[c].y, xv[c].z, xv[c].w);
#pragma unroll
            for (int a = 0; a < COB; ++a)
#pragma unroll
                for (int c = 0; c < CIB; ++c)
                    acc[a][c] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(yb16[a], xb16[c], acc[a][c], 0, 0, 0);
        } else {
#pragma unroll
            for (int a = 0; a < COB; ++a)
#pragma unroll
                for (int c = 0; c < CIB; ++c) {
                    acc[a][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(yv[a].x, xv[c].x, acc[a][c], 0, 0, 0);
                    acc[a][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(yv[a].y, xv[c].y, acc[a][c], 0, 0, 0);
                    acc[a][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(yv[a].z, xv[c].z, acc[a][c], 0, 0, 0);
                    acc[a][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(yv[a].w, xv[c].w, acc[a][c], 0, 0, 0);
                }
        }
    }
};

// 32 positions, from 16-bit gradients.  With dy stored as bf16 a 16-position step moves half the bytes and is no faster: it
// issues one load per row block — sixteen rows x 32 bytes: the vector memory pipe works per row, not per byte — plus the per-row
// coefficient loads.  Here lane (i, k) loads row i, positions pb + 8 k .. 8 k + 7 (sixteen bytes of a bf16 tensor, two float4 of
// an fp32 x), and a lane's eight positions are the eight k-slots of ONE v_mfma_f32_16x16x32_bf16 (gfx950; bf16 operands only: the
// 16-bit entry points require ogc_set_matmul_precision(1)).
struct Raw8 { uint4 a, b; }; // eight positions as loaded: bf16 -> a; fp32 -> a, b
template <typename T>
__device__ __forceinline__ void ogc_widen8(const Raw8 &r, float (&f)[8]) {
    if constexpr (sizeof(T) == 2) {
        ogc_unpack8(r.a, f);
    } else {
        f[0] = __uint_as_float(r.a.x); f[1] = __uint_as_float(r.a.y); f[2] = __uint_as_float(r.a.z); f[3] = __uint_as_float(r.a.w);
        f[4] = __uint_as_float(r.b.x); f[5] = __uint_as_float(r.b.y); f[6] = __uint_as_float(r.b.z); f[7] = __uint_as_float(r.b.w);
    }
}
struct WgradStep32 {
    static constexpr int SHIFT = 5, PER = 8;
    typedef Raw8 Raw;
    static __device__ inline void ld(const ogc_bf16 *p, Raw &r) { r.a = *reinterpret_cast<const uint4 *>(p); }
    static __device__ inline void ld(const float *p, Raw &r) {
        r.a = *reinterpret_cast<const uint4 *>(p);
        r.b = *reinterpret_cast<const uint4 *>(p + 4);
    }
    template <bool PRO, bool POOLED, typename XT, int COB, int CIB, int NP>
    static __device__ inline void mfma(v4f (&acc)[COB][CIB], const Raw (&yraw)[COB], const Raw (&xraw)[CIB],
                                       const float (&fa)[CIB], const float (&fb)[CIB], const float2 (&cc)[NP],
                                       const float2 (&jv)[NP], int jpos, int pro_relu) {
        v4s y0[COB], y1[COB], x0[CIB], x1[CIB];
#pragma unroll
        for (int a = 0; a < COB; ++a) {
            if constexpr (POOLED) {
                float f[8];
                ogc_unpack8(yraw[a].a, f);
                ogc_pooled_grad(f, cc[a].x, cc[a].y, jv[a], jpos);
                y0[a] = ogc_pack_bf16_rr(f[0], f[1], f[2], f[3]);
                y1[a] = ogc_pack_bf16_rr(f[4], f[5], f[6], f[7]);
            } else { // dense gradient: the stored bits are the operand
                y0[a] = __builtin_bit_cast(v4s, make_uint2(yraw[a].a.x, yraw[a].a.y));
                y1[a] = __builtin_bit_cast(v4s, make_uint2(yraw[a].a.z, yraw[a].a.w));
            }
        }
#pragma unroll
        for (int c = 0; c < CIB; ++c) {
            if constexpr (!PRO && sizeof(XT) == 2) {
                x0[c] = __builtin_bit_cast(v4s, make_uint2(xraw[c].a.x, xraw[c].a.y));
                x1[c] = __builtin_bit_cast(v4s, make_uint2(xraw[c].a.z, xraw[c].a.w));
            } else {
                float f[8];
                ogc_widen8<XT>(xraw[c], f);
                if (PRO) ogc_affine_act(f, fa[c], fb[c], pro_relu);
                x0[c] = ogc_pack_bf16_rr(f[0], f[1], f[2], f[3]);
                x1[c] = ogc_pack_bf16_rr(f[4], f[5], f[6], f[7]);
            }
        }
#pragma unroll
        for (int a = 0; a < COB; ++a)
#pragma unroll
            for (int c = 0; c < CIB; ++c) {
                acc[a][c] = ogc_mfma_bf16_k32(y0[a], y1[a], x0[c], x1[c], acc[a][c]); // v_mfma_f32_16x16x32_bf16 (gfx950)
            }
    }
};

template <int COB, int CIB, bool PRO, bool BF, bool POOLED = false, typename XT = float, typename YT = float>
__global__ __launch_bounds__(WG_WAVES *OGC_WAVE) void conv1x1_wgrad_kernel(int batch, int cin, int cout, int hw,
                                                                           int steps_per_wave,
                                                                           const XT *__restrict__ x,
                                                                           const YT *__restrict__ dy,
                                                                           float *__restrict__ dw,
                                                                           const float *__restrict__ aff_a,
                                                                           const float *__restrict__ aff_b, int pro_relu,
                                                                           const float2 *__restrict__ coef2 = nullptr,
                                                                           const float2 *__restrict__ inj = nullptr,
                                                                           int s_shift = 0, long long slab = 0) {
    typedef WgradStep16<BF> STEP;
#include "wgrad_tile_body.inc"
}

// the register-tile weight gradient from 16-bit gradients: 32 positions per step (WgradStep32)
template <int COB, int CIB, bool PRO, bool POOLED, typename XT>
__global__ __launch_bounds__(WG_WAVES *OGC_WAVE) void conv1x1_wgrad16_kernel(int batch, int cin, int cout, int hw,
                                                                             int steps_per_wave, const XT *__restrict__ x,
                                                                             const ogc_bf16 *__restrict__ dy,
                                                                             float *__restrict__ dw,
                                                                             const float *__restrict__ aff_a,
                                                                             const float *__restrict__ aff_b, int pro_relu,
                                                                             const float2 *__restrict__ coef2,
                                                                             const float2 *__restrict__ inj, int s_shift,
                                                                             long long slab) {
    typedef WgradStep32 STEP;
    typedef ogc_bf16 YT;
#include "wgrad_tile_body.inc"
}

// Deterministic mode: `splits` zeroed slabs of cout x cin floats in the stream's scratch (a workgroup without positions leaves
// its slab alone); nullptr + g_wgrad_det_failed when the scratch cannot be had.  Otherwise dw itself and slab 0.
thread_local bool g_wgrad_det_failed = false;
float *wgrad_det_slabs(float *dw, int splits, int cin, int cout, long long &slab, hipStream_t s) {
    slab = 0;
    if (!ogc_deterministic()) return dw;
    const size_t words = (size_t)splits * cout * cin;
    float *part = static_cast<float *>(ogc_det_scratch(s, words * sizeof(float)));
    if (!part) {
        g_wgrad_det_failed = true;
        return nullptr;
    }
    const size_t blocks = (words + 255) / 256;
    hipLaunchKernelGGL(ogc_zero_kernel, dim3((unsigned)(blocks > 2048 ? 2048 : blocks)), dim3(256), 0, s,
                       reinterpret_cast<uint32_t *>(part), words);
    slab = (long long)cout * cin;
    return part;
}
void wgrad_det_finish(float *dw, const float *part, int splits, long long slab, hipStream_t s) {
    if (slab && ogc_det_reduce_f32(dw, part, splits, slab, 1, s) != hipSuccess) g_wgrad_det_failed = true;
}

// The kernel form of a launch: launch(PRO, POOLED, BF) with the three as std::bool_constant values.  The pooled form comes with
// the previous layer's norm folded in and keeps fp32 operands for fp32 tensors whatever the precision switch says; 16-bit
// tensors are checked to come with bf16 operands (wgrad_impl).
// Only forms an entry point can reach are instantiated.  x fp32 with dy bf16 is ogc_conv1x1_wgrad_xf_h alone, which passes
// neither pa nor inj: the plain form.  POOLED_OK = false: a launcher that is never handed inj (the register tiles other than
// 64 x 32 and 64 x 64: wgrad_impl).
template <typename XT, typename YT, bool POOLED_OK = true, typename LAUNCH>
auto wgrad_form(const float2 *inj, const float *pa, LAUNCH &&launch) {
    constexpr bool F32 = sizeof(XT) == 4 && sizeof(YT) == 4, XF_H = sizeof(XT) == 4 && sizeof(YT) == 2;
    typedef std::true_type Y;
    typedef std::false_type N;
    if constexpr (!XF_H) {
        if constexpr (POOLED_OK) {
            if (inj) return launch(Y{}, Y{}, std::bool_constant<!F32>{});
        }
        if constexpr (F32) {
            if (pa && !g_matmul_bf16) return launch(Y{}, N{}, N{});
        }
        if (pa) return launch(Y{}, N{}, Y{});
    }
    if constexpr (F32) {
        if (!g_matmul_bf16) return launch(N{}, N{}, N{});
    }
    return launch(N{}, N{}, Y{});
}

template <int COB, int CIB, typename XT = float, typename YT = float>
void wgrad_launch(int b, int cin, int cout, int hw, const XT *x, const YT *dy, float *dw, const float *pa,
                  const float *pb, int pro_relu, hipStream_t s, const float2 *coef2 = nullptr, const float2 *inj = nullptr,
                  int s_shift = 0) {
    constexpr bool Y16 = sizeof(YT) == 2;
    const bool wide = Y16 && (hw & 31) == 0 && (((uintptr_t)x | (uintptr_t)dy) & 15) == 0; // 32-position steps
    const long long nsteps = (long long)b * (wide ? hw >> 5 : hw >> 4);
    const int tiles = ogc_divup(cout, 16 * COB) * ogc_divup(cin, 16 * CIB);
    // ~2048 wavefronts over the chip per tile pair, but at least 8 steps (128 positions) per wave.  The 64x64 tiles
    // (COB = CIB = 4) run best with ~1024 wavefronts in total — one workgroup per CU, twice the positions per
    // wavefront, half as many LDS reductions and atomic epilogues
    // (64 -> 64: 0.169 -> 0.150 ms, 128 -> 128: 0.258 -> 0.222 ms) — unless the tile grid is ragged (131 -> 128: six
    // tiles, two of them nearly empty), where the finer split balances better; the small tiles keep ~2048.
    long long waves = ((COB * CIB == 16 && tiles <= 4) ? 1024 : 2048) / tiles;
    if (waves < 256) waves = 256;
    long long spw = (nsteps + waves - 1) / waves;
    if (spw < 8) spw = 8;
    spw = (spw + 1) / 2 * 2;
    const int wgs = (int)((nsteps + spw * WG_WAVES - 1) / (spw * WG_WAVES));
    dim3 grid(wgs, ogc_divup(cout, 16 * COB), ogc_divup(cin, 16 * CIB));
    long long slab = 0;
    float *const dst = wgrad_det_slabs(dw, wgs, cin, cout, slab, s); // (dw itself unless the deterministic mode is on)
    if (!dst) return;
    constexpr bool POOLED_OK = COB == 4 && (CIB == 2 || CIB == 4); // (the tiles wgrad_impl offers the pooled form with)
    wgrad_form<XT, YT, POOLED_OK>(inj, pa, [&](auto pro, auto pooled, auto bf) {
        constexpr bool PRO = decltype(pro)::value, POOLED = decltype(pooled)::value, BF = decltype(bf)::value;
        if constexpr (Y16) {
            if (wide) {
                hipLaunchKernelGGL((conv1x1_wgrad16_kernel<COB, CIB, PRO, POOLED, XT>), grid, dim3(WG_WAVES * OGC_WAVE), 0, s, b, cin,
                                   cout, hw, (int)spw, x, dy, dst, pa, pb, pro_relu, coef2, inj, s_shift, slab);
                return;
            }
        }
        hipLaunchKernelGGL((conv1x1_wgrad_kernel<COB, CIB, PRO, BF, POOLED, XT, YT>), grid, dim3(WG_WAVES * OGC_WAVE), 0, s, b, cin,
                           cout, hw, (int)spw, x, dy, dst, pa, pb, pro_relu, coef2, inj, s_shift, slab);
    });
    wgrad_det_finish(dw, dst, wgs, slab, s);
}


// ---- the same weight gradient for WIDE layers (cin, cout >= 128): a 128 x 128 tile of dW per workgroup, operands shared through LDS
// conv1x1_wgrad_kernel gives every wavefront a 64 x 64 tile and its own operand loads: at 128 -> 256 channels that is 8 tile
// pairs, every dy element fetched by two of them and every x element by four — 2.1 GB through the L2s for 0.8 GB of tensors, at
// 81 TFLOP/s.  Here the four wavefronts of a workgroup take the four 64 x 64 quarters of one 128 x 128 tile and walk the SAME
// positions: a stage is 32 positions of 128 dy rows and 128 x rows (32 KiB), loaded ONCE by the workgroup (thread t: the 16-byte
// piece t & 7 of rows (t >> 3) + 32 j — full 128-byte lines), transformed once (PRO: the previous layer's GroupNorm + ReLU on x;
// POOLED: the pooled GroupNorm's gradient rebuilt from y, as in the kernel above, bit for bit) and parked in LDS, from where
// every wavefront reads its 64 + 64 rows in the MFMA operand layout of the kernel above (lane (i, k): row i, positions 4k .. 4k + 3).
// Stages are double-buffered: the loads of stage s + 1 are issued before the 128 MFMAs of stage s, their transform and LDS
// write sit between the stage's two 16-position halves, one barrier per stage.  Two workgroups per CU (72 KiB of LDS each), so
// one's barrier is the other's matrix time.  dy is read once per 128 input channels, x once per 128 output channels.
constexpr int WS_POS = 32;              // positions per stage
constexpr int WS_LD = WS_POS + 4;       // row stride in LDS (floats): 144 bytes, 16-byte aligned, rows spread over the banks

// (Measured, 16 x 32768 positions: 128 -> 256 channels 0.480 -> 0.367 ms = 94 TFLOP/s, 256 -> 128 0.439 -> 0.354, 128 -> 128
// 0.195 -> 0.198, with the previous layer's norm folded in 0.226 -> 0.202.  A 256 x 128 tile on eight wavefronts — both tensors
// read from memory exactly once — gave the same 0.367 ms: the kernel is no longer bound by the operand traffic.)
// BF: operands rounded to bf16 on v_mfma_f32_16x16x16_bf16 (ogc_set_matmul_precision), as in conv1x1_wgrad_kernel.
//
// A stage of the shared-tile kernels, what differs between the two: POS positions per stage, rows LD elements (Elem) apart in
// LDS, moved in 16-byte pieces (Piece) of PER positions; ld: a piece from memory; park_y / park_x: the POOLED / PRO map on a
// piece on its way into LDS; half_stage: half a stage's operands from LDS and its MFMAs (yoff / xoff: the lane's rows).
template <bool BF>
struct WgradStage32 {
    static constexpr int POS = WS_POS, LD = WS_LD, PER = 4;
    typedef float Elem;
    typedef float4 Piece;
    template <typename T>
    static __device__ inline Piece ld(const T *p) { return ogc_ld4(p); }
    template <bool POOLED>
    static __device__ inline void park_y(Piece &v, const float2 &cc, const float2 &jv, int jpos) {
        if constexpr (POOLED) ogc_pooled_grad(v, cc.x, cc.y, jv, jpos);
    }
    template <bool PRO>
    static __device__ inline void park_x(Piece &v, float fa, float fb, int pro_relu) {
        if constexpr (PRO) ogc_affine_act(v, fa, fb, pro_relu);
    }
    // 16 positions: 64 MFMAs
    static __device__ inline void half_stage(v4f (&acc)[4][4], const Elem *buf, int yoff, int xoff, int h) {
        float4 yv[4], xv[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) yv[a] = *reinterpret_cast<const float4 *>(buf + yoff + a * 16 * LD + h * 16);
#pragma unroll
        for (int c = 0; c < 4; ++c) xv[c] = *reinterpret_cast<const float4 *>(buf + xoff + c * 16 * LD + h * 16);
        if constexpr (BF) {
            // the lane's four consecutive positions are the four k-slots 4k .. 4k+3 of ONE 16x16x16 MFMA
            v4s yb16[4], xb16[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) yb16[a] = ogc_pack_bf16(yv[a].x, yv[a].y, yv[a].z, yv[a].w);
#pragma unroll
            for (int c = 0; c < 4; ++c) xb16[c] = ogc_pack_bf16(xv[c].x, xv[c].y, xv[c].z, xv[c].w);
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    acc[a][c] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(yb16[a], xb16[c], acc[a][c], 0, 0, 0);
        } else {
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    acc[a][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(yv[a].x, xv[c].x, acc[a][c], 0, 0, 0);
                    acc[a][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(yv[a].y, xv[c].y, acc[a][c], 0, 0, 0);
                    acc[a][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(yv[a].z, xv[c].z, acc[a][c], 0, 0, 0);
                    acc[a][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(yv[a].w, xv[c].w, acc[a][c], 0, 0, 0);
                }
        }
    }
};

// The shared tile for 16-bit tensors.  WgradStage32 with bf16 tensors still moves 8 bytes per lane and load, parks fp32 in LDS
// and lets every wavefront convert what it reads (each value twice): 128 -> 256 pooled at C2 0.71 ms for 1.6 GB.  Here a stage is
// 64 positions: a thread loads SIXTEEN bytes (8 positions of one row; 8 pieces x 32 rows per pass, four passes for the 128 + 128
// rows), transforms once and parks the values as PACKED bf16 (row stride 72 elements = 144 bytes: the 8-byte operand reads of a
// 16-lane row group fall into distinct bank pairs); a wavefront reads its operands ready-made — lane (i, k): row i, positions
// 8 k .. 8 k + 7 of a 32-position half: one v_mfma_f32_16x16x32_bf16 per accumulator and half stage.
constexpr int W16_POS = 64;            // positions per stage
constexpr int W16_LD = W16_POS + 8;    // row stride in LDS (bf16 elements)
struct WgradStage64 {
    static constexpr int POS = W16_POS, LD = W16_LD, PER = 8;
    typedef ogc_bf16 Elem;
    typedef uint4 Piece;
    static __device__ inline Piece ld(const ogc_bf16 *p) { return *reinterpret_cast<const uint4 *>(p); }
    static __device__ inline Piece pack(const float (&f)[8]) {
        const v4s lo = ogc_pack_bf16(f[0], f[1], f[2], f[3]), hi = ogc_pack_bf16(f[4], f[5], f[6], f[7]);
        const uint2 l2 = __builtin_bit_cast(uint2, lo), h2 = __builtin_bit_cast(uint2, hi);
        return make_uint4(l2.x, l2.y, h2.x, h2.y);
    }
    template <bool POOLED>
    static __device__ inline void park_y(Piece &v, const float2 &cc, const float2 &jv, int jpos) {
        if constexpr (POOLED) {
            float f[8];
            ogc_unpack8(v, f);
            ogc_pooled_grad(f, cc.x, cc.y, jv, jpos);
            v = pack(f);
        }
    }
    template <bool PRO>
    static __device__ inline void park_x(Piece &v, float fa, float fb, int pro_relu) {
        if constexpr (PRO) {
            float f[8];
            ogc_unpack8(v, f);
            ogc_affine_act(f, fa, fb, pro_relu);
            v = pack(f);
        }
    }
    // 32 positions: one k32 MFMA per accumulator
    static __device__ inline void half_stage(v4f (&acc)[4][4], const Elem *buf, int yoff, int xoff, int h) {
        uint4 yv[4], xv[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) yv[a] = *reinterpret_cast<const uint4 *>(buf + yoff + a * 16 * LD + h * 32);
#pragma unroll
        for (int c = 0; c < 4; ++c) xv[c] = *reinterpret_cast<const uint4 *>(buf + xoff + c * 16 * LD + h * 32);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int c = 0; c < 4; ++c)
                acc[a][c] = ogc_mfma_bf16_k32(__builtin_bit_cast(v4s, make_uint2(yv[a].x, yv[a].y)),
                                              __builtin_bit_cast(v4s, make_uint2(yv[a].z, yv[a].w)),
                                              __builtin_bit_cast(v4s, make_uint2(xv[c].x, xv[c].y)),
                                              __builtin_bit_cast(v4s, make_uint2(xv[c].z, xv[c].w)), acc[a][c]);
    }
};

template <bool PRO, bool POOLED, bool BF = false, typename XT = float, typename YT = float>
__global__ __launch_bounds__(256, 2) void conv1x1_wgrad_shared_kernel(int batch, int cin, int cout, int hw, int stages_per_wg,
                                                                      const XT *__restrict__ x, const YT *__restrict__ dy,
                                                                      float *__restrict__ dw, const float *__restrict__ aff_a,
                                                                      const float *__restrict__ aff_b, int pro_relu,
                                                                      const float2 *__restrict__ coef2,
                                                                      const float2 *__restrict__ inj, int s_shift, long long slab) {
    extern __shared__ __attribute__((aligned(16))) float ws_lds[]; // [2][256][WS_LD]
    typedef WgradStage32<BF> STAGE;
    float *const lds = ws_lds;
#include "wgrad_shared_body.inc"
}

template <bool PRO, bool POOLED>
__global__ __launch_bounds__(256, 2) void conv1x1_wgrad_shared16_kernel(int batch, int cin, int cout, int hw, int stages_per_wg,
                                                                        const ogc_bf16 *__restrict__ x, const ogc_bf16 *__restrict__ dy,
                                                                        float *__restrict__ dw, const float *__restrict__ aff_a,
                                                                        const float *__restrict__ aff_b, int pro_relu,
                                                                        const float2 *__restrict__ coef2,
                                                                        const float2 *__restrict__ inj, int s_shift, long long slab) {
    extern __shared__ __attribute__((aligned(16))) ogc_bf16 w16_lds[]; // [2][256][W16_LD]
    typedef WgradStage64 STAGE;
    typedef ogc_bf16 XT, YT;
    ogc_bf16 *const lds = w16_lds;
#include "wgrad_shared_body.inc"
}

// the shared-tile kernels' grid: two workgroups per CU over all tiles, at least 8 stages each (spw: stages per workgroup)
dim3 wgrad_shared_grid(int b, int cin, int cout, int hw, int pos, long long &spw) {
    const int tiles = ogc_divup(cout, 128) * ogc_divup(cin, 128);
    const long long nstages = (long long)b * (hw / pos);
    long long wgs = 512 / tiles;
    if (wgs < 1) wgs = 1;
    spw = (nstages + wgs - 1) / wgs;
    if (spw < 8) spw = 8;
    return dim3((unsigned)((nstages + spw - 1) / spw), ogc_divup(cout, 128), ogc_divup(cin, 128));
}

// KERNEL on 256 threads with `lds` bytes of dynamic LDS; the limit on dynamic LDS is raised once per kernel instantiation (one
// `ok` per KERNEL).  false, with the error cleared, when the runtime refused.
template <auto KERNEL, typename... ARGS>
bool wgrad_lds_launch(dim3 grid, size_t lds, hipStream_t s, ARGS... args) {
    static const bool ok = hipFuncSetAttribute(reinterpret_cast<const void *>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)lds) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        return false;
    }
    hipLaunchKernelGGL(KERNEL, grid, dim3(256), lds, s, args...);
    return true;
}

// true when the launch was made (both tensors bf16, hw a multiple of 64, 16-byte aligned)
bool wgrad_shared16_launch(int b, int cin, int cout, int hw, const ogc_bf16 *x, const ogc_bf16 *dy, float *dw, const float *pa,
                           const float *pb, int pro_relu, hipStream_t s, const float2 *coef2, const float2 *inj, int s_shift) {
    static const bool off = [] { const char *e = getenv("OGC_WGRAD_SHARED16"); return e && e[0] == '0'; }();
    if (off || cin < 128 || cout < 128 || (hw % W16_POS) != 0 || (((uintptr_t)x | (uintptr_t)dy) & 15) != 0) return false;
    if (inj && ((1 << s_shift) < 8 || !pa)) return false;
    const size_t lds = sizeof(ogc_bf16) * 2 * 256 * W16_LD;
    long long spw;
    const dim3 grid = wgrad_shared_grid(b, cin, cout, hw, W16_POS, spw);
    long long slab = 0;
    float *const dst = wgrad_det_slabs(dw, grid.x, cin, cout, slab, s);
    if (!dst) return true; // (the failure is reported by wgrad_impl)
    const bool launched = wgrad_form<ogc_bf16, ogc_bf16>(inj, pa, [&](auto pro, auto pooled, auto) {
        return wgrad_lds_launch<conv1x1_wgrad_shared16_kernel<decltype(pro)::value, decltype(pooled)::value>>(
            grid, lds, s, b, cin, cout, hw, (int)spw, x, dy, dst, pa, pb, pro_relu, coef2, inj, s_shift, slab);
    });
    if (launched) wgrad_det_finish(dw, dst, grid.x, slab, s);
    return launched;
}

// OGC_WGRAD_SHARED=0 in the environment: the 64 x 64 register tiles for every width (A/B runs, tests of both kernels)
bool wgrad_shared_enabled() {
    static const bool on = [] { const char *e = getenv("OGC_WGRAD_SHARED"); return !(e && e[0] == '0'); }();
    return on;
}

// true when the launch was made
template <typename XT, typename YT>
bool wgrad_shared_launch(int b, int cin, int cout, int hw, const XT *x, const YT *dy, float *dw, const float *pa,
                         const float *pb, int pro_relu, hipStream_t s, const float2 *coef2, const float2 *inj, int s_shift) {
    if (!wgrad_shared_enabled() || cin < 128 || cout < 128 || (hw % WS_POS) != 0) return false;
    if (inj && ((1 << s_shift) < 4 || !pa)) return false;
    const size_t lds = sizeof(float) * 2 * 256 * WS_LD;
    long long spw;
    const dim3 grid = wgrad_shared_grid(b, cin, cout, hw, WS_POS, spw);
    long long slab = 0;
    float *const dst = wgrad_det_slabs(dw, grid.x, cin, cout, slab, s);
    if (!dst) return true; // (the failure is reported by wgrad_impl)
    const bool launched = wgrad_form<XT, YT>(inj, pa, [&](auto pro, auto pooled, auto bf) {
        return wgrad_lds_launch<conv1x1_wgrad_shared_kernel<decltype(pro)::value, decltype(pooled)::value, decltype(bf)::value, XT, YT>>(
            grid, lds, s, b, cin, cout, hw, (int)spw, x, dy, dst, pa, pb, pro_relu, coef2, inj, s_shift, slab);
    });
    if (launched) wgrad_det_finish(dw, dst, grid.x, slab, s);
    return launched;
}

template <typename XT, typename YT>
int wgrad_impl(const char *name, int b, int cin, int cout, int hw, const XT *x, const YT *dy, float *dw,
               const float *pa, const float *pb, int pro_relu, ogc_stream_t stream, const float2 *coef2 = nullptr,
               const float2 *inj = nullptr, int s_shift = 0) {
    OGC_REQUIRE(b >= 0 && cin >= 1 && cout >= 1 && hw >= 1, "%s: bad shape", name);
    OGC_REQUIRE(x && dy && dw, "%s: null pointer", name);
    if ((hw & 15) != 0 || ((uintptr_t)x & ogc_act_mask<XT>()) != 0 || ((uintptr_t)dy & ogc_act_mask<YT>()) != 0) {
        ogc_set_error("%s: hw=%d must be a multiple of 16 and x/dy 16-byte aligned", name, hw);
        return OGC_ERR_UNSUPPORTED;
    }
    if ((sizeof(XT) == 2 || sizeof(YT) == 2) && !g_matmul_bf16) {
        ogc_set_error("%s: 16-bit activations need ogc_set_matmul_precision(1)", name);
        return OGC_ERR_UNSUPPORTED;
    }
    OGC_REQUIRE((long long)cin * hw < (1ll << 31) && (long long)cout * hw < (1ll << 31),
                "%s: one sample exceeds 32-bit indexing", name);
    hipStream_t s = (hipStream_t)stream;
    if (ogc_zero_async(dw, sizeof(float) * (size_t)cin * cout, s) != hipSuccess) {
        ogc_set_error("%s: memset failed", name);
        return OGC_ERR_LAUNCH;
    }
    if (b == 0) return OGC_OK;
    g_wgrad_det_failed = false;
    struct DetCheck { // (deterministic mode: a launcher that could not get its slabs or its ordered pass says so here)
        const char *name;
        int status() const {
            if (!g_wgrad_det_failed) return OGC_OK;
            ogc_set_error("%s (deterministic): no scratch memory for the partial tiles, or their ordered pass failed", name);
            return OGC_ERR_LAUNCH;
        }
    } det{name};
    // layers of 128 channels and more on both sides: a 128 x 128 tile per workgroup, operands shared through LDS
    if constexpr (sizeof(XT) == 2 && sizeof(YT) == 2) { // both tensors in 16 bits: 64-position stages of packed operands
        if (wgrad_shared16_launch(b, cin, cout, hw, x, dy, dw, pa, pb, pro_relu, s, coef2, inj, s_shift)) {
            OGC_CHECK_LAUNCH(name);
            return det.status();
        }
    }
    if (wgrad_shared_launch(b, cin, cout, hw, x, dy, dw, pa, pb, pro_relu, s, coef2, inj, s_shift)) {
        OGC_CHECK_LAUNCH(name);
        return det.status();
    }
    // register tile per wave: (16*COB) x (16*CIB) outputs.  Small channel counts use small tiles so that no MFMA
    // work is spent on padding; wide layers use 64x64 tiles (16 accumulators) and split the rest over the grid.
    if (inj) { // (the pooled form is offered for the wide tails only: 64-row tiles)
        if (cin <= 32) wgrad_launch<4, 2, XT, YT>(b, cin, cout, hw, x, dy, dw, pa, pb, pro_relu, s, coef2, inj, s_shift);
        else wgrad_launch<4, 4, XT, YT>(b, cin, cout, hw, x, dy, dw, pa, pb, pro_relu, s, coef2, inj, s_shift);
        OGC_CHECK_LAUNCH(name);
        return det.status();
    }
    if (cout <= 16 && cin <= 16) wgrad_launch<1, 1, XT, YT>(b, cin, cout, hw, x, dy, dw, pa, pb, pro_relu, s);
    else if (cout <= 32 && cin <= 16) wgrad_launch<2, 1, XT, YT>(b, cin, cout, hw, x, dy, dw, pa, pb, pro_relu, s);
    else if (cout <= 32 && cin <= 32) wgrad_launch<2, 2, XT, YT>(b, cin, cout, hw, x, dy, dw, pa, pb, pro_relu, s);
    else if (cin <= 16) wgrad_launch<4, 1, XT, YT>(b, cin, cout, hw, x, dy, dw, pa, pb, pro_relu, s);
    else if (cin <= 32) wgrad_launch<4, 2, XT, YT>(b, cin, cout, hw, x, dy, dw, pa, pb, pro_relu, s);
    else if (cout <= 32) wgrad_launch<2, 4, XT, YT>(b, cin, cout, hw, x, dy, dw, pa, pb, pro_relu, s);
    else wgrad_launch<4, 4, XT, YT>(b, cin, cout, hw, x, dy, dw, pa, pb, pro_relu, s);
    OGC_CHECK_LAUNCH(name);
    return det.status();
}
} // namespace

extern "C" int ogc_conv1x1_wgrad(int b, int cin, int cout, int hw, const float *x, const float *dy, float *dw,
                                 ogc_stream_t stream) {
    return wgrad_impl("ogc_conv1x1_wgrad", b, cin, cout, hw, x, dy, dw, nullptr, nullptr, 0, stream);
}

// 16-bit forms (act_io.h; bf16 operands: need ogc_set_matmul_precision(1)).  _xf: x fp32, dy bf16 (the three coordinate columns of
// a grouped first layer: x = the relative coordinates); _h: both bf16.
extern "C" int ogc_conv1x1_wgrad_xf_h(int b, int cin, int cout, int hw, const float *x, const ogc_bf16_t *dy, float *dw,
                                      ogc_stream_t stream) {
    return wgrad_impl<float, ogc_bf16>("ogc_conv1x1_wgrad_xf_h", b, cin, cout, hw, x, dy, dw, nullptr, nullptr, 0, stream);
}

extern "C" int ogc_conv1x1_wgrad_affine(int b, int cin, int cout, int hw, int relu, const float *x, const float *pa,
                                        const float *pb, const float *dy, float *dw, ogc_stream_t stream) {
    OGC_REQUIRE(pa && pb, "ogc_conv1x1_wgrad_affine: null pointer");
    return wgrad_impl("ogc_conv1x1_wgrad_affine", b, cin, cout, hw, x, dy, dw, pa, pb, relu, stream);
}

extern "C" int ogc_conv1x1_wgrad_affine_h(int b, int cin, int cout, int hw, int relu, const ogc_bf16_t *x, const float *pa,
                                          const float *pb, const ogc_bf16_t *dy, float *dw, ogc_stream_t stream) {
    OGC_REQUIRE(pa && pb, "ogc_conv1x1_wgrad_affine_h: null pointer");
    return wgrad_impl<ogc_bf16, ogc_bf16>("ogc_conv1x1_wgrad_affine_h", b, cin, cout, hw, x, dy, dw, pa, pb, relu, stream);
}

// ogc_conv1x1_wgrad_affine with dy in the sparse form of ogc_group_norm_maxpool_bwd_sparse: y is the convolution's raw output
// (b, cout, hw) and g_y is rebuilt from (y, coef2, inj) while y is loaded (see POOLED at conv1x1_wgrad_kernel) — the weight
// gradient of the LAST layer of a set-abstraction MLP without the dense gradient of its pooled GroupNorm.  fp32 operands.
namespace {
template <typename AT>
int wgrad_affine_pooled_impl(const char *name, int b, int cin, int cout, int hw, int relu, int nsample, const AT *x,
                             const float *pa, const float *pb, const AT *y, const float *coef2, const float *inj, float *dw,
                             ogc_stream_t stream) {
    OGC_REQUIRE(pa && pb && coef2 && inj, "%s: null pointer", name);
    const int sh = nsample == 16 ? 4 : nsample == 32 ? 5 : nsample == 64 ? 6 : -1;
    if (sh < 0 || hw % nsample != 0 || (((uintptr_t)coef2 | (uintptr_t)inj) & 7) != 0) {
        ogc_set_error("%s: nsample=%d must be 16, 32 or 64 and divide hw=%d", name, nsample, hw);
        return OGC_ERR_UNSUPPORTED;
    }
    return wgrad_impl<AT, AT>(name, b, cin, cout, hw, x, y, dw, pa, pb, relu, stream, reinterpret_cast<const float2 *>(coef2),
                              reinterpret_cast<const float2 *>(inj), sh);
}
} // namespace

extern "C" int ogc_conv1x1_wgrad_affine_pooled(int b, int cin, int cout, int hw, int relu, int nsample, const float *x,
                                               const float *pa, const float *pb, const float *y, const float *coef2,
                                               const float *inj, float *dw, ogc_stream_t stream) {
    return wgrad_affine_pooled_impl<float>("ogc_conv1x1_wgrad_affine_pooled", b, cin, cout, hw, relu, nsample, x, pa, pb, y, coef2,
                                           inj, dw, stream);
}

extern "C" int ogc_conv1x1_wgrad_affine_pooled_h(int b, int cin, int cout, int hw, int relu, int nsample, const ogc_bf16_t *x,
                                                 const float *pa, const float *pb, const ogc_bf16_t *y, const float *coef2,
                                                 const float *inj, float *dw, ogc_stream_t stream) {
    return wgrad_affine_pooled_impl<ogc_bf16>("ogc_conv1x1_wgrad_affine_pooled_h", b, cin, cout, hw, relu, nsample, x, pa, pb, y,
                                              coef2, inj, dw, stream);
}

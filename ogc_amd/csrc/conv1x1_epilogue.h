// conv1x1_epilogue.h — what the four forward / input-gradient GEMM kernels share: conv1x1_gemm_kernel and conv1x1_gemm_stream_kernel
// (conv1x1.hip: a register tile per wavefront; persistent, fp32, K > 100) and conv1x1_gemm16_kernel and conv1x1_gemm32_kernel
// (conv1x1_h.hip: persistent, 16-bit tensors; persistent, fp32, K <= 64): constants, the pooled epilogue (PoolOut, see "POOL" at
// conv1x1_gemm_kernel) and its one-instruction maxima, and, on the host, the launch of a persistent kernel.
#pragma once
#include "conv1x1_shared.h"

namespace {

constexpr int FW_KQ_MAX = 40; // K <= 160 channels held in registers (40 float4 per lane)
constexpr int GN_SLOTS = 16;  // spread of the fused GroupNorm statistics over cache lines (see ogc_conv1x1_gemm_gnstats)

// max(x, x of the DPP partner) as ONE instruction.  (fmaxf on a DPP-moved value costs three: the move, a canonicalising
// v_max of the moved value — the compiler cannot know it is not a signalling NaN — and the maximum.)  The two wait states a
// DPP read needs after a VALU write of its source are inside the asm: the hazard recogniser does not look into it.
template <int CTRL>
__device__ __forceinline__ float ogc_max_dpp_f32(float x) {
    float r;
    if constexpr (CTRL == 0xB1)
        asm("s_nop 1\n\tv_max_f32_dpp %0, %1, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(x));
    else if constexpr (CTRL == 0x4E)
        asm("s_nop 1\n\tv_max_f32_dpp %0, %1, %1 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(x));
    else if constexpr (CTRL == 0x141)
        asm("s_nop 1\n\tv_max_f32_dpp %0, %1, %1 row_half_mirror row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(x));
    else
        asm("s_nop 1\n\tv_max_f32_dpp %0, %1, %1 row_mirror row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(x));
    return r;
}
__device__ __forceinline__ float ogc_max3_f32(float a, float b, float c) {
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ float ogc_max2_f32(float a, float b) {
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

struct PoolOut {
    float *yext;          // (b, M, centres) largest raw output where sign[m] >= 0, smallest where sign[m] < 0
    int *aext;            // its neighbour index
    const float *sign;    // (M) the scale of the GroupNorm that follows (only its sign is used)
    int s;
};

// The extremes of the neighbourhoods in a wave's 64-row x 64-position tile (see POOL above).  acc[a][c][r]: row a * 16 + kk * 4 + r,
// position p0 + 4 j + c.  SEG = lanes per neighbourhood (4, 8, 16 for 16, 32, 64 neighbours).  sgn: +-1 per row of the tile (LDS).
template <int SEG, typename ACC>
__device__ __forceinline__ void ogc_pool_extremes_epilogue(const ACC (&acc)[4][4], int nblk, const float *sgn, int j, int kk,
                                                           int m0, int M, int centres, int pool_s, float *ye, int *ae) {
    const bool writer = (j & (SEG - 1)) == 0;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        if (a < nblk) {
            const float4 sg4 = *reinterpret_cast<const float4 *>(sgn + a * 16 + kk * 4);
            const float sga[4] = {sg4.x, sg4.y, sg4.z, sg4.w};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + a * 16 + kk * 4 + r;
                const float sg = sga[r]; // exact: +-1 * v
                const float v0 = sg * acc[a][0][r], v1 = sg * acc[a][1][r];
                const float v2 = sg * acc[a][2][r], v3 = sg * acc[a][3][r];
                float hi = ogc_max3_f32(v0, v1, ogc_max2_f32(v2, v3));
                hi = ogc_max_dpp_f32<0xB1>(hi);
                hi = ogc_max_dpp_f32<0x4E>(hi);
                if (SEG >= 8) hi = ogc_max_dpp_f32<0x141>(hi);
                if (SEG >= 16) hi = ogc_max_dpp_f32<0x140>(hi);
                // first position of the neighbourhood that attains it (64: none in this lane) — selects, no branches
                unsigned idx = v3 == hi ? 4u * j + 3u : 64u;
                idx = v2 == hi ? 4u * j + 2u : idx;
                idx = v1 == hi ? 4u * j + 1u : idx;
                idx = v0 == hi ? 4u * j : idx;
                idx = min(idx, ogc_dpp_u32<0xB1>(idx));
                idx = min(idx, ogc_dpp_u32<0x4E>(idx));
                if (SEG >= 8) idx = min(idx, ogc_dpp_u32<0x141>(idx));
                if (SEG >= 16) idx = min(idx, ogc_dpp_u32<0x140>(idx));
                if (writer && m < M) {
                    const int o = (a * 16 + r) * centres;
                    ye[o] = sg * hi;
                    ae[o] = (int)(idx & (unsigned)(pool_s - 1)); // index inside the neighbourhood
                }
            }
        }
    }
}

// ---- host: the launch of a persistent kernel ------------------------------------------------------------------------------------------
// KERNEL with `lds` bytes of dynamic LDS on min(256 per_cu, ntiles / 4) workgroups of four wavefronts (256 CUs).  The limit on
// dynamic LDS is raised to lds_cap once per kernel instantiation (one `raised` per KERNEL); false, with the error cleared, when
// the runtime refuses.
template <auto KERNEL, typename... ARGS>
bool ogc_persistent_launch(size_t lds, int lds_cap, int per_cu, long long ntiles, hipStream_t s, ARGS... args) {
    static bool raised = false;
    if (!raised) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, lds_cap) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        raised = true;
    }
    long long wgs = 256ll * per_cu;
    if (wgs > ntiles / WG_WAVES) wgs = ntiles / WG_WAVES;
    hipLaunchKernelGGL(KERNEL, dim3((unsigned)wgs), dim3(WG_WAVES * OGC_WAVE), lds, s, args...);
    return true;
}

} // namespace

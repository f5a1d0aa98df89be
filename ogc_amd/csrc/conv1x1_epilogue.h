// conv1x1_epilogue.h — what the four forward / input-gradient GEMM kernels share: conv1x1_gemm_kernel and conv1x1_gemm_stream_kernel
// (conv1x1.hip: a register tile per wavefront; persistent, fp32, K > 100) and conv1x1_gemm16_kernel and conv1x1_gemm32_kernel
// (conv1x1_h.hip: persistent, 16-bit tensors; persistent, fp32, K <= 64): constants, the pooled epilogue (PoolOut, see "POOL" at
// conv1x1_gemm_kernel) and its one-instruction maxima, and, on the host, the launch of a persistent kernel.
#pragma once
#include "conv1x1_shared.h"
#include "live_steps.h"

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

// ---- the fp32 partial sums of the GroupNorm statistics (STATS at conv1x1_gemm_kernel) ------------------------------------------------
// One copy for the dense form and the list form of the tile kernel: the list form must reproduce the dense form's 256-value partial
// sums bit for bit (a GroupNorm coefficient one ulp away moves activations across ReLU and max-pool gates).
// A lane's 4 rows x 4 positions, rows outer: c0 .. c3 are its four column-block accumulators of one 16-row block.
template <typename ACC>
__device__ __forceinline__ void ogc_stats_lane_sum(const ACC &c0, const ACC &c1, const ACC &c2, const ACC &c3, float &sm, float &sq) {
    sm = 0.f; sq = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float v0 = c0[r], v1 = c1[r], v2 = c2[r], v3 = c3[r];
        sm += v0; sq += v0 * v0;
        sm += v1; sq += v1 * v1;
        sm += v2; sq += v2 * v2;
        sm += v3; sq += v3 * v3;
    }
}
// the first two stages of the sum over a DPP row stay inside a quad of lanes (16 positions: one step) ...
__device__ __forceinline__ void ogc_stats_quad_sum(float &sm, float &sq) {
    sm += ogc_dpp_f32<0xB1>(sm); sq += ogc_dpp_f32<0xB1>(sq);
    sm += ogc_dpp_f32<0x4E>(sm); sq += ogc_dpp_f32<0x4E>(sq);
}
// ... the last two join the four quads: (Q0 + Q1) + (Q2 + Q3)
__device__ __forceinline__ void ogc_stats_row_sum(float &sm, float &sq) {
    sm += ogc_dpp_f32<0x141>(sm); sq += ogc_dpp_f32<0x141>(sq);
    sm += ogc_dpp_f32<0x140>(sm); sq += ogc_dpp_f32<0x140>(sq);
}

// ---- the list form of the tile kernel (LIST at conv1x1_gemm_kernel; live_steps.h) ---------------------------------------------------
// A wave's tile is four entries of the forward list; slot e = j >> 2 is the quad of lanes that holds entry e.  What a lane knows
// about the tile, from the four entries alone (no data):
struct LiveTile {
    int pos;          // the lane's first position (of its entry's step: 16 * step + 4 * (j & 3)); 0 for a pad
    bool ok;          // the lane's slot holds an entry
    bool tile_lead;   // ... the first entry of its dense 64-position tile (group): this quad forms the group's partial sums
    bool centre_lead; // ... step 0 of its centre: this quad joins the centre's extremes
    int src[4];       // tile_lead: the slot that stands for step s of the group (its own entry, or the centre's last live one)
    bool dead[4];     // tile_lead: ... as a skipped step (16 copies of that entry's last column)
    bool member[4];   // centre_lead: slot t (> e) holds a later step of the same centre
};
__device__ __forceinline__ LiveTile ogc_live_tile(const int *lv, int n_lv, int tile, int hw, int s_shift, int j) {
    LiveTile lt;
    int ent[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) ent[t] = 4 * tile + t < n_lv ? lv[4 * tile + t] : LIVE_PAD;
    const int e = j >> 2;
    const int mine = e == 0 ? ent[0] : e == 1 ? ent[1] : e == 2 ? ent[2] : ent[3];
    const int step = min(mine & LIVE_MASK, (hw >> 4) - 1); // (a list that breaks the rule may give wrong sums, never a wild address)
    const int t_shift = s_shift - 4;                        // steps per centre: 1 << t_shift
    lt.ok = mine >= 0;
    lt.pos = lt.ok ? step * 16 + 4 * (j & 3) : 0;
    lt.centre_lead = lt.ok && (step & ((1 << t_shift) - 1)) == 0;
    lt.tile_lead = lt.ok;
#pragma unroll
    for (int s = 0; s < 4; ++s) { lt.src[s] = e; lt.dead[s] = (step & 3) != s; lt.member[s] = false; }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int st = ent[t] & LIVE_MASK;
        const bool same_tile = lt.ok && ent[t] >= 0 && (st >> 2) == (step >> 2);
        if (t < e && same_tile) lt.tile_lead = false;
        if (t > e && same_tile) {
#pragma unroll
            for (int s = 0; s < 4; ++s)
                if ((st & 3) <= s) { lt.src[s] = t; lt.dead[s] = (st & 3) != s; }
            lt.member[t] = (st >> t_shift) == (step >> t_shift);
        }
    }
    return lt;
}

// LDS of the list form, per wave: [slot][kk][a] float4 (Q sum, Q squares, the same two of a skipped step) | [slot][kk][a][row] float2
// (extreme, its position in the neighbourhood)
constexpr int LIVE_WAVE_FLOATS = 4 * 4 * 4 * 4 + 4 * 4 * 4 * 4 * 2;

// The statistics of the list form: every dense tile's 256-value partial sum, rebuilt from the quads that hold its live steps.
// A skipped step holds 16 copies of the last column of its centre's last live step: each of its lanes would have summed that
// column's four rows four times each (d), and its quad (d + d) + (d + d) — the lane of that column (j & 3 == 3, c = 3) forms it.
// add(a, sum, squares) is called by lane j & 3 == 0 of the quad of each group's first entry.
template <typename ACC, typename ADD>
__device__ __forceinline__ void ogc_live_stats_epilogue(const ACC (&acc)[4][4], int nblk, const LiveTile &lt, float *wl, int j, int kk,
                                                        ADD add) {
    float4 *tab = reinterpret_cast<float4 *>(wl);
    const int e = j >> 2;
    __builtin_amdgcn_wave_barrier(); // (the strip's readers of the previous row tile are done)
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        if (a < nblk) {
            float sm, sq, dm, dq;
            ogc_stats_lane_sum(acc[a][0], acc[a][1], acc[a][2], acc[a][3], sm, sq);
            ogc_stats_quad_sum(sm, sq);
            ogc_stats_lane_sum(acc[a][3], acc[a][3], acc[a][3], acc[a][3], dm, dq);
            dm += dm; dq += dq; // the two quad stages on four equal lanes
            dm += dm; dq += dq;
            if ((j & 3) == 3) tab[(e * 4 + kk) * 4 + a] = make_float4(sm, sq, dm, dq);
        }
    }
    __builtin_amdgcn_wave_barrier();
    if (lt.tile_lead && (j & 3) == 0) {
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            if (a < nblk) {
                float qm[4], qq[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const float4 v = tab[(lt.src[s] * 4 + kk) * 4 + a];
                    qm[s] = lt.dead[s] ? v.z : v.x;
                    qq[s] = lt.dead[s] ? v.w : v.y;
                }
                add(a, (qm[0] + qm[1]) + (qm[2] + qm[3]), (qq[0] + qq[1]) + (qq[2] + qq[3]));
            }
        }
    }
}

// The extremes of the list form: each entry's 16 positions as ogc_pool_extremes_epilogue<4> reduces them, then the entries of
// a centre joined by the quad of its step 0 — the largest value, and the smallest position among the entries that attain it (a
// skipped step only repeats column 0, which lies in step 0).  Lane j & 3 == r keeps and writes row r of each 16-row block.
template <typename ACC>
__device__ __forceinline__ void ogc_live_pool_epilogue(const ACC (&acc)[4][4], int nblk, const LiveTile &lt, float *wl, const float *sgn,
                                                       int j, int kk, int m0, int M, int centres, int pool_s, float *ye, int *ae) {
    float2 *tab = reinterpret_cast<float2 *>(wl + 4 * 4 * 4 * 4);
    const int e = j >> 2, jj = j & 3;
    const unsigned base = (unsigned)(lt.pos & (pool_s - 1)); // of the lane's four positions inside the neighbourhood
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        if (a < nblk) {
            const float4 sg4 = *reinterpret_cast<const float4 *>(sgn + a * 16 + kk * 4);
            const float sga[4] = {sg4.x, sg4.y, sg4.z, sg4.w};
            float keep_hi = 0.f;
            unsigned keep_idx = 64u;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float sg = sga[r]; // exact: +-1 * v
                const float v0 = sg * acc[a][0][r], v1 = sg * acc[a][1][r];
                const float v2 = sg * acc[a][2][r], v3 = sg * acc[a][3][r];
                float hi = ogc_max3_f32(v0, v1, ogc_max2_f32(v2, v3));
                hi = ogc_max_dpp_f32<0xB1>(hi);
                hi = ogc_max_dpp_f32<0x4E>(hi);
                unsigned idx = v3 == hi ? base + 3u : 64u;
                idx = v2 == hi ? base + 2u : idx;
                idx = v1 == hi ? base + 1u : idx;
                idx = v0 == hi ? base : idx;
                idx = min(idx, ogc_dpp_u32<0xB1>(idx));
                idx = min(idx, ogc_dpp_u32<0x4E>(idx));
                keep_hi = jj == r ? hi : keep_hi;
                keep_idx = jj == r ? idx : keep_idx;
            }
            tab[((e * 4 + kk) * 4 + a) * 4 + jj] = make_float2(keep_hi, __uint_as_float(keep_idx));
        }
    }
    __builtin_amdgcn_wave_barrier();
    if (lt.centre_lead) {
        const int centre = lt.pos / pool_s;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int m = m0 + a * 16 + kk * 4 + jj;
            if (a < nblk && m < M) {
                float2 v[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) v[t] = tab[((t * 4 + kk) * 4 + a) * 4 + jj];
                float hi = e == 0 ? v[0].x : e == 1 ? v[1].x : e == 2 ? v[2].x : v[3].x;
#pragma unroll
                for (int t = 1; t < 4; ++t)
                    if (lt.member[t]) hi = ogc_max2_f32(hi, v[t].x);
                unsigned idx = 64u;
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if ((t == e || lt.member[t]) && v[t].x == hi) idx = min(idx, __float_as_uint(v[t].y));
                const size_t o = ((size_t)(a * 16 + jj)) * centres + centre;
                ye[o] = sgn[a * 16 + kk * 4 + jj] * hi;
                ae[o] = (int)(idx & (unsigned)(pool_s - 1));
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

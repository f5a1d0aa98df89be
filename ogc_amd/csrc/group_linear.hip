// group_linear.hip — the first layer of a set-abstraction MLP without the grouped tensor (forward; its gradient is
// ogc_group_linear_bwd of gather_group.hip).  The layer is linear in [x_j - c_i ; f_j], so the
// feature part commutes with the gather:  y[b, m, (i, j)] = P[b, m, idx[b, i, j]] + sum_k wx[m, k] * rel[b, k, (i, j)]
// with P = W_f . f computed per POINT (a small GEMM) and rel = x_j - c_i formed first, exactly as the reference
// does (pointnet2.py:286-288), so nothing cancels.  A thread owns four consecutive positions: one 16-byte index load,
// three 16-byte loads of rel, then per output channel four gathered reads of P (L2-resident: b*m*n floats) and a
// 16-byte store.  A workgroup stays inside one GroupNorm group and adds its (sum, sum of squares) to one of
// GL_SLOTS copies of the (b, groups, 2) fp64 accumulator — the layout ogc_conv1x1_gemm_gnstats fills.
#include "ogc_common.h"
#include "act_io.h"
#include "launch_shape.h"

namespace {
constexpr int GL_SLOTS = 16;

// where this workgroup adds the (sum, sum of squares) of GroupNorm group `group` of sample b: the slot follows blockIdx.x
__device__ __forceinline__ double *gl_stats_slot(double *stats, int b, int groups, int group) {
    return stats + (((size_t)(blockIdx.x % GL_SLOTS) * gridDim.z + b) * groups + group) * 2;
}

// The statistics of the two channel-major kernels: the threads' fp32 (sum, sum of squares) are added up in fp64 over the
// workgroup (wavefront shuffles, then red[2 * GG_THREADS / 64] in LDS) and thread 0 adds the pair to the workgroup's slot.
__device__ __forceinline__ void group_stats_tail(float s, float ss, double *red, double *stats, int b, int groups, int group) {
    double ds = s, dss = ss;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        ds += __shfl_down(ds, off, 64);
        dss += __shfl_down(dss, off, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        red[wave * 2] = ds;
        red[wave * 2 + 1] = dss;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, q = 0.0;
        for (int w = 0; w < GG_THREADS / 64; ++w) {
            a += red[w * 2];
            q += red[w * 2 + 1];
        }
        double *dst = gl_stats_slot(stats, b, groups, group);
        atomicAdd(dst, a);
        atomicAdd(dst + 1, q);
    }
}

// the indices and the relative coordinates of positions t4 .. t4 + 3 of sample b: four 16-byte loads
__device__ __forceinline__ void group_load_positions(const int *__restrict__ idx, const float *__restrict__ rel, int b, int T, int t4,
                                                     int4 &i4, float4 &rx, float4 &ry, float4 &rz) {
    i4 = *reinterpret_cast<const int4 *>(idx + (size_t)b * T + t4);
    const float *rb = rel + (size_t)b * 3 * T + t4;
    rx = *reinterpret_cast<const float4 *>(rb);
    ry = *reinterpret_cast<const float4 *>(rb + T);
    rz = *reinterpret_cast<const float4 *>(rb + 2 * (size_t)T);
}

// OT: element type of y (float / ogc_bf16: act_io.h); the statistics are those of the stored values.
template <typename OT>
__global__ __launch_bounds__(GG_THREADS) void group_linear_fwd_kernel(int m, int n, int T, int cpb, int cg, int groups,
                                                                      const float *__restrict__ P,
                                                                      const int *__restrict__ idx,
                                                                      const float *__restrict__ rel,
                                                                      const float *__restrict__ wx,
                                                                      OT *__restrict__ y,
                                                                      double *__restrict__ stats) {
    __shared__ double red[2 * GG_THREADS / 64];
    const int b = blockIdx.z, c0 = blockIdx.y * cpb;
    const int t4 = (blockIdx.x * GG_THREADS + threadIdx.x) * 4;
    float s = 0.f, ss = 0.f;
    if (t4 < T) {
        int4 i4;
        float4 rx, ry, rz;
        group_load_positions(idx, rel, b, T, t4, i4, rx, ry, rz);
        const float *p = P + ((size_t)b * m + c0) * n;
        OT *o = y + ((size_t)b * m + c0) * T + t4;
        for (int ch = c0; ch < c0 + cpb; ++ch, p += n, o += T) {
            const float w0 = wx[ch * 3], w1 = wx[ch * 3 + 1], w2 = wx[ch * 3 + 2];
            float4 v;
            v.x = fmaf(w2, rz.x, fmaf(w1, ry.x, fmaf(w0, rx.x, p[i4.x])));
            v.y = fmaf(w2, rz.y, fmaf(w1, ry.y, fmaf(w0, rx.y, p[i4.y])));
            v.z = fmaf(w2, rz.z, fmaf(w1, ry.z, fmaf(w0, rx.z, p[i4.z])));
            v.w = fmaf(w2, rz.w, fmaf(w1, ry.w, fmaf(w0, rx.w, p[i4.w])));
#include "group_linear_store.inc"
        }
    }
    if (stats) group_stats_tail(s, ss, red, stats, b, groups, c0 / cg); // uniform
}

// The same layer for FEW feature channels (the first level of an encoder: the features are the coordinates, CF = 3): the reduction
// has 3 + CF terms, so the feature part is applied per POSITION as well — CF gathered feature values instead of one gathered value of
// P per OUTPUT channel (m >= 32 of them), and no point-wise product in front — and every output is ONE fused-multiply-add chain over
// the layer's input channels in their order, [rel x, y, z, f_0 ..] — the order in which the reference's convolution and this library's
// matrix kernels (v_mfma_f32_16x16x4_f32, k ascending) walk cat([grouped_xyz, grouped_features]).  P[idx] + W_xyz rel rounds the two
// halves separately; on the segnet_ogcdr fixture that one bit put an activation of the first level on the other side of its
// ReLU / max-pool gate and moved 68 gradient tensors by 1e-3 (tests/golden_cases.py, gate_flip_tensors.json until round 6).
template <typename OT, int CF>
__global__ __launch_bounds__(GG_THREADS) void group_linear_direct_kernel(int m, int n, int T, int cpb, int cg, int groups,
                                                                         const float *__restrict__ feats, // (b, CF, n)
                                                                         const int *__restrict__ idx,
                                                                         const float *__restrict__ rel,
                                                                         const float *__restrict__ w,     // (m, 3 + CF)
                                                                         OT *__restrict__ y, double *__restrict__ stats) {
    __shared__ double red[2 * GG_THREADS / 64];
    const int b = blockIdx.z, c0 = blockIdx.y * cpb;
    const int t4 = (blockIdx.x * GG_THREADS + threadIdx.x) * 4;
    float s = 0.f, ss = 0.f;
    if (t4 < T) {
        int4 i4;
        float4 rx, ry, rz;
        group_load_positions(idx, rel, b, T, t4, i4, rx, ry, rz);
        float4 f[CF];
#pragma unroll
        for (int c = 0; c < CF; ++c) {
            const float *fp = feats + ((size_t)b * CF + c) * n;
            f[c] = make_float4(fp[i4.x], fp[i4.y], fp[i4.z], fp[i4.w]);
        }
        OT *o = y + ((size_t)b * m + c0) * T + t4;
        for (int ch = c0; ch < c0 + cpb; ++ch, o += T) {
            const float *wr = w + (size_t)ch * (3 + CF);
            float4 v;
            v.x = fmaf(wr[2], rz.x, fmaf(wr[1], ry.x, wr[0] * rx.x));
            v.y = fmaf(wr[2], rz.y, fmaf(wr[1], ry.y, wr[0] * rx.y));
            v.z = fmaf(wr[2], rz.z, fmaf(wr[1], ry.z, wr[0] * rx.z));
            v.w = fmaf(wr[2], rz.w, fmaf(wr[1], ry.w, wr[0] * rx.w));
#pragma unroll
            for (int c = 0; c < CF; ++c) {
                const float wc = wr[3 + c];
                v.x = fmaf(wc, f[c].x, v.x); v.y = fmaf(wc, f[c].y, v.y); v.z = fmaf(wc, f[c].z, v.z); v.w = fmaf(wc, f[c].w, v.w);
            }
#include "group_linear_store.inc"
        }
    }
    if (stats) group_stats_tail(s, ss, red, stats, b, groups, c0 / cg); // uniform
}
} // namespace

namespace {
// What the two channel-major forms share in front of their launch: the preconditions, the channels per workgroup and the zeroed
// statistics.  cf: feature channels of the direct form (src = feats (b, cf, n), w (m, 3 + cf)), GL_OVER_P for the
// form over P (src = P (b, m, n), w = wx).  launch stays false when there is nothing to compute.
constexpr int GL_OVER_P = -1;

struct GroupLinearLaunch {
    bool launch = false;
    int T, cg, cpb;
    dim3 grid;
    double *stats; // nullptr without GroupNorm groups
};

template <typename OT>
int group_linear_prepare(const char *name, int cf, int b, int m, int n, int npoints, int nsample, int groups, const float *src,
                         const int *idx, const float *rel, const float *w, OT *y, double *stats, hipStream_t s, GroupLinearLaunch *l) {
    if (const int rc = group_open(name, b >= 0 && m >= 1 && n >= 1 && groups >= 0, npoints, nsample, &l->T)) return rc;
    if (cf != GL_OVER_P) OGC_REQUIRE(cf >= 1 && cf <= 4, "%s: 1 .. 4 feature channels (got %d)", name, cf);
    const int T = l->T;
    if (b == 0 || T == 0) return OGC_OK;
    OGC_REQUIRE(src && idx && rel && w && y && (stats || groups == 0), "%s: null pointer", name);
    OGC_REQUIRE((long long)m * T < (1ll << 31) && (long long)(cf == GL_OVER_P ? m : cf) * n < (1ll << 31) && b <= 65535,
                "%s: one sample exceeds 32-bit indexing", name);
    if ((T & 3) != 0 || !aligned16(idx) || !aligned16(rel) || ((uintptr_t)y & ogc_act_mask<OT>()) != 0 || (groups > 0 && m % groups != 0)) {
        ogc_set_error("%s: needs npoints * nsample %% 4 == 0, 16-byte aligned tensors, m %% groups == 0", name);
        return OGC_ERR_UNSUPPORTED;
    }
    l->cg = groups > 0 ? m / groups : m;
    l->cpb = 1; // channels per workgroup: the largest power of two <= 16 dividing the group width
    while (l->cpb < 16 && l->cg % (l->cpb * 2) == 0) l->cpb *= 2;
    if (groups > 0 && ogc_zero_async(stats, sizeof(double) * 2 * GL_SLOTS * (size_t)b * groups, s) != hipSuccess) {
        ogc_set_error("%s: memset failed", name);
        return OGC_ERR_LAUNCH;
    }
    l->grid = dim3(ogc_divup(T, GG_THREADS * 4), m / l->cpb, b);
    l->stats = groups > 0 ? stats : nullptr;
    l->launch = true;
    return OGC_OK;
}

template <typename OT>
int group_linear_fwd_direct_impl(int b, int m, int cf, int n, int npoints, int nsample, int groups, const float *feats,
                                 const int *idx, const float *rel, const float *w, OT *y, double *stats, ogc_stream_t stream) {
    GroupLinearLaunch l;
    const int rc = group_linear_prepare("ogc_group_linear_fwd_direct", cf, b, m, n, npoints, nsample, groups, feats, idx, rel, w, y, stats,
                                        (hipStream_t)stream, &l);
    if (rc != OGC_OK || !l.launch) return rc;
#define OGC_GLD(CFV)                                                                                                              \
    hipLaunchKernelGGL((group_linear_direct_kernel<OT, CFV>), l.grid, dim3(GG_THREADS), 0, (hipStream_t)stream, m, n, l.T, l.cpb, l.cg, \
                       groups, feats, idx, rel, w, y, l.stats)
    if (cf == 1) OGC_GLD(1);
    else if (cf == 2) OGC_GLD(2);
    else if (cf == 3) OGC_GLD(3);
    else OGC_GLD(4);
#undef OGC_GLD
    OGC_CHECK_LAUNCH("ogc_group_linear_fwd_direct");
    return OGC_OK;
}

template <typename OT>
int group_linear_fwd_impl(int b, int m, int n, int npoints, int nsample, int groups, const float *P, const int *idx,
                          const float *rel, const float *wx, OT *y, double *stats, ogc_stream_t stream) {
    GroupLinearLaunch l;
    const int rc = group_linear_prepare("ogc_group_linear_fwd", GL_OVER_P, b, m, n, npoints, nsample, groups, P, idx, rel, wx, y, stats,
                                        (hipStream_t)stream, &l);
    if (rc != OGC_OK || !l.launch) return rc;
    hipLaunchKernelGGL(group_linear_fwd_kernel<OT>, l.grid, dim3(GG_THREADS), 0, (hipStream_t)stream, m, n, l.T, l.cpb, l.cg, groups, P,
                       idx, rel, wx, y, l.stats);
    OGC_CHECK_LAUNCH("ogc_group_linear_fwd");
    return OGC_OK;
}
} // namespace

// ogc_group_linear_fwd for 1 .. 4 feature channels without P: y[b, ch, (i, j)] = the fused-multiply-add chain over
// [rel (3), features[:, idx] (cf)] with the layer's weight rows w (m, 3 + cf), input channels ascending.  feats (b, cf, n); the other
// arguments, the statistics layout and the preconditions are ogc_group_linear_fwd's.
extern "C" int ogc_group_linear_fwd_direct(int b, int m, int cf, int n, int npoints, int nsample, int groups, const float *feats,
                                           const int *idx, const float *rel, const float *w, float *y, double *stats,
                                           ogc_stream_t stream) {
    return group_linear_fwd_direct_impl<float>(b, m, cf, n, npoints, nsample, groups, feats, idx, rel, w, y, stats, stream);
}

// 16-bit activations (act_io.h): y stored as bf16, the statistics those of the stored values — 12 gathered bytes per position
// instead of the 4 m bytes of a P row (ogc_group_linear_fwd_pt_h: 256 bytes at m = 64)
extern "C" int ogc_group_linear_fwd_direct_h(int b, int m, int cf, int n, int npoints, int nsample, int groups, const float *feats,
                                             const int *idx, const float *rel, const float *w, ogc_bf16_t *y, double *stats,
                                             ogc_stream_t stream) {
    return group_linear_fwd_direct_impl<ogc_bf16>(b, m, cf, n, npoints, nsample, groups, feats, idx, rel, w,
                                                  reinterpret_cast<ogc_bf16 *>(y), stats, stream);
}

extern "C" int ogc_group_linear_fwd(int b, int m, int n, int npoints, int nsample, int groups, const float *P,
                                    const int *idx, const float *rel, const float *wx, float *y, double *stats,
                                    ogc_stream_t stream) {
    return group_linear_fwd_impl<float>(b, m, n, npoints, nsample, groups, P, idx, rel, wx, y, stats, stream);
}

extern "C" int ogc_group_linear_fwd_h(int b, int m, int n, int npoints, int nsample, int groups, const float *P,
                                      const int *idx, const float *rel, const float *wx, ogc_bf16_t *y, double *stats,
                                      ogc_stream_t stream) {
    return group_linear_fwd_impl<ogc_bf16>(b, m, n, npoints, nsample, groups, P, idx, rel, wx, y, stats, stream);
}

namespace {
// ---- the same layer for 16-bit outputs with P stored POINT-MAJOR ------------------------------------------------------------------
// group_linear_fwd_kernel reads P (b, m, n) with one four-byte gather per output element — 268 M of them for C2's first level, each
// its own cache-line lookup, which is what its 0.32 ms are once the output is written as bf16 (0.54 GB: 1.7 TB/s).  Here P is
// (b, n, m): a position's 64 channels are 256 contiguous bytes, fetched as sixteen 16-byte loads by the ONE lane that owns the
// position (a quarter of the lookups, four channels each).  A lane owns two consecutive positions, so that every channel leaves as
// a 4-byte store and a wavefront writes 256 contiguous bytes per channel; a workgroup handles 64 channels (blockIdx.y picks the
// slice) of GLP_ITERS x 512 positions.  Same expression per element as group_linear_fwd_kernel (fmaf chain over x, y, z on top of
// P), outputs rounded before the statistics: y is bit-identical, the statistics differ in the order of their additions.
// CG: channels per GroupNorm group (16, 32 or 64: compile time, so that the per-group sums index registers).
constexpr int GLP_ITERS = 4;

template <int CG>
__global__ __launch_bounds__(GG_THREADS) void group_linear_fwd_pt_kernel(int m, int n, int T, int groups, int with_stats,
                                                                         const float *__restrict__ Pt,  // (b, n, m)
                                                                         const int *__restrict__ idx,   // (b, T)
                                                                         const float *__restrict__ rel, // (b, 3, T)
                                                                         const float *__restrict__ wx,  // (m, 3)
                                                                         ogc_bf16 *__restrict__ y,      // (b, m, T)
                                                                         double *__restrict__ stats) {
    constexpr int NG = 64 / CG; // groups inside the workgroup's 64 channels
    __shared__ float s_wx[64 * 3];
    __shared__ double red[GG_THREADS / 64][NG][2];
    const int b = blockIdx.z, c0 = blockIdx.y * 64;
    for (int e = threadIdx.x; e < 64 * 3; e += GG_THREADS) s_wx[e] = c0 + e / 3 < m ? wx[(c0 + e / 3) * 3 + e % 3] : 0.f;
    __syncthreads();
    double dgs[NG], dgss[NG]; // per iteration the fp32 partial sums of 2 x CG values move into fp64
#pragma unroll
    for (int g = 0; g < NG; ++g) dgs[g] = dgss[g] = 0.0;
    const int *ib = idx + (size_t)b * T;
    const float *rb = rel + (size_t)b * 3 * T;
    const float *pb_ = Pt + (size_t)b * n * m + c0;
    ogc_bf16 *yb = y + ((size_t)b * m + c0) * T;
    for (int it = 0; it < GLP_ITERS; ++it) {
        const int t2 = ((blockIdx.x * GLP_ITERS + it) * GG_THREADS + threadIdx.x) * 2;
        if (t2 >= T) break;
        const int2 i2 = *reinterpret_cast<const int2 *>(ib + t2);
        const float2 rx = *reinterpret_cast<const float2 *>(rb + t2), ry = *reinterpret_cast<const float2 *>(rb + T + t2),
                     rz = *reinterpret_cast<const float2 *>(rb + 2 * (size_t)T + t2);
        const float4 *p0 = reinterpret_cast<const float4 *>(pb_ + (size_t)i2.x * m);
        const float4 *p1 = reinterpret_cast<const float4 *>(pb_ + (size_t)i2.y * m);
        float gs[NG], gss[NG];
#pragma unroll
        for (int g = 0; g < NG; ++g) gs[g] = gss[g] = 0.f;
        float4 a[16], c[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) a[q] = p0[q];
#pragma unroll
        for (int q = 0; q < 16; ++q) c[q] = p1[q];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const float pa4[4] = {a[q].x, a[q].y, a[q].z, a[q].w}, pc4[4] = {c[q].x, c[q].y, c[q].z, c[q].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int ch = q * 4 + e;
                const float w0 = s_wx[ch * 3], w1 = s_wx[ch * 3 + 1], w2 = s_wx[ch * 3 + 2];
                float v0 = fmaf(w2, rz.x, fmaf(w1, ry.x, fmaf(w0, rx.x, pa4[e])));
                float v1 = fmaf(w2, rz.y, fmaf(w1, ry.y, fmaf(w0, rx.y, pc4[e])));
                v0 = ogc_as_stored<ogc_bf16>(v0);
                v1 = ogc_as_stored<ogc_bf16>(v1);
                if (c0 + ch < m)
                    *reinterpret_cast<unsigned *>(yb + (size_t)ch * T + t2) = (__float_as_uint(v0) >> 16) | (__float_as_uint(v1) & 0xFFFF0000u);
                gs[ch / CG] += v0 + v1;
                gss[ch / CG] += v0 * v0 + v1 * v1;
            }
        }
#pragma unroll
        for (int g = 0; g < NG; ++g) { dgs[g] += (double)gs[g]; dgss[g] += (double)gss[g]; }
    }
    if (with_stats) { // uniform
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            double ds = dgs[g], dss = dgss[g];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                ds += __shfl_down(ds, off, 64);
                dss += __shfl_down(dss, off, 64);
            }
            if (lane == 0) { red[wave][g][0] = ds; red[wave][g][1] = dss; }
        }
        __syncthreads();
        if (threadIdx.x < NG * 2) {
            const int g = threadIdx.x >> 1, which = threadIdx.x & 1;
            double v = 0.0;
            for (int w = 0; w < GG_THREADS / 64; ++w) v += red[w][g][which];
            const int gg = c0 / CG + g;
            if (gg < groups) atomicAdd(gl_stats_slot(stats, b, groups, gg) + which, v);
        }
    }
}
} // namespace

// ogc_group_linear_fwd_h with P stored point-major, Pt (b, n, m) — see group_linear_fwd_pt_kernel.  Needs m % 64 == 0, groups in
// {0} or m / groups in {16, 32, 64}, npoints * nsample % 2 == 0, n * m and m * T below 2^31 (OGC_ERR_UNSUPPORTED otherwise: the
// caller keeps the channel-major form).
extern "C" int ogc_group_linear_fwd_pt_h(int b, int m, int n, int npoints, int nsample, int groups, const float *Pt,
                                         const int *idx, const float *rel, const float *wx, ogc_bf16_t *y, double *stats,
                                         ogc_stream_t stream) {
    int T;
    if (const int rc = group_open("ogc_group_linear_fwd_pt_h", b >= 0 && m >= 1 && n >= 1 && groups >= 0, npoints, nsample, &T)) return rc;
    if (b == 0 || T == 0) return OGC_OK;
    OGC_REQUIRE(Pt && idx && rel && wx && y && (stats || groups == 0), "ogc_group_linear_fwd_pt_h: null pointer");
    const int cg = groups > 0 ? m / groups : 64;
    if ((m & 63) != 0 || (T & 1) != 0 || (groups > 0 && (m % groups != 0 || (cg != 16 && cg != 32 && cg != 64))) ||
        (long long)m * T >= (1ll << 31) || (long long)m * n >= (1ll << 31) || b > 65535 ||
        (((uintptr_t)Pt) & 15) != 0 || (((uintptr_t)idx | (uintptr_t)rel) & 7) != 0 || (((uintptr_t)y) & 3) != 0) {
        ogc_set_error("ogc_group_linear_fwd_pt_h: needs m %% 64 == 0, m / groups in {16, 32, 64}, an even position count and aligned tensors");
        return OGC_ERR_UNSUPPORTED;
    }
    hipStream_t s = (hipStream_t)stream;
    if (groups > 0 && ogc_zero_async(stats, sizeof(double) * 2 * GL_SLOTS * (size_t)b * groups, s) != hipSuccess) {
        ogc_set_error("ogc_group_linear_fwd_pt_h: memset failed");
        return OGC_ERR_LAUNCH;
    }
    dim3 grid(ogc_divup(T, GG_THREADS * 2 * GLP_ITERS), m / 64, b);
#define GLP(CGV) hipLaunchKernelGGL(group_linear_fwd_pt_kernel<CGV>, grid, dim3(GG_THREADS), 0, s, m, n, T, groups, groups > 0 ? 1 : 0, \
                                    Pt, idx, rel, wx, y, stats)
    if (cg == 16) GLP(16);
    else if (cg == 32) GLP(32);
    else GLP(64);
#undef GLP
    OGC_CHECK_LAUNCH("ogc_group_linear_fwd_pt_h");
    return OGC_OK;
}

// gather_group.hip — index gathers and their scatter-add gradients (bandwidth kernels).
//
// Replaces gather_points_kernel_fast / gather_points_grad_kernel_fast
//   (reference: pointnet2/src/sampling_gpu.cu:8-24, :46-63) and
// group_points_kernel_fast / group_points_grad_kernel_fast
//   (reference: pointnet2/src/group_points_gpu.cu:47-66, :8-25).
//
// The reference launches one thread per (channel, output element), so the index tensor is re-read
// once per channel (grid.y = C).  Here a thread owns up to four consecutive output positions, loads
// their indices once (one 16-byte load) and walks the channels, issuing 16-byte stores; a group of
// CH_PER_BLOCK channels per workgroup keeps enough workgroups in flight for small tensors.
//
// group_points is ONE kernel for both ops: gather_points is group_points with nsample = 1.
#include "ogc_common.h"
#include "launch_shape.h"

namespace {

// The gathered rows of channels c0 .. c1 - 1: o[(ch - c0) T + t] = p[(ch - c0) n + id[t]].  VEC4: a thread owns four consecutive
// positions (one 16-byte index load, 16-byte stores), otherwise one.
template <bool VEC4>
__device__ __forceinline__ void gather_rows(int c0, int c1, int n, int T, const int *__restrict__ id, const float *__restrict__ p,
                                            float *__restrict__ o) {
    if (VEC4) {
        const int t4 = (blockIdx.x * GG_THREADS + threadIdx.x) * 4;
        if (t4 >= T) return;
        const int4 i4 = *reinterpret_cast<const int4 *>(id + t4);
        for (int ch = c0; ch < c1; ++ch, p += n, o += T) {
            float4 v;
            v.x = p[i4.x]; v.y = p[i4.y]; v.z = p[i4.z]; v.w = p[i4.w];
            *reinterpret_cast<float4 *>(o + t4) = v;
        }
    } else {
        const int t = blockIdx.x * GG_THREADS + threadIdx.x;
        if (t >= T) return;
        const int i = id[t];
        for (int ch = c0; ch < c1; ++ch, p += n, o += T) o[t] = p[i];
    }
}

// The three relative-coordinate rows of one sample: o[a T + t] = xb[id[t]][a] - qb[t / nsample][a], a in 0..2 — what QueryAndGroup
// puts in front of the grouped features (pointnet2.py:286-288: group, then subtract the centre).  xb (n, 3), qb (npoints, 3).
template <bool VEC4>
__device__ __forceinline__ void rel_rows(int T, int nsample, const int *__restrict__ id, const float *__restrict__ xb,
                                         const float *__restrict__ qb, float *__restrict__ o) {
    if (VEC4) {
        const int t4 = (blockIdx.x * GG_THREADS + threadIdx.x) * 4;
        if (t4 >= T) return;
        const int4 i4 = *reinterpret_cast<const int4 *>(id + t4);
        const int ii[4] = {i4.x, i4.y, i4.z, i4.w};
        float r[3][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float *p = xb + (size_t)ii[j] * 3, *q = qb + (size_t)((t4 + j) / nsample) * 3;
            r[0][j] = __fsub_rn(p[0], q[0]);
            r[1][j] = __fsub_rn(p[1], q[1]);
            r[2][j] = __fsub_rn(p[2], q[2]);
        }
#pragma unroll
        for (int a = 0; a < 3; ++a)
            *reinterpret_cast<float4 *>(o + (size_t)a * T + t4) = make_float4(r[a][0], r[a][1], r[a][2], r[a][3]);
    } else {
        const int t = blockIdx.x * GG_THREADS + threadIdx.x;
        if (t >= T) return;
        const float *p = xb + (size_t)id[t] * 3, *q = qb + (size_t)(t / nsample) * 3;
        o[t] = __fsub_rn(p[0], q[0]);
        o[(size_t)T + t] = __fsub_rn(p[1], q[1]);
        o[2 * (size_t)T + t] = __fsub_rn(p[2], q[2]);
    }
}

// out[b,c,t] = points[b,c,idx[b,t]],  t in [0, T)   (T = npoints*nsample)
template <bool VEC4>
__global__ __launch_bounds__(GG_THREADS) void group_fwd_kernel(int c, int n, int T, int ch_per_block,
                                                               long long out_bstride,
                                                               const float *__restrict__ points,
                                                               const int *__restrict__ idx,
                                                               float *__restrict__ out) {
    const int b = blockIdx.z;
    const int c0 = blockIdx.y * ch_per_block;
    const int c1 = min(c, c0 + ch_per_block);
    const int *id = idx + (size_t)b * T;
    const float *p = points + ((size_t)b * c + c0) * n;
    float *o = out + (size_t)b * out_bstride + (size_t)c0 * T; // out_bstride = c*T for a dense (b,c,T) output
    gather_rows<VEC4>(c0, c1, n, T, id, p, o);
}

// grad_points[b,c,idx[b,t]] += grad_out[b,c,t]
template <bool VEC4>
__global__ __launch_bounds__(GG_THREADS) void group_bwd_kernel(int c, int n, int T, int ch_per_block,
                                                               long long go_bstride,
                                                               const float *__restrict__ grad_out,
                                                               const int *__restrict__ idx,
                                                               float *__restrict__ grad_points) {
    const int b = blockIdx.z;
    const int c0 = blockIdx.y * ch_per_block;
    const int c1 = min(c, c0 + ch_per_block);
    const int *id = idx + (size_t)b * T;
    const float *g = grad_out + (size_t)b * go_bstride + (size_t)c0 * T;
    float *gp = grad_points + ((size_t)b * c + c0) * n;
    if (VEC4) {
        const int t4 = (blockIdx.x * GG_THREADS + threadIdx.x) * 4;
        if (t4 >= T) return;
        const int4 i4 = *reinterpret_cast<const int4 *>(id + t4);
        for (int ch = c0; ch < c1; ++ch, g += T, gp += n) {
            const float4 v = *reinterpret_cast<const float4 *>(g + t4);
            unsafeAtomicAdd(gp + i4.x, v.x);
            unsafeAtomicAdd(gp + i4.y, v.y);
            unsafeAtomicAdd(gp + i4.z, v.z);
            unsafeAtomicAdd(gp + i4.w, v.w);
        }
    } else {
        const int t = blockIdx.x * GG_THREADS + threadIdx.x;
        if (t >= T) return;
        const int i = id[t];
        for (int ch = c0; ch < c1; ++ch, g += T, gp += n) unsafeAtomicAdd(gp + i, g[t]);
    }
}

// LDS-privatised scatter-add: a workgroup owns CC channels x one slice of the T positions of batch b,
// accumulates into an LDS image acc[CC][n] with ds_add_f32 (no global atomic contention: kNN neighbour lists
// overlap heavily, group_points_gpu.cu:24 serialises on popular points), then merges the non-zero entries
// into grad_points with one global atomic each.
// WX: the gradient tensor is also multiplied with the relative coordinates rel (b, 3, T) on the way —
// dwx[ch, k] += sum_t grad_out[b, ch, t] * rel[b, k, t], the xyz columns of the weight gradient of ogc_group_linear_fwd's
// layer — so that the tensor is read once for both results.
template <int CC, bool WX>
__global__ __launch_bounds__(GG_THREADS) void group_bwd_lds_kernel(int c, int n, int T, int t_per_block,
                                                                   long long go_bstride,
                                                                   const float *__restrict__ grad_out,
                                                                   const int *__restrict__ idx,
                                                                   float *__restrict__ grad_points,
                                                                   const float *__restrict__ rel,
                                                                   float *__restrict__ dwx) {
    extern __shared__ __attribute__((aligned(16))) float gb_acc[]; // [CC][n]
    const int b = blockIdx.z;
    const int c0 = blockIdx.y * CC;
    const int ncc = min(CC, c - c0);
    const int t_begin = blockIdx.x * t_per_block;
    const int t_end = min(T, t_begin + t_per_block);
    for (int i = threadIdx.x; i < CC * n; i += GG_THREADS) gb_acc[i] = 0.0f;
    __syncthreads();
    const int *id = idx + (size_t)b * T;
    const float *g = grad_out + (size_t)b * go_bstride + (size_t)c0 * T;
    // A thread owns 16 consecutive positions (64 contiguous bytes per channel) and merges runs of equal indices
    // before touching LDS: neighbour rows end in long runs of the SAME index (kNN rows clamped to the nearest
    // neighbour beyond the radius, ball-query rows padded with the first hit), which would otherwise serialise as
    // same-address atomics.  t_begin, t_per_block and T are multiples of 16 on this path.
    float wacc[WX ? CC : 1][3];
#pragma unroll
    for (int cc = 0; cc < (WX ? CC : 1); ++cc) wacc[cc][0] = wacc[cc][1] = wacc[cc][2] = 0.0f;
    for (int t16 = t_begin + threadIdx.x * 16; t16 < t_end; t16 += GG_THREADS * 16) {
        int ids[16];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int4 i4 = *reinterpret_cast<const int4 *>(id + t16 + 4 * u);
            ids[4 * u] = i4.x; ids[4 * u + 1] = i4.y; ids[4 * u + 2] = i4.z; ids[4 * u + 3] = i4.w;
        }
        float rl[WX ? 3 : 1][16];
        if constexpr (WX) {
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float4 f = *reinterpret_cast<const float4 *>(rel + ((size_t)b * 3 + k) * T + t16 + 4 * u);
                    rl[k][4 * u] = f.x; rl[k][4 * u + 1] = f.y; rl[k][4 * u + 2] = f.z; rl[k][4 * u + 3] = f.w;
                }
        }
#pragma unroll
        for (int cc = 0; cc < CC; ++cc) {
            if (cc < ncc) {
                float v[16];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float4 f = *reinterpret_cast<const float4 *>(g + (size_t)cc * T + t16 + 4 * u);
                    v[4 * u] = f.x; v[4 * u + 1] = f.y; v[4 * u + 2] = f.z; v[4 * u + 3] = f.w;
                }
                if constexpr (WX) {
#pragma unroll
                    for (int k = 0; k < 3; ++k)
#pragma unroll
                        for (int u = 0; u < 16; ++u) wacc[cc][k] = fmaf(v[u], rl[k][u], wacc[cc][k]);
                }
                float *a = gb_acc + cc * n;
                float run = v[0];
#pragma unroll
                for (int u = 1; u < 16; ++u) {
                    if (ids[u] == ids[u - 1]) {
                        run += v[u];
                    } else {
                        atomicAdd(a + ids[u - 1], run);
                        run = v[u];
                    }
                }
                atomicAdd(a + ids[15], run);
            }
        }
    }
    __syncthreads();
    float *gp = grad_points + ((size_t)b * c + c0) * n;
    for (int i = threadIdx.x; i < ncc * n; i += GG_THREADS) {
        const float v = gb_acc[i];
        if (v != 0.0f) unsafeAtomicAdd(gp + i, v);
    }
    if constexpr (WX) { // wavefront sums, then one atomic per (channel, axis) and wavefront
#pragma unroll
        for (int cc = 0; cc < CC; ++cc)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float w = wacc[cc][k];
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) w += __shfl_down(w, off, 64);
                if ((threadIdx.x & 63) == 0 && cc < ncc && w != 0.0f) unsafeAtomicAdd(dwx + (size_t)(c0 + cc) * 3 + k, w);
            }
    }
}

// out[b, ch, p*nsample + s] = xyz[b, idx[b,p,s], ch] - new_xyz[b, p, ch],  ch in 0..2 (rel_rows)
__global__ __launch_bounds__(GG_THREADS) void group_xyz_rel_kernel(int n, int npoints, int nsample,
                                                                   long long out_bstride,
                                                                   const float *__restrict__ xyz,
                                                                   const float *__restrict__ new_xyz,
                                                                   const int *__restrict__ idx,
                                                                   float *__restrict__ out) {
    const int b = blockIdx.y;
    const int T = npoints * nsample;
    rel_rows<false>(T, nsample, idx + (size_t)b * T, xyz + (size_t)b * n * 3, new_xyz + (size_t)b * npoints * 3,
                    out + (size_t)b * out_bstride);
}

// ogc_group_concat in ONE launch: the workgroups of the last y-row write the three relative-coordinate rows (as
// group_xyz_rel_kernel), the others the gathered feature rows behind them (group_fwd_kernel).  At B = 1 (FlowStep3D inference: ~46
// groupers per forward) the two launches of the pair are ~4 us each on a serial timeline.
template <bool VEC4>
__global__ __launch_bounds__(GG_THREADS) void group_concat_kernel(int c, int n, int T, int nsample, int ch_per_block,
                                                                  long long out_bstride, const float *__restrict__ points,
                                                                  const int *__restrict__ idx, const float *__restrict__ xyz,
                                                                  const float *__restrict__ new_xyz, float *__restrict__ out) {
    const int b = blockIdx.z;
    const int *id = idx + (size_t)b * T;
    float *ob = out + (size_t)b * out_bstride;
    if (blockIdx.y == gridDim.y - 1) { // rows 0..2: xyz[idx] - centre
        const int npoints = T / nsample;
        const float *xb = xyz + (size_t)b * n * 3, *qb = new_xyz + (size_t)b * npoints * 3;
        rel_rows<VEC4>(T, nsample, id, xb, qb, ob);
        return;
    }
    const int c0 = blockIdx.y * ch_per_block;
    const int c1 = min(c, c0 + ch_per_block);
    const float *p = points + ((size_t)b * c + c0) * n;
    float *o = ob + (size_t)(3 + c0) * T;
    gather_rows<VEC4>(c0, c1, n, T, id, p, o);
}

// The launch shape of the kernels above and of group_bwd_kernel: the 4-wide form needs a position count, an index tensor, a data
// tensor and a batch stride that all allow 16-byte accesses.  extra_rows: y-rows on top of the channel groups.
struct Vec4Shape {
    bool vec;
    int cpb;
    dim3 grid;
};

Vec4Shape vec4_shape(int b, int c, int T, const int *idx, const float *tensor, long long bstride, int extra_rows = 0) {
    Vec4Shape sh;
    sh.vec = (T % 4 == 0) && aligned16(idx) && aligned16(tensor) && bstride % 4 == 0;
    const int bx = ogc_divup(T, sh.vec ? GG_THREADS * 4 : GG_THREADS);
    sh.cpb = pick_ch_per_block(b, c, bx);
    sh.grid = dim3(bx, ogc_divup(c, sh.cpb) + extra_rows, b);
    return sh;
}

#define GG_LAUNCH_VEC4(KERNEL, SH, STREAM, ...)                                                                       \
    do {                                                                                                              \
        if ((SH).vec)                                                                                                 \
            hipLaunchKernelGGL(KERNEL<true>, (SH).grid, dim3(GG_THREADS), 0, (hipStream_t)(STREAM), __VA_ARGS__);     \
        else                                                                                                          \
            hipLaunchKernelGGL(KERNEL<false>, (SH).grid, dim3(GG_THREADS), 0, (hipStream_t)(STREAM), __VA_ARGS__);    \
    } while (0)

int group_fwd(const char *name, int b, int c, int n, int T, const float *points, const int *idx,
              float *out, ogc_stream_t stream, long long out_bstride = -1) {
    if (out_bstride < 0) out_bstride = (long long)c * T;
    OGC_REQUIRE(b >= 0 && c >= 0 && n >= 0 && T >= 0, "%s: negative dimension", name);
    if (b == 0 || c == 0 || T == 0) return OGC_OK;
    OGC_REQUIRE(points && idx && out, "%s: null pointer", name);
    // the reference indexes the whole tensor with 32-bit ints (group_points_gpu.cu:63); here batch offsets are 64-bit
    OGC_REQUIRE(out_bstride < (1ll << 31) && (long long)c * n < (1ll << 31) && b <= 65535,
                "%s: one sample exceeds 32-bit indexing", name);
    const Vec4Shape sh = vec4_shape(b, c, T, idx, out, out_bstride);
    GG_LAUNCH_VEC4(group_fwd_kernel, sh, stream, c, n, T, sh.cpb, out_bstride, points, idx, out);
    OGC_CHECK_LAUNCH(name);
    return OGC_OK;
}

// deterministic mode: dwx[ch][k] += sum over samples and positions of grad_out[b, ch, t] * rel[b, k, t] — one workgroup per channel,
// thread i takes positions i, i + 256, ... of sample 0, 1, ... in that order, then a fixed tree over the 256 partial sums
__global__ __launch_bounds__(256) void det_dwx_kernel(int b, int c, int T, long long go_bstride, const float *__restrict__ grad_out,
                                                      const float *__restrict__ rel, float *__restrict__ dwx) {
    __shared__ float red[3][256];
    const int ch = blockIdx.x, t0 = threadIdx.x;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int bb = 0; bb < b; ++bb) {
        const float *g = grad_out + (size_t)bb * go_bstride + (size_t)ch * T;
        const float *r = rel + (size_t)bb * 3 * T;
        for (int t = t0; t < T; t += 256) {
            const float v = g[t];
            a0 = fmaf(v, r[t], a0);
            a1 = fmaf(v, r[(size_t)T + t], a1);
            a2 = fmaf(v, r[2 * (size_t)T + t], a2);
        }
    }
    red[0][t0] = a0; red[1][t0] = a1; red[2][t0] = a2;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t0 < off) {
            red[0][t0] += red[0][t0 + off]; red[1][t0] += red[1][t0 + off]; red[2][t0] += red[2][t0 + off];
        }
        __syncthreads();
    }
    if (t0 < 3) dwx[ch * 3 + t0] += red[t0][0];
}

int group_bwd(const char *name, int b, int c, int n, int T, const float *grad_out, const int *idx,
              float *grad_points, ogc_stream_t stream, long long go_bstride = -1, const float *rel = nullptr,
              float *dwx = nullptr) {
    // rel / dwx: also accumulate dwx[ch, k] += sum grad_out * rel (LDS path only; the caller checks group_bwd_fuses_wx)
    if (go_bstride < 0) go_bstride = (long long)c * T;
    OGC_REQUIRE(b >= 0 && c >= 0 && n >= 0 && T >= 0, "%s: negative dimension", name);
    if (b == 0 || c == 0 || T == 0) return OGC_OK;
    OGC_REQUIRE(grad_out && idx && grad_points, "%s: null pointer", name);
    OGC_REQUIRE(go_bstride < (1ll << 31) && (long long)c * n < (1ll << 31) && b <= 65535,
                "%s: one sample exceeds 32-bit indexing", name);
    if (ogc_deterministic()) {
        // every sum in ascending position order, one thread per output (det.hip); the coordinate columns of a grouped first
        // layer's weight gradient by one workgroup per channel in a fixed order
        const int rc = ogc_det_scatter_add(name, b, c, n, T, idx, grad_out, go_bstride, nullptr, 0, grad_points, 1, (hipStream_t)stream);
        if (rc != OGC_OK || !dwx) return rc;
        hipLaunchKernelGGL(det_dwx_kernel, dim3(c), dim3(256), 0, (hipStream_t)stream, b, c, T, go_bstride, grad_out, rel, dwx);
        OGC_CHECK_LAUNCH(name);
        return OGC_OK;
    }
    const Vec4Shape sh = vec4_shape(b, c, T, idx, grad_out, go_bstride);
    // LDS-privatised path: the per-channel image (n floats) must fit a 64 KiB budget at least once
    if (sh.vec && n <= 16384 && T >= 4096 && T % 16 == 0) {
        // channels per workgroup: one channel image of n floats (several only below 1024 points).  Small images mean
        // more workgroups per CU: at C4, 8 channels x 2048 points (64 KiB) ran at 235 us per call, 2 channels at 179 us,
        // 1 at 175 us; 2 x 8192 points at 151 us, 1 x 8192 at 135 us; 4 x 1024 at 231 us, 1 x 1024 at 175 us (the
        // index and rel rows a workgroup re-reads per channel group are small next to its share of the gradient tensor).
        const int cc = lds_image_channels(1024, n, c);
        const int chunks = ogc_divup(c, cc);
        // split T so that >= ~512 workgroups exist, but keep >= 8192 positions per workgroup
        int splits = 1;
        while ((long long)b * chunks * splits < 512 && T / (splits * 2) >= 8192) splits *= 2;
        int tpb = ogc_divup(T, splits);
        tpb = (tpb + 4095) / 4096 * 4096; // multiple of 256 threads x 16 positions
        dim3 grid(ogc_divup(T, tpb), chunks, b);
        const size_t lds = (size_t)cc * n * sizeof(float);
#define GB_LAUNCH(CCV)                                                                                             \
    do {                                                                                                           \
        if (dwx)                                                                                                   \
            hipLaunchKernelGGL((group_bwd_lds_kernel<CCV, true>), grid, dim3(GG_THREADS), lds, (hipStream_t)stream, c, n, \
                               T, tpb, go_bstride, grad_out, idx, grad_points, rel, dwx);                          \
        else                                                                                                       \
            hipLaunchKernelGGL((group_bwd_lds_kernel<CCV, false>), grid, dim3(GG_THREADS), lds, (hipStream_t)stream, c,  \
                               n, T, tpb, go_bstride, grad_out, idx, grad_points, rel, dwx);                       \
    } while (0)
        if (cc == 8) GB_LAUNCH(8);
        else if (cc == 4) GB_LAUNCH(4);
        else if (cc == 2) GB_LAUNCH(2);
        else GB_LAUNCH(1);
#undef GB_LAUNCH
        OGC_CHECK_LAUNCH(name);
        return OGC_OK;
    }
    if (dwx) {
        ogc_set_error("%s: the fused xyz weight gradient needs the LDS path (n <= 16384, T >= 4096, T %% 16 == 0)", name);
        return OGC_ERR_UNSUPPORTED;
    }
    GG_LAUNCH_VEC4(group_bwd_kernel, sh, stream, c, n, T, sh.cpb, go_bstride, grad_out, idx, grad_points);
    OGC_CHECK_LAUNCH(name);
    return OGC_OK;
}

} // namespace

extern "C" int ogc_gather_points(int b, int c, int n, int npoints, const float *points, const int *idx,
                                 float *out, ogc_stream_t stream) {
    return group_fwd("ogc_gather_points", b, c, n, npoints, points, idx, out, stream);
}

extern "C" int ogc_gather_points_grad(int b, int c, int n, int npoints, const float *grad_out,
                                      const int *idx, float *grad_points, ogc_stream_t stream) {
    return group_bwd("ogc_gather_points_grad", b, c, n, npoints, grad_out, idx, grad_points, stream);
}

extern "C" int ogc_group_points(int b, int c, int n, int npoints, int nsample, const float *points,
                                const int *idx, float *out, ogc_stream_t stream) {
    OGC_REQUIRE(npoints >= 0 && nsample >= 0 && (long long)npoints * nsample < (1ll << 31),
                "ogc_group_points: bad npoints/nsample");
    return group_fwd("ogc_group_points", b, c, n, npoints * nsample, points, idx, out, stream);
}

extern "C" int ogc_group_points_grad(int b, int c, int n, int npoints, int nsample, const float *grad_out,
                                     const int *idx, float *grad_points, ogc_stream_t stream) {
    OGC_REQUIRE(npoints >= 0 && nsample >= 0 && (long long)npoints * nsample < (1ll << 31),
                "ogc_group_points_grad: bad npoints/nsample");
    return group_bwd("ogc_group_points_grad", b, c, n, npoints * nsample, grad_out, idx, grad_points, stream);
}

extern "C" int ogc_group_concat(int b, int c, int n, int npoints, int nsample, const float *xyz, const float *new_xyz,
                                const float *points, const int *idx, float *out, ogc_stream_t stream) {
    int T;
    if (const int rc = group_open("ogc_group_concat", b >= 0 && c >= 0 && n >= 0, npoints, nsample, &T)) return rc;
    if (b == 0 || T == 0) return OGC_OK;
    OGC_REQUIRE(xyz && new_xyz && idx && out && (points || c == 0), "ogc_group_concat: null pointer");
    const long long bstride = (long long)(3 + c) * T;
    OGC_REQUIRE(bstride < (1ll << 31) && b <= 65535, "ogc_group_concat: one sample exceeds 32-bit indexing");
    if (c > 0 && nsample > 0 && (long long)c * n < (1ll << 31)) { // both halves in one launch (group_concat_kernel)
        const Vec4Shape sh = vec4_shape(b, c, T, idx, out, bstride, 1);
        GG_LAUNCH_VEC4(group_concat_kernel, sh, stream, c, n, T, nsample, sh.cpb, bstride, points, idx, xyz, new_xyz, out);
        OGC_CHECK_LAUNCH("ogc_group_concat");
        return OGC_OK;
    }
    hipLaunchKernelGGL(group_xyz_rel_kernel, dim3(ogc_divup(T, GG_THREADS), b), dim3(GG_THREADS), 0,
                       (hipStream_t)stream, n, npoints, nsample, bstride, xyz, new_xyz, idx, out);
    OGC_CHECK_LAUNCH("ogc_group_concat");
    if (c == 0) return OGC_OK;
    return group_fwd("ogc_group_concat", b, c, n, T, points, idx, out + 3 * (size_t)T, stream, bstride);
}

extern "C" int ogc_group_linear_bwd(int b, int m, int n, int npoints, int nsample, const float *grad_y, const int *idx,
                                    const float *rel, float *grad_p, float *dwx, ogc_stream_t stream) {
    int T;
    if (const int rc = group_open("ogc_group_linear_bwd", b >= 0 && m >= 1 && n >= 1, npoints, nsample, &T)) return rc;
    if (b == 0 || T == 0) return OGC_OK;
    OGC_REQUIRE(grad_y && idx && rel && grad_p && dwx, "ogc_group_linear_bwd: null pointer");
    if (!aligned16(rel) || !aligned16(grad_y) || !aligned16(idx)) {
        ogc_set_error("ogc_group_linear_bwd: tensors must be 16-byte aligned");
        return OGC_ERR_UNSUPPORTED;
    }
    return group_bwd("ogc_group_linear_bwd", b, m, n, T, grad_y, idx, grad_p, stream, -1, rel, dwx);
}

extern "C" int ogc_group_concat_grad(int b, int c, int n, int npoints, int nsample, const float *grad_out,
                                     const int *idx, float *grad_points, ogc_stream_t stream) {
    int T;
    if (const int rc = group_open("ogc_group_concat_grad", b >= 0 && c >= 0 && n >= 0, npoints, nsample, &T)) return rc;
    if (b == 0 || c == 0 || T == 0) return OGC_OK;
    OGC_REQUIRE(grad_out, "ogc_group_concat_grad: null pointer");
    return group_bwd("ogc_group_concat_grad", b, c, n, T, grad_out + 3 * (size_t)T, idx, grad_points, stream,
                     (long long)(3 + c) * T);
}

// soft_carry.hip — values carried over a soft correspondence, fused:  out = softmax_rows(-cdist(p1, p2) / temperature) @ x.
//
// Reference (vote.py:17-28 followed by the products of :52-58, :112-122): the (N1, N2) correspondence of a flow-warped frame with
// its neighbour is materialised (268 MB at KITTI-SF's 8192 points, plus cdist's temporaries) and then multiplied into thin
// matrices — the masks of the frames inside the voting window, with a column of ones for the row normalisers.  Nothing of size
// N1 x N2 needs to exist: per query m
//     out_m = sum_n e_mn x_n / sum_n e_mn,   e_mn = exp(y_mn - max_n y_mn),   y_mn = -d_mn / temperature.
// Both products run on v_mfma_f32_16x16x4_f32.  The score tile is computed TRANSPOSED (rows = 16 candidates, columns = 16
// queries: the operands of soft_nn_mfma_kernel's distance MFMAs swapped), because in the MFMA's result layout register r of lane l
// then holds candidate 4 (l >> 4) + r and query l & 15 — exactly a B operand (k = l >> 4, n = l & 15) of
//     out^T (channels x queries) += X^T (channels x candidates) . P^T (candidates x queries):
// four MFMAs per 16 channels per tile, MFMA r covering the candidates {r, 4 + r, 8 + r, 12 + r} of the tile, its A operand
// X[candidate 4 (l >> 4) + r][channel l & 15].  The weights never leave the registers they were computed in.
// The maximum is taken FIRST: pass 1 walks the candidates with the two distance MFMAs only and keeps the smallest squared distance
// of every query (clamp, sqrt and the negative scale are monotone, so that is the largest score, computed from bit-identical
// MFMA results), pass 2 walks them again with that maximum fixed.  Against a running maximum this repeats two of the
// 2 + 4 NT MFMAs of a tile but needs no rescaling of the accumulators — whose factor is per query COLUMN here, spread over four lane
// groups, so every rescaling step would need two cross-lane exchanges — and no exponential for the factor; the weights are
// exp2(y - max) <= 1 with the nearest candidate's exactly 1.
// Distances follow torch.cdist's matrix path as in soft_nn.hip (|a|^2 + |b|^2 - 2 a.b as one reduction, clamp, sqrt), so the
// values track the reference's fp32 where that form is ill-conditioned; exponentials in base 2 with log2(e) folded into the
// -1 / temperature scale.  The candidates and x are constant over a call: packed once into the operand layout in the stream's
// workspace.  The SC_SPLITS wavefronts of a workgroup share QT tiles of 16 queries and split the candidates; their partial sums
// are added through LDS in wavefront order, so a result does not depend on the batch it was computed in.
#include "ogc_common.h"

namespace {

typedef float sc_v4f __attribute__((ext_vector_type(4)));
constexpr int SC_SPLITS = 4;     // wavefronts per workgroup = splits of the candidate range
constexpr float SC_FAR = 1e30f;  // |b|^2 of a padding candidate: finite, its weight exp2(-huge) = 0

// floats of a packed candidate tile: (x, y, z, 1) and (|b|^2, 0, 0, 0) as 4 x 16 operand blocks, then per 16 channels 64 lanes x 4
constexpr int sc_block(int nt) { return 128 + nt * 256; }

// one thread per (candidate, channel slot) of the padded table (b, tiles_pad, sc_block(NT))
template <int NT>
__global__ __launch_bounds__(256) void soft_carry_pack_kernel(long long total, int n2, int c, int tiles_pad,
                                                              const float *__restrict__ p2, const float *__restrict__ x,
                                                              float *__restrict__ table) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    const int cs = (int)(g % (NT * 16));
    const long long jj = g / (NT * 16);
    const int j = (int)(jj % (tiles_pad * 16)), b = (int)(jj / (tiles_pad * 16));
    const bool real = j < n2;
    const int cl = j & 15;
    float *t = table + ((size_t)b * tiles_pad + (j >> 4)) * sc_block(NT);
    const float v = (real && cs < c) ? x[((size_t)b * n2 + j) * c + cs] : 0.f;
    t[128 + (cs >> 4) * 256 + (((cl >> 2) * 16 + (cs & 15)) << 2) + (cl & 3)] = v;
    if (cs == 0) {
        float px = 0.f, py = 0.f, pz = 0.f, nn = SC_FAR;
        if (real) {
            const float *p = p2 + ((size_t)b * n2 + j) * 3;
            px = p[0]; py = p[1]; pz = p[2];
            nn = (px * px + py * py) + pz * pz;
        }
        t[cl] = px; t[16 + cl] = py; t[32 + cl] = pz; t[48 + cl] = 1.0f;
        t[64 + cl] = nn; t[80 + cl] = 0.f; t[96 + cl] = 0.f; t[112 + cl] = 0.f;
    }
}

template <int NT, int QT>
__global__ __launch_bounds__(SC_SPLITS *OGC_WAVE) void soft_carry_kernel(int n1, int c, int tiles_pad, int qblocks, float scale2,
                                                                         const float *__restrict__ p1,
                                                                         const float *__restrict__ table,
                                                                         float *__restrict__ out) {
    constexpr int BLK = sc_block(NT);
    __shared__ __attribute__((aligned(16))) float part[SC_SPLITS][QT * NT * 256];
    __shared__ float smin[SC_SPLITS][QT * 16], zs[SC_SPLITS][QT * 16];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col = lane & 15, kk = lane >> 4;
    const int b = blockIdx.x / qblocks, qbase = (blockIdx.x - b * qblocks) * (QT * 16);
    // B operands: lane (col, kk) supplies element kk of query column `col`
    float q1[QT], q2[QT];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        const int q = qbase + qt * 16 + col;
        float x = 0.f, y = 0.f, z = 0.f;
        if (q < n1) {
            const float *p = p1 + ((size_t)b * n1 + q) * 3;
            x = p[0]; y = p[1]; z = p[2];
        }
        const float an = (x * x + y * y) + z * z;
        q1[qt] = kk == 0 ? -2.f * x : kk == 1 ? -2.f * y : kk == 2 ? -2.f * z : an;
        q2[qt] = kk == 0 ? 1.f : 0.f;
    }
    const int per = tiles_pad / SC_SPLITS;
    const float *tb = table + ((size_t)b * tiles_pad + (size_t)wave * per) * BLK + lane;
    const sc_v4f zero = {0.f, 0.f, 0.f, 0.f};

    // pass 1: the smallest squared distance of every query
    float dmin[QT];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) dmin[qt] = 3.0e38f;
    for (int t = 0; t < per; ++t) {
        const float a1 = tb[(size_t)t * BLK], a2 = tb[(size_t)t * BLK + 64];
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
            sc_v4f dd = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, q1[qt], zero, 0, 0, 0);
            dd = __builtin_amdgcn_mfma_f32_16x16x4f32(a2, q2[qt], dd, 0, 0, 0);
            dmin[qt] = fminf(dmin[qt], fminf(fminf(dd[0], dd[1]), fminf(dd[2], dd[3])));
        }
    }
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        float d = dmin[qt];
        d = fminf(d, __shfl_xor(d, 16, 64));
        d = fminf(d, __shfl_xor(d, 32, 64));
        if (kk == 0) smin[wave][qt * 16 + col] = d;
    }
    __syncthreads();
    float ymax[QT];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        float d = smin[0][qt * 16 + col];
#pragma unroll
        for (int w = 1; w < SC_SPLITS; ++w) d = fminf(d, smin[w][qt * 16 + col]);
        ymax[qt] = __builtin_amdgcn_sqrtf(fmaxf(d, 1e-30f)) * scale2;
    }

    // pass 2: weights against the fixed maximum, straight into the second product
    sc_v4f acc[QT][NT];
    float z[QT];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        z[qt] = 0.f;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[qt][nt] = zero;
    }
    for (int t = 0; t < per; ++t) {
        const float *tt = tb + (size_t)t * BLK;
        const float a1 = tt[0], a2 = tt[64];
        sc_v4f xa[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) xa[nt] = *reinterpret_cast<const sc_v4f *>(tt - lane + 128 + nt * 256 + lane * 4);
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
            sc_v4f dd = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, q1[qt], zero, 0, 0, 0);
            dd = __builtin_amdgcn_mfma_f32_16x16x4f32(a2, q2[qt], dd, 0, 0, 0);
            float e[4];
#pragma unroll
            for (int r = 0; r < 4; ++r)
                e[r] = __builtin_amdgcn_exp2f(__builtin_amdgcn_sqrtf(fmaxf(dd[r], 1e-30f)) * scale2 - ymax[qt]);
            z[qt] += (e[0] + e[1]) + (e[2] + e[3]);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    acc[qt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[nt][r], e[r], acc[qt][nt], 0, 0, 0);
        }
    }
    // a lane's z covers the candidates of its lane group: add the four groups, then the wavefronts through LDS
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        float s = z[qt];
        s += __shfl_xor(s, 16, 64);
        s += __shfl_xor(s, 32, 64);
        if (kk == 0) zs[wave][qt * 16 + col] = s;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) *reinterpret_cast<sc_v4f *>(&part[wave][(qt * NT + nt) * 256 + lane * 4]) = acc[qt][nt];
    }
    __syncthreads();
    // register r of lane l of tile (qt, nt): channel 16 nt + 4 (l >> 4) + r of query 16 qt + (l & 15)
    for (int i = threadIdx.x; i < QT * 16 * c; i += SC_SPLITS * OGC_WAVE) {
        const int q = i / c, ch = i - q * c;
        if (qbase + q >= n1) break;
        const int pos = ((q >> 4) * NT + (ch >> 4)) * 256 + ((((ch & 15) >> 2) * 16 + (q & 15)) << 2) + (ch & 3);
        float s = part[0][pos], zz = zs[0][q];
#pragma unroll
        for (int w = 1; w < SC_SPLITS; ++w) {
            s += part[w][pos];
            zz += zs[w][q];
        }
        out[((size_t)b * n1 + qbase + q) * c + ch] = s / zz;
    }
}

template <int NT, int QT>
int soft_carry_launch(int b, int n1, int n2, int c, float temperature, const float *p1, const float *p2, const float *x,
                      float *out, hipStream_t s) {
    const int tiles_pad = ogc_divup(ogc_divup(n2, 16), SC_SPLITS) * SC_SPLITS;
    const int qblocks = ogc_divup(n1, QT * 16);
    const long long pack_total = (long long)b * tiles_pad * 16 * NT * 16;
    if ((long long)b * qblocks > 2147483647LL || (pack_total + 255) / 256 > 2147483647LL) {
        ogc_set_error("ogc_soft_carry: b = %d, n1 = %d, n2 = %d is beyond the launch grid", b, n1, n2);
        return OGC_ERR_UNSUPPORTED;
    }
    float *table = static_cast<float *>(ogc_workspace(s, (size_t)b * tiles_pad * sc_block(NT) * sizeof(float) + 64));
    if (!table) {
        ogc_set_error("ogc_soft_carry: no workspace for the packed candidates");
        return OGC_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(soft_carry_pack_kernel<NT>, dim3((unsigned)((pack_total + 255) / 256)), dim3(256), 0, s, pack_total, n2, c,
                       tiles_pad, p2, x, table);
    const float scale2 = (float)(-1.4426950408889634 / (double)temperature);
    hipLaunchKernelGGL((soft_carry_kernel<NT, QT>), dim3((unsigned)(b * qblocks)), dim3(SC_SPLITS * OGC_WAVE), 0, s, n1, c, tiles_pad,
                       qblocks, scale2, p1, table, out);
    OGC_CHECK_LAUNCH("ogc_soft_carry");
    return OGC_OK;
}

} // namespace

extern "C" int ogc_soft_carry(int b, int n1, int n2, int c, float temperature, const float *p1, const float *p2, const float *x,
                              float *out, ogc_stream_t stream) {
    OGC_REQUIRE(b >= 0 && n1 >= 0 && n2 >= 1 && c >= 1, "ogc_soft_carry: bad shape");
    OGC_REQUIRE(temperature > 0.0f, "ogc_soft_carry: temperature must be positive");
    if (b == 0 || n1 == 0) return OGC_OK;
    OGC_REQUIRE(p1 && p2 && x && out, "ogc_soft_carry: null pointer");
    if (c > 64) {
        ogc_set_error("ogc_soft_carry: more than 64 columns (c=%d); split x by columns", c);
        return OGC_ERR_UNSUPPORTED;
    }
    hipStream_t s = (hipStream_t)stream;
    // four query tiles per wavefront while the accumulators are small (every tile of queries re-reads the packed candidates)
    if (c <= 16) return soft_carry_launch<1, 4>(b, n1, n2, c, temperature, p1, p2, x, out, s);
    if (c <= 32) return soft_carry_launch<2, 4>(b, n1, n2, c, temperature, p1, p2, x, out, s);
    if (c <= 48) return soft_carry_launch<3, 2>(b, n1, n2, c, temperature, p1, p2, x, out, s);
    return soft_carry_launch<4, 2>(b, n1, n2, c, temperature, p1, p2, x, out, s);
}

// nearest_label.hip — label transfer by the nearest source point: what data_prepare/ogcdrsv/collect_segm.py:59-61 does
// with scipy, `segm_src[cdist(pc, pc_src).argmin(1)]`, for a batch of frames in one launch.
//
//   distance   sqrt(((dx*dx) + (dy*dy)) + (dz*dz)) in fp64 from the fp32 inputs, one rounding per operation, the square root
//              correctly rounded: cdist's expression.  The ROOT is compared, not the square: two squares can round to one root,
//              and argmin then takes the earlier index.
//   ties       the lowest source index among the minima (a strict `<` over ascending indices).
//   geometry   a thread per query, 256 queries per workgroup, the sample's source points staged through LDS 1024 at a time.
#include <math.h>

#include "ogc_common.h"

namespace {

constexpr int NL_THREADS = 256;
constexpr int NL_TILE = 1024;

__global__ __launch_bounds__(NL_THREADS) void nearest_label_kernel(int Nq, int Ns, const float *__restrict__ query,
                                                                   const float *__restrict__ source, const int *__restrict__ labels,
                                                                   int *__restrict__ out_label, int *__restrict__ out_idx) {
#pragma clang fp contract(off)
    __shared__ float tile[NL_TILE * 3];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int q = blockIdx.x * NL_THREADS + tid;
    const bool live = q < Nq;
    const float *src = source + (size_t)b * Ns * 3;
    double x = 0.0, y = 0.0, z = 0.0;
    if (live) {
        const float *p = query + ((size_t)b * Nq + q) * 3;
        x = (double)p[0];
        y = (double)p[1];
        z = (double)p[2];
    }
    double best = INFINITY;
    int best_idx = 0;
    for (int base = 0; base < Ns; base += NL_TILE) {
        const int cnt = min(NL_TILE, Ns - base);
        __syncthreads(); // the previous tile has been read by everyone
        for (int e = tid; e < cnt * 3; e += NL_THREADS) tile[e] = src[(size_t)base * 3 + e];
        __syncthreads();
        if (live) {
            for (int s = 0; s < cnt; ++s) { // every lane reads the same address: a broadcast
                const double dx = x - (double)tile[s * 3 + 0], dy = y - (double)tile[s * 3 + 1], dz = z - (double)tile[s * 3 + 2];
                const double d = __dsqrt_rn(((dx * dx) + (dy * dy)) + (dz * dz));
                if (d < best) {
                    best = d;
                    best_idx = base + s;
                }
            }
        }
    }
    if (live) {
        out_idx[(size_t)b * Nq + q] = best_idx;
        out_label[(size_t)b * Nq + q] = labels[(size_t)b * Ns + best_idx];
    }
}

} // namespace

extern "C" int ogc_nearest_label(int B, int Nq, int Ns, const float *query, const float *source, const int *labels, int *out_label,
                                 int *out_idx, ogc_stream_t stream) {
    const char *name = "ogc_nearest_label";
    OGC_REQUIRE(B >= 0 && Nq >= 0 && Ns >= 0, "%s: negative size (B = %d, Nq = %d, Ns = %d)", name, B, Nq, Ns);
    OGC_REQUIRE(B <= 65535, "%s: B = %d, at most 65535 samples per call", name, B);
    OGC_REQUIRE((long long)B * Nq <= 0x7fffffff / 3 && (long long)B * Ns <= 0x7fffffff / 3, "%s: B * Nq = %lld, B * Ns = %lld beyond 32-bit indexing",
                name, (long long)B * Nq, (long long)B * Ns);
    if (B == 0 || Nq == 0) return OGC_OK;
    OGC_REQUIRE(Ns >= 1, "%s: Ns = %d, a query needs a source point", name, Ns);
    OGC_REQUIRE(query && source && labels && out_label && out_idx, "%s: null pointer (query, source, labels, out_label or out_idx)", name);
    hipLaunchKernelGGL(nearest_label_kernel, dim3((unsigned)ogc_divup(Nq, NL_THREADS), (unsigned)B), dim3(NL_THREADS), 0, (hipStream_t)stream, Nq,
                       Ns, query, source, labels, out_label, out_idx);
    OGC_CHECK_LAUNCH(name);
    return OGC_OK;
}

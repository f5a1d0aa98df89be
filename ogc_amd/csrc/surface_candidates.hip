// surface_candidates.hip — area-weighted random points on the triangles of the meshes of one frame, fp64.  Replaces the
// candidate draw of trimesh.sample.sample_surface inside data_prepare/ogcdr/sample_pointcloud.py:57 with a counter-based form: a
// candidate is a function of (seed, mesh, index in the mesh) and of that mesh's faces alone.
//
//   inputs     vertices (V, 3) f64 and faces (F, 3) i32 of all meshes concatenated (faces index the concatenated vertices);
//              cum_area (F) f64, per mesh the running sum of its face areas; face_offsets, cand_offsets (M + 1) i32.
//   random     Philox4x32-10, key = the two halves of the seed, counter = (j, m, block, 0) for candidate j of mesh m; block 0 gives
//              u0 (words 0, 1) and u1 (words 2, 3), block 1 gives u2 (words 0, 1).  u = ((hi >> 5) * 2^26 + (lo >> 6)) * 2^-53.
//   face       pick = u0 * total; the first face whose running sum exceeds pick (searchsorted side = "right"), clamped to the first
//              face whose running sum reaches the total, i.e. the mesh's last face of non-zero area.  A face that adds nothing to
//              the running sum is never chosen.
//   point      if u1 + u2 > 1: (u1, u2) = (1 - u1, 1 - u2);  p = (o + u1 * e1) + u2 * e2 per coordinate, one rounding per operation.
//   refusals   checked by one workgroup ahead of the draw, into status[0]: 1 a face index outside [0, V), 2 offsets that do not
//              start at 0, descend or do not end at F / C, 3 a mesh with candidates and no area (or a running sum that is not
//              finite).  With a status set nothing else is written.
#include <math.h>

#include "ogc_common.h"
#include "philox.h"

namespace {

constexpr int SC_THREADS = 256;
constexpr int SC_CHECK_THREADS = 1024;

__global__ __launch_bounds__(SC_CHECK_THREADS) void surface_check_kernel(int C, int M, int V, int F, const int *__restrict__ faces,
                                                                         const double *__restrict__ cum_area,
                                                                         const int *__restrict__ face_offsets,
                                                                         const int *__restrict__ cand_offsets, int *__restrict__ status) {
    const int tid = threadIdx.x;
    int bad_offsets = 0, bad_area = 0, bad_face = 0;
    if (tid == 0 && (face_offsets[0] != 0 || cand_offsets[0] != 0 || face_offsets[M] != F || cand_offsets[M] != C)) bad_offsets = 1;
    for (int m = tid; m < M; m += SC_CHECK_THREADS)
        if (face_offsets[m + 1] < face_offsets[m] || cand_offsets[m + 1] < cand_offsets[m]) bad_offsets = 1;
    bad_offsets = __syncthreads_or(bad_offsets);
    if (!bad_offsets) { // the offsets delimit the arrays: the reads below stay inside them
        for (int m = tid; m < M; m += SC_CHECK_THREADS) {
            const int f0 = face_offsets[m], f1 = face_offsets[m + 1];
            if (cand_offsets[m + 1] > cand_offsets[m]) {
                const double total = f1 > f0 ? cum_area[f1 - 1] : 0.0;
                if (!(total > 0.0) || !isfinite(total)) bad_area = 1;
            }
        }
        for (int e = tid; e < 3 * F; e += SC_CHECK_THREADS) {
            const int v = faces[e];
            if (v < 0 || v >= V) bad_face = 1;
        }
    }
    bad_area = __syncthreads_or(bad_area);
    bad_face = __syncthreads_or(bad_face);
    if (tid == 0) status[0] = bad_offsets ? 2 : bad_face ? 1 : bad_area ? 3 : 0;
}

__global__ __launch_bounds__(SC_THREADS) void surface_candidates_kernel(int C, int M, const double *__restrict__ vertices,
                                                                        const int *__restrict__ faces, const double *__restrict__ cum_area,
                                                                        const int *__restrict__ face_offsets,
                                                                        const int *__restrict__ cand_offsets, uint32_t key0, uint32_t key1,
                                                                        const int *__restrict__ status, double *__restrict__ points,
                                                                        int *__restrict__ face_idx) {
#pragma clang fp contract(off)
    if (status[0] != 0) return;
    const int i = blockIdx.x * SC_THREADS + threadIdx.x;
    if (i >= C) return;
    const int m = ogc_owner(cand_offsets, M, i);
    const uint32_t j = (uint32_t)(i - cand_offsets[m]);
    const Philox4 a = philox4x32_10(j, (uint32_t)m, 0u, 0u, key0, key1);
    const Philox4 b = philox4x32_10(j, (uint32_t)m, 1u, 0u, key0, key1);
    const double u0 = uniform53(a.w[0], a.w[1]);
    double u1 = uniform53(a.w[2], a.w[3]), u2 = uniform53(b.w[0], b.w[1]);

    const int f0 = face_offsets[m], nf = face_offsets[m + 1] - f0;
    const double *cum = cum_area + f0;
    const double total = cum[nf - 1];
    const double pick = u0 * total;
    int lo = 0, hi = nf; // first k with cum[k] > pick
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cum[mid] > pick) hi = mid; else lo = mid + 1;
    }
    int last = 0, top = nf; // first k with cum[k] >= total: the last face that adds area
    while (last < top) {
        const int mid = (last + top) >> 1;
        if (cum[mid] >= total) top = mid; else last = mid + 1;
    }
    const int f = f0 + min(lo, last);

    if (u1 + u2 > 1.0) {
        u1 = 1.0 - u1;
        u2 = 1.0 - u2;
    }
    const double *o = vertices + (size_t)faces[(size_t)f * 3 + 0] * 3;
    const double *p1 = vertices + (size_t)faces[(size_t)f * 3 + 1] * 3;
    const double *p2 = vertices + (size_t)faces[(size_t)f * 3 + 2] * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double e1 = p1[k] - o[k], e2 = p2[k] - o[k];
        points[(size_t)i * 3 + k] = (o[k] + u1 * e1) + u2 * e2;
    }
    face_idx[i] = f;
}

} // namespace

extern "C" int ogc_surface_candidates(int C, int M, int V, int F, const double *vertices, const int *faces, const double *cum_area,
                                      const int *face_offsets, const int *cand_offsets, long long seed, double *points, int *face_idx,
                                      int *status, ogc_stream_t stream) {
    const char *name = "ogc_surface_candidates";
    OGC_REQUIRE(C >= 0 && M >= 0 && V >= 0 && F >= 0, "%s: negative size (C = %d, M = %d, V = %d, F = %d)", name, C, M, V, F);
    OGC_REQUIRE(F <= 0x7fffffff / 3, "%s: F = %d, 3 * F must fit 32-bit indexing", name, F);
    if (C == 0) return OGC_OK;
    OGC_REQUIRE(M >= 1 && V >= 1 && F >= 1, "%s: %d candidates need a mesh (M = %d, V = %d, F = %d)", name, C, M, V, F);
    OGC_REQUIRE(vertices && faces && cum_area && face_offsets && cand_offsets, "%s: null pointer (vertices, faces, cum_area or offsets)", name);
    OGC_REQUIRE(points && face_idx && status, "%s: null pointer (points, face_idx or status)", name);
    hipLaunchKernelGGL(surface_check_kernel, dim3(1), dim3(SC_CHECK_THREADS), 0, (hipStream_t)stream, C, M, V, F, faces, cum_area,
                       face_offsets, cand_offsets, status);
    OGC_CHECK_LAUNCH(name);
    const unsigned long long s = (unsigned long long)seed;
    hipLaunchKernelGGL(surface_candidates_kernel, dim3((unsigned)ogc_divup(C, SC_THREADS)), dim3(SC_THREADS), 0, (hipStream_t)stream, C, M,
                       vertices, faces, cum_area, face_offsets, cand_offsets, (uint32_t)(s & 0xffffffffu), (uint32_t)(s >> 32), status,
                       points, face_idx);
    OGC_CHECK_LAUNCH(name);
    return OGC_OK;
}

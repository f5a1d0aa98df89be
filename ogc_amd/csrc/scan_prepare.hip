// scan_prepare.hip — the two device stages of data preparation around FPS: the crop of a raw scan to the front-view
// cloud, and the labelling of points by oriented boxes.
//
// Crop (ogc_scan_crop_camera / ogc_scan_crop_front): one kernel pair, the predicate a template parameter.
//   camera   process_kittidet.py:99-114, process_semantickitti.py:61-78: projection of every point into the image in fp64
//            (V2C, optionally R0, P, division), five comparisons, the kept point is fp32(rect * (-1, -1, 1)), then the depth
//            test on that fp32 value.  A zero img2 gives inf / NaN pixels, which fail the comparisons as they do in numpy.
//   front    process_waymo.py:132-141: five fp32 comparisons on an (N, 6) scan, each operation rounded once (the *_rn
//            intrinsics), the kept point is the input xyz.
// The reference indexes with the boolean mask — a STABLE compaction, and FPS starts at row 0 and breaks ties by index, so the
// order is part of the result.  Two ordinary launches on the caller's stream, no waiting between workgroups:
//   count    a workgroup per tile of OGC_SCAN_CROP_TILE points evaluates the predicate and stores the tile's number of kept
//            points in the stream's workspace;
//   scatter  every workgroup adds up the counts of the tiles before its own (a few hundred integers at 180 000 points),
//            RECOMPUTES the predicate — the same device function on the same bits, compiled without contraction, so the same
//            decisions; a bit mask would be one more buffer for a predicate of at most ~40 fp64 operations — ranks the kept
//            points of its tile by a wave ballot plus the 16 wave totals in LDS, and writes them.  The last tile also writes
//            `count`.  Whatever the predicate said, a row index is below the number of points before it: no write goes past
//            row n - 1.
// Tile layout: round j of a 256-thread workgroup takes the points tile * T + j * 256 + tid (coalesced rows), so the scan order
// inside a tile is (round, wave, lane).
//
// Labelling (ogc_box_segm): process_waymo.py:48-84 and process_kittidet.py:33-65 are loops over the boxes that overwrite the
// labels of the points inside — the label of a point is that of the LAST box holding it.  One thread per point; the boxes
// (18 doubles and 2 ints each) pass through LDS in chunks of OGC_BOX_SEGM_CHUNK, from the last chunk to the first, every
// lane reading the same address (a broadcast); a thread stops at its first hit and a workgroup once all its points are hit.
//   d = sign * p - c,  q_i = (rot_i0 d_0 + rot_i1 d_1) + rot_i2 d_2  in fp64,  inside iff lo_i < q_i < hi_i on all axes.
#include "ogc_common.h"

namespace {

constexpr int SP_THREADS = 256;
constexpr int SP_WAVES = SP_THREADS / OGC_WAVE;
constexpr int SP_ROUNDS = OGC_SCAN_CROP_TILE / SP_THREADS;
static_assert(OGC_SCAN_CROP_TILE % SP_THREADS == 0, "a tile is a whole number of rounds");

struct CropCamera {
    const double *cam; // OGC_SCAN_CROP_CAMERA_DOUBLES values, layout in include/ogc_ops.h
    float clip, depth;
    static constexpr int MIN_STRIDE = 3;
    // true: the point is kept and (ox, oy, oz) is what is stored for it
    __device__ __forceinline__ bool operator()(const float *__restrict__ p, float &ox, float &oy, float &oz) const {
        const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
        const double *V = cam, *R = cam + 12, *P = cam + 21;
        double r0 = ((V[0] * x + V[1] * y) + V[2] * z) + V[3];
        double r1 = ((V[4] * x + V[5] * y) + V[6] * z) + V[7];
        double r2 = ((V[8] * x + V[9] * y) + V[10] * z) + V[11];
        if (cam[35] != 0.0) {
            const double a = r0, b = r1, c = r2;
            r0 = (R[0] * a + R[1] * b) + R[2] * c;
            r1 = (R[3] * a + R[4] * b) + R[5] * c;
            r2 = (R[6] * a + R[7] * b) + R[8] * c;
        }
        const double i0 = ((P[0] * r0 + P[1] * r1) + P[2] * r2) + P[3];
        const double i1 = ((P[4] * r0 + P[5] * r1) + P[6] * r2) + P[7];
        const double i2 = ((P[8] * r0 + P[9] * r1) + P[10] * r2) + P[11];
        const double u = i0 / i2, v = i1 / i2;
        ox = (float)(-r0);
        oy = (float)(-r1);
        oz = (float)r2;
        return u < cam[33] && u >= 0.0 && v < cam[34] && v >= 0.0 && p[0] > clip && oz < depth;
    }
};

struct CropFront {
    static constexpr int MIN_STRIDE = 6;
    __device__ __forceinline__ bool operator()(const float *__restrict__ p, float &ox, float &oy, float &oz) const {
        const float x = p[0], y = p[1], z = p[2];
        ox = x;
        oy = y;
        oz = z;
        const float ay = fabsf(y);
        const float r2 = __fadd_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)), __fmul_rn(z, z));
        return p[5] == -1.0f && x > ay && r2 < 3600.0f && ay < 50.0f && x < 35.0f;
    }
};

template <class Pred>
__global__ __launch_bounds__(SP_THREADS) void scan_crop_count_kernel(int n, int stride, const float *__restrict__ scan, Pred pred,
                                                                     int *__restrict__ tile_count) {
    __shared__ int wave_total[SP_WAVES];
    const int tid = threadIdx.x, lane = tid & (OGC_WAVE - 1), wave = tid / OGC_WAVE;
    const long long first = (long long)blockIdx.x * OGC_SCAN_CROP_TILE;
    int kept = 0;
#pragma unroll
    for (int j = 0; j < SP_ROUNDS; ++j) {
        const long long i = first + j * SP_THREADS + tid;
        float ox, oy, oz;
        const bool keep = i < n && pred(scan + (size_t)i * stride, ox, oy, oz);
        kept += __popcll(__ballot(keep)); // uniform over the wave
    }
    if (lane == 0) wave_total[wave] = kept;
    __syncthreads();
    if (tid == 0) {
        int total = 0;
        for (int w = 0; w < SP_WAVES; ++w) total += wave_total[w];
        tile_count[blockIdx.x] = total;
    }
}

template <class Pred>
__global__ __launch_bounds__(SP_THREADS) void scan_crop_scatter_kernel(int n, int stride, const float *__restrict__ scan, Pred pred,
                                                                       const int *__restrict__ tile_count,
                                                                       float *__restrict__ out_pc, int *__restrict__ keep_idx,
                                                                       int *__restrict__ count) {
    __shared__ int before[SP_WAVES];                // partial sums of the counts of the earlier tiles
    __shared__ int wave_total[SP_ROUNDS][SP_WAVES]; // kept points of (round, wave) of this tile
    const int tid = threadIdx.x, lane = tid & (OGC_WAVE - 1), wave = tid / OGC_WAVE;
    const int tile = blockIdx.x;
    const long long first = (long long)tile * OGC_SCAN_CROP_TILE;

    int acc = 0;
    for (int t = tid; t < tile; t += SP_THREADS) acc += tile_count[t];
#pragma unroll
    for (int off = OGC_WAVE / 2; off > 0; off >>= 1) acc += __shfl_down(acc, off, OGC_WAVE);
    if (lane == 0) before[wave] = acc;

    bool keep[SP_ROUNDS];
    float ox[SP_ROUNDS], oy[SP_ROUNDS], oz[SP_ROUNDS];
    int rank[SP_ROUNDS]; // kept points of the same wave and round in front of this one
#pragma unroll
    for (int j = 0; j < SP_ROUNDS; ++j) {
        const long long i = first + j * SP_THREADS + tid;
        keep[j] = i < n && pred(scan + (size_t)i * stride, ox[j], oy[j], oz[j]);
        const unsigned long long m = __ballot(keep[j]);
        rank[j] = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wave_total[j][wave] = __popcll(m);
    }
    __syncthreads();

    int base = 0;
    for (int w = 0; w < SP_WAVES; ++w) base += before[w];
    int row = base;
#pragma unroll
    for (int j = 0; j < SP_ROUNDS; ++j) {
#pragma unroll
        for (int w = 0; w < SP_WAVES; ++w) {
            const int c = wave_total[j][w];
            if (w == wave && keep[j]) {
                const int r = row + rank[j]; // < the number of points before this one: inside the n rows
                out_pc[(size_t)r * 3 + 0] = ox[j];
                out_pc[(size_t)r * 3 + 1] = oy[j];
                out_pc[(size_t)r * 3 + 2] = oz[j];
                keep_idx[r] = (int)(first + j * SP_THREADS + tid);
            }
            row += c;
        }
    }
    if (tile == (int)gridDim.x - 1 && tid == 0) *count = row;
}

template <class Pred>
int scan_crop_launch(const char *name, int n, int stride, const float *scan, const Pred &pred, float *out_pc, int *keep_idx,
                     int *count, ogc_stream_t stream) {
    OGC_REQUIRE(n >= 0, "%s: n = %d is negative", name, n);
    OGC_REQUIRE(stride >= Pred::MIN_STRIDE, "%s: stride = %d, the scan needs at least %d columns", name, stride, Pred::MIN_STRIDE);
    OGC_REQUIRE(count != nullptr, "%s: null pointer (count)", name);
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        if (hipMemsetAsync(count, 0, sizeof(int), s) != hipSuccess) {
            ogc_set_error("%s: could not clear count", name);
            return OGC_ERR_LAUNCH;
        }
        return OGC_OK;
    }
    OGC_REQUIRE(scan && out_pc && keep_idx, "%s: null pointer", name);
    const int tiles = ogc_divup(n, OGC_SCAN_CROP_TILE);
    int *tile_count = static_cast<int *>(ogc_workspace(s, (size_t)tiles * sizeof(int)));
    if (!tile_count) {
        ogc_set_error("%s: no workspace for the tile counts", name);
        return OGC_ERR_LAUNCH;
    }
    hipLaunchKernelGGL((scan_crop_count_kernel<Pred>), dim3(tiles), dim3(SP_THREADS), 0, s, n, stride, scan, pred, tile_count);
    OGC_CHECK_LAUNCH(name);
    hipLaunchKernelGGL((scan_crop_scatter_kernel<Pred>), dim3(tiles), dim3(SP_THREADS), 0, s, n, stride, scan, pred, tile_count,
                       out_pc, keep_idx, count);
    OGC_CHECK_LAUNCH(name);
    return OGC_OK;
}

// ---- labelling by boxes ----------------------------------------------------------------------------------------------------
constexpr int BS_THREADS = 256;
constexpr int BS_BOX = OGC_BOX_SEGM_BOX_DOUBLES;

__global__ __launch_bounds__(BS_THREADS) void box_segm_kernel(int n, int k, const float *__restrict__ pc, float sx, float sy, float sz,
                                                              const double *__restrict__ boxes, const int *__restrict__ ids,
                                                              int *__restrict__ segm, int *__restrict__ semantic_segm) {
    __shared__ double box[OGC_BOX_SEGM_CHUNK * BS_BOX];
    __shared__ int id[OGC_BOX_SEGM_CHUNK * 2];
    const int tid = threadIdx.x;
    const long long i = (long long)blockIdx.x * BS_THREADS + tid;
    const bool live = i < n;
    double px = 0.0, py = 0.0, pz = 0.0;
    if (live) { // the sign is +-1: the product is exact in fp32
        px = (double)__fmul_rn(sx, pc[(size_t)i * 3 + 0]);
        py = (double)__fmul_rn(sy, pc[(size_t)i * 3 + 1]);
        pz = (double)__fmul_rn(sz, pc[(size_t)i * 3 + 2]);
    }
    int object = 0, cls = 0;
    bool open = live; // no box found yet
    const int chunks = (k + OGC_BOX_SEGM_CHUNK - 1) / OGC_BOX_SEGM_CHUNK;
    for (int c = chunks - 1; c >= 0; --c) {
        const int k0 = c * OGC_BOX_SEGM_CHUNK;
        const int kc = min(OGC_BOX_SEGM_CHUNK, k - k0);
        for (int e = tid; e < kc * BS_BOX; e += BS_THREADS) box[e] = boxes[(size_t)k0 * BS_BOX + e];
        for (int e = tid; e < kc * 2; e += BS_THREADS) id[e] = ids[(size_t)k0 * 2 + e];
        __syncthreads();
        if (open) {
            for (int j = kc - 1; j >= 0; --j) {
                const double *b = box + j * BS_BOX;
                const double d0 = px - b[9], d1 = py - b[10], d2 = pz - b[11];
                const double q0 = (b[0] * d0 + b[1] * d1) + b[2] * d2;
                const double q1 = (b[3] * d0 + b[4] * d1) + b[5] * d2;
                const double q2 = (b[6] * d0 + b[7] * d1) + b[8] * d2;
                if (b[12] < q0 && q0 < b[15] && b[13] < q1 && q1 < b[16] && b[14] < q2 && q2 < b[17]) {
                    object = id[2 * j];
                    cls = id[2 * j + 1];
                    open = false;
                    break;
                }
            }
        }
        if (__syncthreads_or(open) == 0) break; // also the barrier before the next chunk overwrites the LDS
    }
    if (live) {
        segm[i] = object;
        semantic_segm[i] = cls;
    }
}

} // namespace

extern "C" int ogc_scan_crop_camera(int n, int stride, const float *scan, const double *cam, float clip_distance,
                                    float depth_thresh, float *out_pc, int *keep_idx, int *count, ogc_stream_t stream) {
    OGC_REQUIRE(n == 0 || cam != nullptr, "ogc_scan_crop_camera: null pointer (cam)");
    return scan_crop_launch("ogc_scan_crop_camera", n, stride, scan, CropCamera{cam, clip_distance, depth_thresh}, out_pc, keep_idx,
                            count, stream);
}

extern "C" int ogc_scan_crop_front(int n, int stride, const float *scan, float *out_pc, int *keep_idx, int *count,
                                   ogc_stream_t stream) {
    return scan_crop_launch("ogc_scan_crop_front", n, stride, scan, CropFront{}, out_pc, keep_idx, count, stream);
}

extern "C" int ogc_scan_crop_tile(void) { return OGC_SCAN_CROP_TILE; }

extern "C" int ogc_box_segm_chunk(void) { return OGC_BOX_SEGM_CHUNK; }

extern "C" int ogc_box_segm(int n, int k, const float *pc, int sign_x, int sign_y, int sign_z, const double *boxes, const int *ids,
                            int *segm, int *semantic_segm, ogc_stream_t stream) {
    OGC_REQUIRE(n >= 0 && k >= 0, "ogc_box_segm: negative size (n = %d, k = %d)", n, k);
    OGC_REQUIRE((sign_x == 1 || sign_x == -1) && (sign_y == 1 || sign_y == -1) && (sign_z == 1 || sign_z == -1),
                "ogc_box_segm: sign = (%d, %d, %d), every entry must be 1 or -1", sign_x, sign_y, sign_z);
    if (n == 0) return OGC_OK;
    OGC_REQUIRE(pc && segm && semantic_segm, "ogc_box_segm: null pointer");
    OGC_REQUIRE(k == 0 || (boxes && ids), "ogc_box_segm: null pointer (boxes / ids)");
    hipLaunchKernelGGL(box_segm_kernel, dim3(ogc_divup(n, BS_THREADS)), dim3(BS_THREADS), 0, (hipStream_t)stream, n, k, pc,
                       (float)sign_x, (float)sign_y, (float)sign_z, boxes, ids, segm, semantic_segm);
    OGC_CHECK_LAUNCH("ogc_box_segm");
    return OGC_OK;
}

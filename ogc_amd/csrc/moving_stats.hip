// moving_stats.hip — the three integers per frame pair that the selection of moving Waymo samples needs, for a ragged
// batch of samples in ONE launch.  Replaces, per pair, data_prepare/waymo/select_mov.py:74-96 with the reader's filter_segm
// (datasets/dataset_waymo.py:110-128) on the pair's first frame: two np.unique, two isin, a boolean compaction, an fp64 einsum, a
// norm and a count — of which only three integers leave.
//
//   inputs     the raw arrays of the first frames as stored on disk, concatenated along points; offsets (B + 1) delimits them.
//   geometry   one workgroup of 256 threads per sample; thread t takes the sample's points t, t + 256, ...
//   labels     a table in LDS with two counters per label l in [0, OGC_MOVING_STATS_LABEL_CAP): size[l] the points of object l,
//              kept[l] those of them whose semantic class is not ignored.  The filter sends a point to label 0 when its class is
//              ignored or size[its label] < ignore_npoint_thresh, so the distinct values of the filtered labels are
//                l > 0  iff size[l] >= thresh and kept[l] > 0
//                0      iff size[0] > 0, or a point of an ignored class exists, or an object with 0 < size[l] < thresh exists.
//   points     foreground: y >= ground_y in fp32.  Moving: in fp64 from the fp32 inputs, one rounding per operation, nothing
//              contracted: d_i = ((((r_i0 x + r_i1 y) + r_i2 z) + t_i) - p_i) - f_i,  sqrt((d_0^2 + d_1^2) + d_2^2) > moving_thresh,
//              the square root correctly rounded.
//   sums       integers only: LDS atomic adds into the table, per-thread counters added by a shuffle tree and over the four waves.
//              Nothing depends on the order of the points or on the launch geometry.
//   refusals   per sample, in stats[b][3]: 1 a label outside the table, 2 offsets that descend or leave [0, total].  Such a sample
//              reads nothing beyond what told it so and writes {0, 0, 0, status}; its neighbours are not affected.
#include <math.h>

#include "ogc_common.h"

namespace {

constexpr int MS_THREADS = 256;
constexpr int MS_WAVES = MS_THREADS / OGC_WAVE;
constexpr int MS_CAP = OGC_MOVING_STATS_LABEL_CAP;
static_assert(MS_CAP >= 4096 && MS_CAP % MS_THREADS == 0, "every thread owns the same number of table rows");
static_assert(2 * MS_CAP * sizeof(int) <= 60 * 1024, "the table has to fit the 64 KiB of LDS a workgroup may use");

__device__ __forceinline__ int ms_wave_sum(int v) {
#pragma unroll
    for (int off = OGC_WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, OGC_WAVE);
    return v; // lane 0 holds the sum
}

__global__ __launch_bounds__(MS_THREADS) void moving_stats_kernel(int total, const int *__restrict__ offsets, const float *__restrict__ pc_all,
                                                                  const float *__restrict__ flow_all, const int *__restrict__ segm_all,
                                                                  const int *__restrict__ semantic_all, const double *__restrict__ motion,
                                                                  const int *__restrict__ ignore_ids, int n_ignore, int thresh,
                                                                  float ground_y, double moving_thresh, int *__restrict__ stats) {
#pragma clang fp contract(off)
    __shared__ int size[MS_CAP];
    __shared__ int kept[MS_CAP];
    __shared__ int flags[2];               // [0] a label outside the table, [1] a point of an ignored class
    __shared__ int part[MS_WAVES][4];      // n_distinct (labels > 0), n_fg, n_mov, small objects
    const int tid = threadIdx.x, lane = tid & (OGC_WAVE - 1), wave = tid / OGC_WAVE;
    const int b = blockIdx.x;
    int *out = stats + (size_t)b * 4;
    const int lo = offsets[b], hi = offsets[b + 1];
    if (lo < 0 || hi < lo || hi > total) { // uniform over the workgroup
        if (tid < 4) out[tid] = tid == 3 ? 2 : 0;
        return;
    }
    const int n = hi - lo;
    for (int l = tid; l < MS_CAP; l += MS_THREADS) {
        size[l] = 0;
        kept[l] = 0;
    }
    if (tid < 2) flags[tid] = 0;
    double m[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) m[k] = motion[(size_t)b * 12 + k];
    __syncthreads();

    const float *pc = pc_all + (size_t)lo * 3, *flow = flow_all + (size_t)lo * 3;
    const int *segm = segm_all + lo, *semantic = semantic_all + lo;
    int n_fg = 0, n_mov = 0;
    bool bad = false, ignored_any = false;
    for (int p = tid; p < n; p += MS_THREADS) {
        const int l = segm[p], c = semantic[p];
        if (l < 0 || l >= MS_CAP) {
            bad = true;
        } else {
            bool ignored = false;
            for (int e = 0; e < n_ignore; ++e) ignored |= ignore_ids[e] == c;
            atomicAdd(&size[l], 1);
            if (ignored)
                ignored_any = true;
            else
                atomicAdd(&kept[l], 1);
        }
        const float xf = pc[(size_t)p * 3 + 0], yf = pc[(size_t)p * 3 + 1], zf = pc[(size_t)p * 3 + 2];
        if (yf >= ground_y) {
            const double x = (double)xf, y = (double)yf, z = (double)zf;
            const double d0 = ((((m[0] * x + m[1] * y) + m[2] * z) + m[9]) - x) - (double)flow[(size_t)p * 3 + 0];
            const double d1 = ((((m[3] * x + m[4] * y) + m[5] * z) + m[10]) - y) - (double)flow[(size_t)p * 3 + 1];
            const double d2 = ((((m[6] * x + m[7] * y) + m[8] * z) + m[11]) - z) - (double)flow[(size_t)p * 3 + 2];
            const double norm = __dsqrt_rn((d0 * d0 + d1 * d1) + d2 * d2);
            n_fg += 1;
            n_mov += norm > moving_thresh ? 1 : 0; // a NaN is not moving, as in numpy
        }
    }
    if (bad) atomicOr(&flags[0], 1);
    if (ignored_any) atomicOr(&flags[1], 1);
    __syncthreads();

    int distinct = 0, small = 0;
    for (int l = tid; l < MS_CAP; l += MS_THREADS) {
        const int s = size[l];
        if (l > 0 && s >= thresh && kept[l] > 0) distinct += 1;
        if (l > 0 && s > 0 && s < thresh) small += 1;
    }
    distinct = ms_wave_sum(distinct);
    n_fg = ms_wave_sum(n_fg);
    n_mov = ms_wave_sum(n_mov);
    small = ms_wave_sum(small);
    if (lane == 0) {
        part[wave][0] = distinct;
        part[wave][1] = n_fg;
        part[wave][2] = n_mov;
        part[wave][3] = small;
    }
    __syncthreads();
    if (tid == 0) {
        int t[4] = {0, 0, 0, 0};
        for (int w = 0; w < MS_WAVES; ++w)
            for (int k = 0; k < 4; ++k) t[k] += part[w][k];
        if (flags[0]) {
            out[0] = out[1] = out[2] = 0;
            out[3] = 1;
        } else {
            const int zero = (size[0] > 0 || flags[1] || t[3] > 0) ? 1 : 0;
            out[0] = t[0] + zero;
            out[1] = t[1];
            out[2] = t[2];
            out[3] = 0;
        }
    }
}

} // namespace

extern "C" int ogc_moving_stats_label_cap(void) { return OGC_MOVING_STATS_LABEL_CAP; }

extern "C" int ogc_moving_stats(int B, int total, const int *offsets, const float *pc, const float *flow, const int *segm,
                                const int *semantic_segm, const double *motion, const int *ignore_class_ids, int n_ignore,
                                int ignore_npoint_thresh, double ground_y, double moving_thresh, int *stats, ogc_stream_t stream) {
    const char *name = "ogc_moving_stats";
    OGC_REQUIRE(B >= 0 && total >= 0, "%s: negative size (B = %d, total = %d)", name, B, total);
    OGC_REQUIRE(n_ignore >= 0, "%s: n_ignore = %d, must not be negative", name, n_ignore);
    OGC_REQUIRE(ignore_npoint_thresh >= 0, "%s: ignore_npoint_thresh = %d, must not be negative", name, ignore_npoint_thresh);
    OGC_REQUIRE(isfinite(ground_y), "%s: ground_y = %g, need a finite value", name, ground_y);
    OGC_REQUIRE(isfinite(moving_thresh) && moving_thresh >= 0.0, "%s: moving_thresh = %g, need a finite value >= 0", name, moving_thresh);
    if (B == 0) return OGC_OK;
    OGC_REQUIRE(offsets && motion && stats, "%s: null pointer (offsets, motion or stats)", name);
    OGC_REQUIRE(total == 0 || (pc && flow && segm && semantic_segm), "%s: null pointer (pc, flow, segm or semantic_segm)", name);
    OGC_REQUIRE(n_ignore == 0 || ignore_class_ids != nullptr, "%s: null pointer (ignore_class_ids)", name);
    hipLaunchKernelGGL(moving_stats_kernel, dim3((unsigned)B), dim3(MS_THREADS), 0, (hipStream_t)stream, total, offsets, pc, flow, segm,
                       semantic_segm, motion, ignore_class_ids, n_ignore, ignore_npoint_thresh, (float)ground_y, moving_thresh, stats);
    OGC_CHECK_LAUNCH(name);
    return OGC_OK;
}

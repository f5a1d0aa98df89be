// seg_eval.hip — everything the segmentation evaluation needs from a batch of soft masks except the assignment, in ONE launch
// (the reference's metrics/seg_metric.py: eval_segm :38-93 and ClusteringMetrics :181-243, numpy loops on the host per sample).
//
// One workgroup per sample, n rounded up to whole waves, 1024 threads at most.  All results are functions of one small table,
// tab[g][p] = points with GT label g and arg-max slot p, indexed by the RAW label (absent labels are empty rows; neither the
// maximum over kept rows nor their number depends on label ranks), plus at most k conditional sums of mask values.
//
//   pass 1     a thread owns points tid, tid + blockDim, ...: arg-max of the mask row (first maximum; a NaN is the maximum and the
//              first NaN wins, as torch.argmax / numpy.argmax), label range check, one integer LDS atomic into the table, `hard`.
//   wave 0     (64 threads: one per label, then one per slot) sizes, ignore / keep / valid flags, the source slot of every
//              column, the Rand-index sums in 64-bit integers; published in LDS.
//   all        counts, pred_iou (fp64 on exact integers), the float32 score matrix of the clustering metrics.
//   pass 2     the confidence sums: for column c every thread adds mask[i, c] over its own points with hard[i] == source[c] in
//              fp64, ascending; shuffle tree inside the wave; wave partials in LDS, added in wave order by thread c.  No
//              floating-point atomics anywhere: the integer sums are order-independent, the fp64 ones have a fixed order, so two
//              calls give identical bits.
//
// A sample that holds a label outside [0, OGC_SEG_EVAL_MAX_LABELS) only sets its status bits in pass 1 (nothing is indexed with
// such a label) and has every other output zeroed; the decision is one LDS word read by all threads after a barrier.
// Private arrays are not indexed at run time: per-label and per-slot values live in LDS.
//
// ogc_seg_eval_ignore is the same kernel with the template parameter IGN: a point whose `ignore` word is non-zero is
// counted in ign[slot] instead of the table and its label is never read; per slot psize = sum_g tab + ign and the ignored area
// is ign + the dropped rows' points.  Everything after pass 1 follows from those two numbers as before, and the confidence pass
// still sums over every point of the source slot.  With IGN = false nothing of this is compiled in.
#include <math.h>

#include "ogc_common.h"

namespace {

constexpr int SE_THREADS = 1024;
constexpr int SE_WAVES = SE_THREADS / OGC_WAVE;
constexpr int SE_L = OGC_SEG_EVAL_MAX_LABELS; // table rows; also the side of the score matrix (the LSAP kernel's limit)
static_assert(SE_L == OGC_WAVE, "wave 0 holds one label, then one slot, per lane");

struct SegEvalShared {
    alignas(16) int tab[SE_L * SE_L];  // [g * k + p]
    double part[SE_L][SE_WAVES];       // wave partials of the confidence sum of column c
    int gsize[SE_L];                   // points of label g
    int psize[SE_L];                   // points of slot p
    int kept[SE_L];                    // psize minus the points inside ignored (= dropped, non-empty) GT objects
    int source[SE_L];                  // the slot whose points column c is averaged over
    int ign[SE_L];                     // IGN: points of slot p that the caller's mask ignores (they are in no row of tab)
    unsigned char keep[SE_L];          // label present and not ignored
    unsigned char dropped[SE_L];       // thresh > 0 and size < thresh: the row leaves the clustering table
    int status;
};

template <typename T>
__device__ __forceinline__ T se_wave_sum(T v) {
#pragma unroll
    for (int off = OGC_WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, OGC_WAVE);
    return v; // lane 0 holds the sum
}

// first maximum of the row so far; a NaN is the maximum and stays
__device__ __forceinline__ void se_argmax_step(float v, int p, float &best, int &at) {
    if (best == best && (v > best || v != v)) {
        best = v;
        at = p;
    }
}

template <bool VEC4>
__device__ __forceinline__ int se_argmax(const float *__restrict__ row, int k) {
    float best;
    int at = 0;
    if (VEC4) {
        const float4 *r4 = reinterpret_cast<const float4 *>(row);
        float4 v = r4[0];
        best = v.x;
        se_argmax_step(v.y, 1, best, at);
        se_argmax_step(v.z, 2, best, at);
        se_argmax_step(v.w, 3, best, at);
        for (int q = 1; q < (k >> 2); ++q) {
            v = r4[q];
            se_argmax_step(v.x, 4 * q, best, at);
            se_argmax_step(v.y, 4 * q + 1, best, at);
            se_argmax_step(v.z, 4 * q + 2, best, at);
            se_argmax_step(v.w, 4 * q + 3, best, at);
        }
    } else {
        best = row[0];
        for (int p = 1; p < k; ++p) se_argmax_step(row[p], p, best, at);
    }
    return at;
}

template <bool VEC4, bool IGN>
__global__ __launch_bounds__(SE_THREADS) void seg_eval_kernel(int n, int k, int thresh, const int *__restrict__ segm_all,
                                                              const float *__restrict__ mask_all,
                                                              const int *__restrict__ ignore_all, int *hard_all,
                                                              int *__restrict__ counts_all, int *__restrict__ ignored_all,
                                                              double *__restrict__ pred_iou_all,
                                                              double *__restrict__ confidence_all, int *__restrict__ valid_all,
                                                              int *__restrict__ n_gt_all, float *__restrict__ score_all,
                                                              int *__restrict__ rows_all, double *__restrict__ ri_all,
                                                              int *__restrict__ status_all) {
    __shared__ SegEvalShared sh;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int lane = tid & (OGC_WAVE - 1), wave = tid / OGC_WAVE, nwaves = nt / OGC_WAVE;
    const size_t b = blockIdx.x;
    const int *segm = segm_all + b * n;
    const float *mask = mask_all + b * n * k;
    int *hard = hard_all + b * n;
    int *counts = counts_all + b * SE_L * k;
    float *score = score_all + b * SE_L * SE_L;
    const int cells = SE_L * k;

    for (int e = tid; e < cells; e += nt) sh.tab[e] = 0;
    if (IGN && tid < SE_L) sh.ign[tid] = 0;
    if (tid == 0) sh.status = 0;
    __syncthreads();

    // pass 1
    for (int i = tid; i < n; i += nt) {
        const int at = se_argmax<VEC4>(mask + (size_t)i * k, k);
        hard[i] = at;
        if (IGN && ignore_all[b * n + i] != 0) {
            atomicAdd(&sh.ign[at], 1); // the label of an ignored point is not read
            continue;
        }
        const int g = segm[i];
        if (g < 0) atomicOr(&sh.status, 2);
        else if (g >= SE_L) atomicOr(&sh.status, 1);
        else atomicAdd(&sh.tab[g * k + at], 1);
    }
    __syncthreads();

    const int status = sh.status; // uniform over the workgroup
    if (status != 0) {
        for (int i = tid; i < n; i += nt) hard[i] = 0;
        for (int e = tid; e < cells; e += nt) counts[e] = 0;
        for (int e = tid; e < SE_L * SE_L; e += nt) score[e] = 0.f;
        if (tid < k) {
            pred_iou_all[b * k + tid] = 0.0;
            confidence_all[b * k + tid] = 0.0;
            valid_all[b * k + tid] = 0;
            if (IGN) ignored_all[b * k + tid] = 0;
        }
        if (tid == 0) {
            n_gt_all[b] = 0;
            rows_all[b] = 0;
            ri_all[b] = 0.0;
            status_all[b] = status;
        }
        return;
    }

    // wave 0, lane = label g
    long long n_v = 0, sum_a2 = 0;
    if (tid < SE_L) {
        int gs = 0;
        for (int q = 0; q < k; ++q) {
            const int p = (q + tid) % k; // a rotated start spreads the lanes over the banks
            gs += sh.tab[tid * k + p];
        }
        const bool dropped = thresh > 0 && gs < thresh;
        const bool keep = gs > 0 && !dropped;
        sh.gsize[tid] = gs;
        sh.keep[tid] = keep;
        sh.dropped[tid] = dropped;
        const unsigned long long present_m = __ballot(gs > 0), keep_m = __ballot(keep), dropped_m = __ballot(dropped);
        const int n_gt_segm = present_m ? 64 - __clzll((long long)present_m) : 0; // largest label + 1
        const unsigned long long below = n_gt_segm >= 64 ? ~0ull : ((1ull << n_gt_segm) - 1ull);
        const long long a = dropped ? 0 : gs;
        n_v = se_wave_sum(a);
        sum_a2 = se_wave_sum(a * a);
        if (tid == 0) {
            n_gt_all[b] = __popcll(keep_m);
            rows_all[b] = __popcll(~dropped_m & below);
            status_all[b] = 0;
        }
    }
    __syncthreads();

    // wave 0, lane = slot p
    if (tid < SE_L) {
        int ps = 0, ignored = 0;
        long long m2 = 0;
        if (tid < k) {
            for (int g = 0; g < SE_L; ++g) {
                const int m = sh.tab[g * k + tid];
                ps += m;
                if (sh.dropped[g]) ignored += m; // empty rows add nothing: dropped and ignored rows hold the same points
                else m2 += (long long)m * m;
            }
            if (IGN) {
                const int ig = sh.ign[tid];
                ps += ig;
                ignored += ig;
                ignored_all[b * k + tid] = ig;
            }
        }
        const int kept = ps - ignored;
        const bool present = ps > 0;
        const bool invalid = 2ll * ignored > (long long)ps; // ignored / ps > 0.5 on exact integers
        const bool valid = present && kept > 0 && !invalid;
        const unsigned long long valid_m = __ballot(valid), present_m = __ballot(present);
        // position among the valid slots -> that many present slots are skipped (the reference's column shift)
        const unsigned long long upto = tid >= 63 ? ~0ull : ((2ull << tid) - 1ull);
        int skip = __popcll(valid_m & upto) - 1;
        skip = skip < 0 ? 0 : skip;
        unsigned long long rest = present_m;
        for (int j = 0; j < skip; ++j) rest &= rest - 1ull;
        const int src = rest ? __ffsll((long long)rest) - 1 : tid; // rest != 0: valid slots are present ones
        sh.psize[tid] = ps;
        sh.kept[tid] = kept;
        sh.source[tid] = src < k ? src : 0;
        if (tid < k) valid_all[b * k + tid] = valid ? 1 : 0;
        const long long sum_b2 = se_wave_sum((long long)kept * kept);
        const long long sum_m2 = se_wave_sum(m2);
        if (tid == 0) {
            const long long pairs = n_v * n_v;
            ri_all[b] = n_v ? (double)(pairs - sum_a2 - sum_b2 + 2 * sum_m2) / (double)pairs : (double)NAN;
        }
    }
    __syncthreads();

    for (int e = tid; e < cells; e += nt) counts[e] = sh.tab[e];

    if (tid < k) {
        double best = 0.0;
        const int kept = sh.kept[tid];
        for (int g = 0; g < SE_L; ++g) {
            if (!sh.keep[g]) continue;
            const int inter = sh.tab[g * k + tid];
            const int uni = sh.gsize[g] + kept - inter; // > 0: a kept row is not empty
            best = fmax(best, (double)inter / (double)uni);
        }
        pred_iou_all[b * k + tid] = best;
    }

    // m / ((a_g + b_p - m) + 1e-8f) in float32, one rounding per operation
    for (int e = tid; e < SE_L * SE_L; e += nt) {
        const int g = e / SE_L, p = e % SE_L;
        float s = 0.f;
        if (p < k && !sh.dropped[g]) {
            const float m = (float)sh.tab[g * k + p];
            const float uni = __fsub_rn(__fadd_rn((float)sh.gsize[g], (float)sh.kept[p]), m);
            s = __fdiv_rn(m, __fadd_rn(uni, 1e-8f));
        }
        score[e] = s;
    }

    // pass 2
    for (int c = 0; c < k; ++c) {
        const int src = sh.source[c];
        if (sh.psize[src] == 0) continue; // uniform
        double acc = 0.0;
        for (int i = tid; i < n; i += nt)
            if (hard[i] == src) acc += (double)mask[(size_t)i * k + c];
        acc = se_wave_sum(acc);
        if (lane == 0) sh.part[c][wave] = acc;
    }
    __syncthreads();
    if (tid < k) {
        const int ps = sh.psize[sh.source[tid]];
        double total = 0.0;
        if (ps > 0) {
            total = sh.part[tid][0];
            for (int w = 1; w < nwaves; ++w) total += sh.part[tid][w];
        }
        confidence_all[b * k + tid] = total / (double)(ps > 1 ? ps : 1);
    }
}

// the argument checks and the launch of both entry points; `ignore` and `ignored` are null exactly when IGN is false
template <bool IGN>
int seg_eval_launch(const char *name, int B, int n, int k, const int *segm, const float *mask, const int *ignore,
                    int ignore_npoint_thresh, int *hard, int *counts, int *ignored, double *pred_iou, double *confidence,
                    int *valid, int *n_gt, float *score, int *rows, double *ri, int *status, ogc_stream_t stream) {
    OGC_REQUIRE(B >= 0, "%s: negative batch", name);
    if (B == 0) return OGC_OK;
    OGC_REQUIRE(n >= 1, "%s: n = %d, need at least one point per sample", name, n);
    OGC_REQUIRE(k >= 1 && k <= OGC_SEG_EVAL_MAX_LABELS, "%s: k = %d, need 1 <= k <= %d slots", name, k, OGC_SEG_EVAL_MAX_LABELS);
    OGC_REQUIRE(ignore_npoint_thresh >= 0, "%s: ignore_npoint_thresh = %d is negative", name, ignore_npoint_thresh);
    OGC_REQUIRE(segm && mask && hard && counts && pred_iou && confidence && valid && n_gt && score && rows && ri && status,
                "%s: null pointer", name);
    OGC_REQUIRE(!IGN || (ignore && ignored), "%s: null pointer (ignore / ignored)", name);
    const int threads = min(SE_THREADS, ogc_divup(n, OGC_WAVE) * OGC_WAVE);
    const bool vec4 = (k & 3) == 0 && ((uintptr_t)mask & 15) == 0; // every row starts on a 16-byte boundary
#define OGC_SEG_EVAL_LAUNCH(VEC4)                                                                                                \
    hipLaunchKernelGGL((seg_eval_kernel<VEC4, IGN>), dim3(B), dim3(threads), 0, (hipStream_t)stream, n, k, ignore_npoint_thresh, \
                       segm, mask, ignore, hard, counts, ignored, pred_iou, confidence, valid, n_gt, score, rows, ri, status)
    if (vec4) OGC_SEG_EVAL_LAUNCH(true);
    else OGC_SEG_EVAL_LAUNCH(false);
#undef OGC_SEG_EVAL_LAUNCH
    OGC_CHECK_LAUNCH(name);
    return OGC_OK;
}

} // namespace

extern "C" int ogc_seg_eval(int B, int n, int k, const int *segm, const float *mask, int ignore_npoint_thresh, int *hard,
                            int *counts, double *pred_iou, double *confidence, int *valid, int *n_gt, float *score, int *rows,
                            double *ri, int *status, ogc_stream_t stream) {
    return seg_eval_launch<false>("ogc_seg_eval", B, n, k, segm, mask, nullptr, ignore_npoint_thresh, hard, counts, nullptr,
                                  pred_iou, confidence, valid, n_gt, score, rows, ri, status, stream);
}

extern "C" int ogc_seg_eval_ignore(int B, int n, int k, const int *segm, const float *mask, const int *ignore,
                                   int ignore_npoint_thresh, int *hard, int *counts, int *ignored, double *pred_iou,
                                   double *confidence, int *valid, int *n_gt, float *score, int *rows, double *ri, int *status,
                                   ogc_stream_t stream) {
    return seg_eval_launch<true>("ogc_seg_eval_ignore", B, n, k, segm, mask, ignore, ignore_npoint_thresh, hard, counts, ignored,
                                 pred_iou, confidence, valid, n_gt, score, rows, ri, status, stream);
}

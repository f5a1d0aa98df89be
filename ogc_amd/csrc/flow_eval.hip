// flow_eval.hip — the scene-flow metrics of a batch in ONE launch (the reference's metrics/flow_metric.py:16-24: two norms, a
// ratio, three pairs of comparisons and four means, about fifteen framework launches on tensors copied to the host first).
//
// Per sample: epe_sum = the fp64 sum of the end-point errors, counts = {strict-accurate, relaxed-accurate, outlier} points.
// The caller divides (metrics/flow_eval.py), per sample or over the batch.
//
//   geometry   G * B workgroups of 256 threads: workgroup g of sample b owns a contiguous run of GROUPS of four points; thread t takes
//              the groups lo + t, lo + t + 256, ...  Groups are cut on multiples of four of the GLOBAL point index b * N + i, so
//              that a whole group is 48 bytes starting on a 16-byte boundary — three float4 loads per tensor and lane — also in
//              the samples whose base is not aligned (N % 4 != 0): those start with a short group.  Short groups, and every
//              group when a base pointer is not 16-byte aligned, take the scalar path; both paths visit the points in the same
//              order, so the result does not depend on which one ran.
//   per point  fp32, one rounding per operation, nothing contracted (the library is built with -ffp-contract=off).
//   sums       counts in integers; the error in fp64: a thread adds its points in ascending order, a shuffle tree adds the lanes,
//              thread 0 adds the four wave sums in wave order — the workgroup's partial.  With G == 1 that is the result.
//              With G > 1 every workgroup publishes its partial in a slot of a static table and takes a ticket of its sample;
//              the workgroup that draws the last ticket adds the G partials in slot order (lane l of its first wave the slots
//              l, l + 64, ... ascending, then the same shuffle tree) and writes the outputs.  Which workgroup finishes depends
//              on timing; what it computes does not: no floating-point atomics, a fixed order, identical bits from call to call.
//   hand-off   partials and tickets are agent-scope atomics (gfx950: eight XCDs with private L2s, a CU's L1 is never refreshed
//              by other CUs' stores): relaxed write-through stores of the partial, an acq_rel ticket add behind them, relaxed
//              agent-scope loads in the finisher.  Nobody waits for anybody: there is no spin, hence no residency assumption.
//   state      the table is static device memory, zero when the module is loaded; the finisher puts its sample's ticket back
//              to zero.  So a call allocates nothing, zeroes nothing, and is ONE kernel launch (capturable).  The price: calls
//              with G > 1 that OVERLAP IN TIME on different streams of one device would share the table; launch this entry
//              point from one stream per device at a time (stream order is all the kernel needs between calls).
#include <math.h>

#include "ogc_common.h"

namespace {

constexpr int FE_THREADS = 256;
constexpr int FE_WAVES = FE_THREADS / OGC_WAVE;
constexpr int FE_SLOTS = 4096;  // partials of one call: B * G <= FE_SLOTS whenever G > 1
constexpr int FE_MAX_G = 1024;

__device__ double fe_part_epe[FE_SLOTS];
__device__ unsigned long long fe_part_cnt[FE_SLOTS][2]; // {strict | relaxed << 32, outlier}
__device__ unsigned fe_ticket[FE_SLOTS];                 // per sample; zero between calls

struct FlowEvalAcc {
    double epe;
    int strict, relaxed, outlier;
};

struct FlowEvalThresholds {
    float t1, t2, t6, eps;
};

template <typename T>
__device__ __forceinline__ T fe_wave_sum(T v) {
#pragma unroll
    for (int off = OGC_WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, OGC_WAVE);
    return v; // lane 0 holds the sum
}

__device__ __forceinline__ void fe_point(float gx, float gy, float gz, float px, float py, float pz, const FlowEvalThresholds &th,
                                         FlowEvalAcc &acc) {
    const float dx = px - gx, dy = py - gy, dz = pz - gz;
    const float e = sqrtf((dx * dx + dy * dy) + dz * dz);
    const float s = sqrtf((gx * gx + gy * gy) + gz * gz);
    const float r = e / (s + th.eps);
    acc.epe += (double)e;                                 // a NaN stays in its own sample's sum
    acc.strict += (e < th.t1 || r < 0.05f) ? 1 : 0;       // a NaN satisfies no comparison
    acc.relaxed += (e < th.t2 || r < 0.1f) ? 1 : 0;
    acc.outlier += (e > th.t6 || r > 0.1f) ? 1 : 0;
}

__global__ __launch_bounds__(FE_THREADS) void flow_eval_kernel(int n, int G, int groups_per_wg, int vec_ok, const float *__restrict__ gt_all,
                                                               const float *__restrict__ pred_all, FlowEvalThresholds th,
                                                               double *__restrict__ epe_sum, int *__restrict__ counts) {
    __shared__ double sh_epe[FE_WAVES];
    __shared__ int sh_cnt[FE_WAVES][3];
    const int tid = threadIdx.x, lane = tid & (OGC_WAVE - 1), wave = tid / OGC_WAVE;
    const int g = (int)(blockIdx.x % (unsigned)G);
    const size_t b = blockIdx.x / (unsigned)G;
    const size_t first = b * (size_t)n;                  // global index of the sample's point 0
    const int off = (int)(first & 3);                    // group j holds the sample's points 4j - off .. 4j - off + 3
    const int ngroups = (int)(((long long)n + off + 3) >> 2);
    const long long lo_ll = (long long)g * groups_per_wg;
    const int lo = (int)(lo_ll < ngroups ? lo_ll : ngroups);
    const int hi = (int)(lo_ll + groups_per_wg < ngroups ? lo_ll + groups_per_wg : ngroups);
    const float *gt = gt_all + first * 3, *pred = pred_all + first * 3;

    FlowEvalAcc acc = {0.0, 0, 0, 0};
    for (int j = lo + tid; j < hi; j += FE_THREADS) {
        const long long p0 = 4ll * j - off;              // may be negative in group 0, and p0 + 3 may pass n in the last one
        if (vec_ok && p0 >= 0 && p0 + 4 <= n) {
            const float4 *g4 = reinterpret_cast<const float4 *>(gt + p0 * 3);
            const float4 *p4 = reinterpret_cast<const float4 *>(pred + p0 * 3);
            const float4 ga = g4[0], gb = g4[1], gc = g4[2];
            const float4 pa = p4[0], pb = p4[1], pc = p4[2];
            fe_point(ga.x, ga.y, ga.z, pa.x, pa.y, pa.z, th, acc);
            fe_point(ga.w, gb.x, gb.y, pa.w, pb.x, pb.y, th, acc);
            fe_point(gb.z, gb.w, gc.x, pb.z, pb.w, pc.x, th, acc);
            fe_point(gc.y, gc.z, gc.w, pc.y, pc.z, pc.w, th, acc);
        } else {
            for (int u = 0; u < 4; ++u) {
                const long long p = p0 + u;
                if (p < 0 || p >= n) continue;
                const float *gq = gt + p * 3, *pq = pred + p * 3;
                fe_point(gq[0], gq[1], gq[2], pq[0], pq[1], pq[2], th, acc);
            }
        }
    }

    acc.epe = fe_wave_sum(acc.epe);
    acc.strict = fe_wave_sum(acc.strict);
    acc.relaxed = fe_wave_sum(acc.relaxed);
    acc.outlier = fe_wave_sum(acc.outlier);
    if (lane == 0) {
        sh_epe[wave] = acc.epe;
        sh_cnt[wave][0] = acc.strict;
        sh_cnt[wave][1] = acc.relaxed;
        sh_cnt[wave][2] = acc.outlier;
    }
    __syncthreads();
    if (wave != 0) return;

    int last = 0;
    if (tid == 0) {
        for (int w = 1; w < FE_WAVES; ++w) {
            acc.epe += sh_epe[w];
            acc.strict += sh_cnt[w][0];
            acc.relaxed += sh_cnt[w][1];
            acc.outlier += sh_cnt[w][2];
        }
        if (G == 1) {
            epe_sum[b] = acc.epe;
            counts[b * 3 + 0] = acc.strict;
            counts[b * 3 + 1] = acc.relaxed;
            counts[b * 3 + 2] = acc.outlier;
        } else {
            const size_t slot = b * G + g;
            __hip_atomic_store(reinterpret_cast<unsigned long long *>(&fe_part_epe[slot]),
                               (unsigned long long)__double_as_longlong(acc.epe), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&fe_part_cnt[slot][0], (unsigned long long)(unsigned)acc.strict | ((unsigned long long)(unsigned)acc.relaxed << 32),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&fe_part_cnt[slot][1], (unsigned long long)(unsigned)acc.outlier, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
            // release: the partial is visible to whoever sees this ticket; acquire: the finisher sees everybody's
            const unsigned drawn = __hip_atomic_fetch_add(&fe_ticket[b], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
            last = drawn == (unsigned)(G - 1);
        }
    }
    if (!__shfl(last, 0, OGC_WAVE)) return;

    // the finisher: G partials in slot order
    FlowEvalAcc tot = {0.0, 0, 0, 0};
    for (int s = lane; s < G; s += OGC_WAVE) {
        const size_t slot = b * G + s;
        const unsigned long long e = __hip_atomic_load(reinterpret_cast<unsigned long long *>(&fe_part_epe[slot]), __ATOMIC_RELAXED,
                                                       __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long c0 = __hip_atomic_load(&fe_part_cnt[slot][0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long c1 = __hip_atomic_load(&fe_part_cnt[slot][1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        tot.epe += __longlong_as_double((long long)e);
        tot.strict += (int)(unsigned)c0;
        tot.relaxed += (int)(unsigned)(c0 >> 32);
        tot.outlier += (int)(unsigned)c1;
    }
    tot.epe = fe_wave_sum(tot.epe);
    tot.strict = fe_wave_sum(tot.strict);
    tot.relaxed = fe_wave_sum(tot.relaxed);
    tot.outlier = fe_wave_sum(tot.outlier);
    if (tid == 0) {
        epe_sum[b] = tot.epe;
        counts[b * 3 + 0] = tot.strict;
        counts[b * 3 + 1] = tot.relaxed;
        counts[b * 3 + 2] = tot.outlier;
        __hip_atomic_store(&fe_ticket[b], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // for the next call on the stream
    }
}

} // namespace

extern "C" int ogc_flow_eval(int B, int N, const float *gt_flow, const float *flow_pred, double epe_norm_thresh, double eps,
                             double *epe_sum, int *counts, ogc_stream_t stream) {
    OGC_REQUIRE(B >= 0, "ogc_flow_eval: negative batch");
    if (B == 0) return OGC_OK;
    OGC_REQUIRE(N >= 1, "ogc_flow_eval: N = %d, need at least one point per sample", N);
    OGC_REQUIRE(isfinite(epe_norm_thresh) && epe_norm_thresh > 0.0, "ogc_flow_eval: epe_norm_thresh = %g, need a finite value > 0",
                epe_norm_thresh);
    OGC_REQUIRE(isfinite(eps) && eps >= 0.0, "ogc_flow_eval: eps = %g, need a finite value >= 0", eps);
    OGC_REQUIRE(gt_flow && flow_pred && epe_sum && counts, "ogc_flow_eval: null pointer");
    // a function of (B, N) alone: the order of the fp64 sum must not change from call to call
    const long long max_groups = ((long long)N + 3 + 3) >> 2; // the sample with the longest head
    long long G = (max_groups + FE_THREADS - 1) / FE_THREADS;
    if (G > FE_MAX_G) G = FE_MAX_G;
    if (G * B > FE_SLOTS) G = FE_SLOTS / B;
    if (G < 1) G = 1;
    const long long groups_per_wg = (max_groups + G - 1) / G;
    G = (max_groups + groups_per_wg - 1) / groups_per_wg;      // no workgroup without a group
    const int vec_ok = (((uintptr_t)gt_flow | (uintptr_t)flow_pred) & 15) == 0;
    const FlowEvalThresholds th = {(float)epe_norm_thresh, (float)(2 * epe_norm_thresh), (float)(6 * epe_norm_thresh), (float)eps};
    hipLaunchKernelGGL(flow_eval_kernel, dim3((unsigned)(G * B)), dim3(FE_THREADS), 0, (hipStream_t)stream, N, (int)G,
                       (int)groups_per_wg, vec_ok, gt_flow, flow_pred, th, epe_sum, counts);
    OGC_CHECK_LAUNCH("ogc_flow_eval");
    return OGC_OK;
}

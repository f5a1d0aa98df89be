// seg_conf.hip — the confidences of a batch of PREDICTED segmentations in ONE launch: per sample the arg-max labels, the slots
// that own a point in the order compress_label_id numbers them, their sizes and the mean of each slot's own mask value over its
// own points (the reference's metrics/seg_metric.py:81-85 for a prediction, without that function's validity filter and column
// shift).  No ground truth is read: this is what a self-training round saves beside segm.npy.
//
//   geometry   G * B workgroups of 256 threads; workgroup g of sample b owns tiles_per_wg consecutive TILES of
//              OGC_SLOT_CONF_TILE points (one tile unless the static table below would overflow).
//   pass 1     per tile, a thread takes the points tid, tid + 256, ...: arg-max of the mask row by the rule of seg_eval.hip (first
//              maximum; a NaN is the maximum and the first NaN wins — sc_argmax_step is se_argmax_step, and a test holds the two
//              kernels' `hard` together), writes `hard`, and leaves the slot and the maximum itself, which IS mask[p, slot], in LDS.
//   pass 2     per tile, wave w takes the slots w, w + 4, ...: lane l adds the tile's points l, l + 64, ... of that slot, ascending,
//              in fp64, and counts them; a shuffle tree adds the lanes; lane 0 adds the tile's sum to the workgroup's partial of
//              the slot in LDS (tiles ascending).  Per-slot values live in LDS, not in run-time indexed private arrays (§4d).
//   finish     G == 1: the partial is the result.  G > 1: wave 0 (lane = slot) publishes the partial in a row of a static table
//              and takes a ticket of its sample; the workgroup that draws the last ticket adds the G rows in ascending order and
//              writes the outputs.  Which workgroup finishes depends on timing; what it computes does not: no floating-point
//              atomics, a fixed order, identical bits from call to call.  With one tile per workgroup the order depends on n
//              alone, so a sample's bits do not depend on the batch it sits in.
//   hand-off   as flow_eval.hip: relaxed agent-scope (write-through) stores of the partial, drained by the storing wave, an
//              acq_rel ticket add by its lane 0 behind them, relaxed agent-scope loads in the finisher, which is the same wave
//              of the last workgroup.  Nobody waits for anybody: no spin, no residency assumption.  As there, the ordering of the
//              OTHER lanes' stores before lane 0's ticket rests on the hardware — a wave's stores are drained by its own
//              s_waitcnt vmcnt(0), which is per wave, not per lane — and not on the formal memory model, in which a release by
//              lane 0 orders lane 0's accesses only.
//   state      the table is static device memory, zero when the module is loaded; the finisher puts its sample's ticket back to
//              zero.  So a call allocates nothing, zeroes nothing, and is ONE kernel launch (capturable).  The price: calls with
//              G > 1 that OVERLAP IN TIME on different streams of one device would share the table.
#include <math.h>

#include "ogc_common.h"

namespace {

constexpr int SC_THREADS = 256;
constexpr int SC_WAVES = SC_THREADS / OGC_WAVE;
constexpr int SC_TILE = OGC_SLOT_CONF_TILE;
constexpr int SC_K = OGC_SLOT_CONF_MAX_K;
constexpr int SC_ROWS = OGC_SLOT_CONF_MAX_PARTIALS; // workgroup partials of one call: B * G <= SC_ROWS whenever G > 1
static_assert(SC_K == OGC_WAVE, "the finish holds one slot per lane of one wave");
static_assert(SC_K <= 256, "a point's slot is kept in one byte");

__device__ double sc_part_sum[SC_ROWS][SC_K];
__device__ int sc_part_cnt[SC_ROWS][SC_K];
__device__ unsigned sc_ticket[SC_ROWS]; // per sample; zero between calls

constexpr int SC_FINISH_ROWS = 16; // rows of the table whose loads the finisher keeps in flight together

__device__ __forceinline__ void sc_load_partial(size_t row, int slot, double &sum, int &cnt) {
    const unsigned long long e = __hip_atomic_load(reinterpret_cast<unsigned long long *>(&sc_part_sum[row][slot]),
                                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sum = __longlong_as_double((long long)e);
    cnt = __hip_atomic_load(&sc_part_cnt[row][slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct SlotConfShared {
    double sum[SC_K];          // the workgroup's partial of slot c
    int cnt[SC_K];
    float val[SC_TILE];        // of the tile's point j: the maximum of its row
    unsigned char at[SC_TILE]; // and the slot that holds it
};

template <typename T>
__device__ __forceinline__ T sc_wave_sum(T v) {
#pragma unroll
    for (int off = OGC_WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, OGC_WAVE);
    return v; // lane 0 holds the sum
}

// first maximum of the row so far; a NaN is the maximum and stays
__device__ __forceinline__ void sc_argmax_step(float v, int p, float &best, int &at) {
    if (best == best && (v > best || v != v)) {
        best = v;
        at = p;
    }
}

template <bool VEC4>
__device__ __forceinline__ int sc_argmax(const float *__restrict__ row, int k, float &best) {
    int at = 0;
    if (VEC4) {
        const float4 *r4 = reinterpret_cast<const float4 *>(row);
        float4 v = r4[0];
        best = v.x;
        sc_argmax_step(v.y, 1, best, at);
        sc_argmax_step(v.z, 2, best, at);
        sc_argmax_step(v.w, 3, best, at);
        for (int q = 1; q < (k >> 2); ++q) {
            v = r4[q];
            sc_argmax_step(v.x, 4 * q, best, at);
            sc_argmax_step(v.y, 4 * q + 1, best, at);
            sc_argmax_step(v.z, 4 * q + 2, best, at);
            sc_argmax_step(v.w, 4 * q + 3, best, at);
        }
    } else {
        best = row[0];
        for (int p = 1; p < k; ++p) sc_argmax_step(row[p], p, best, at);
    }
    return at;
}

template <bool VEC4>
__global__ __launch_bounds__(SC_THREADS) void slot_confidence_kernel(int n, int k, int G, int tiles_per_wg,
                                                                     const float *__restrict__ mask_all, int *hard_all,
                                                                     int *__restrict__ slots_all, int *__restrict__ sizes_all,
                                                                     float *__restrict__ conf_all, int *__restrict__ n_object_all) {
    __shared__ SlotConfShared sh;
    const int tid = threadIdx.x, lane = tid & (OGC_WAVE - 1), wave = tid / OGC_WAVE;
    const int g = (int)(blockIdx.x % (unsigned)G);
    const size_t b = blockIdx.x / (unsigned)G;
    const float *mask = mask_all + b * (size_t)n * k;
    int *hard = hard_all ? hard_all + b * (size_t)n : nullptr;

    if (tid < SC_K) { // first touched again behind the barrier of pass 1
        sh.sum[tid] = 0.0;
        sh.cnt[tid] = 0;
    }
    for (int t = 0; t < tiles_per_wg; ++t) {
        const long long lo = ((long long)g * tiles_per_wg + t) * SC_TILE;
        if (lo >= n) break; // uniform
        const int cnt = (int)(n - lo < SC_TILE ? n - lo : SC_TILE);
        for (int j = tid; j < cnt; j += SC_THREADS) {
            float best;
            const int at = sc_argmax<VEC4>(mask + (size_t)(lo + j) * k, k, best);
            if (hard) hard[lo + j] = at;
            sh.val[j] = best;
            sh.at[j] = (unsigned char)at;
        }
        __syncthreads();
        for (int c = wave; c < k; c += SC_WAVES) {
            double s = 0.0;
            int m = 0;
            for (int j = lane; j < cnt; j += OGC_WAVE)
                if (sh.at[j] == c) {
                    s += (double)sh.val[j];
                    ++m;
                }
            s = sc_wave_sum(s);
            m = sc_wave_sum(m);
            if (lane == 0) { // slot c belongs to this wave in every tile
                sh.sum[c] += s;
                sh.cnt[c] += m;
            }
        }
        __syncthreads(); // val / at are free for the next tile; after the last one, sum / cnt are complete
    }
    if (wave != 0) return;

    // wave 0, lane = slot
    double s = lane < k ? sh.sum[lane] : 0.0;
    int m = lane < k ? sh.cnt[lane] : 0;
    if (G > 1) {
        const size_t row = b * G + g;
        if (lane < k) {
            __hip_atomic_store(reinterpret_cast<unsigned long long *>(&sc_part_sum[row][lane]),
                               (unsigned long long)__double_as_longlong(s), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&sc_part_cnt[row][lane], m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the storing wave drains before its lane 0 signals
        int last = 0;
        if (lane == 0) {
            // release: the partial is visible to whoever sees this ticket; acquire: the finisher sees everybody's
            const unsigned drawn = __hip_atomic_fetch_add(&sc_ticket[b], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
            last = drawn == (unsigned)(G - 1);
        }
        if (!__shfl(last, 0, OGC_WAVE)) return;

        // the finisher: G partials in row order, the loads of SC_FINISH_ROWS rows in flight together
        s = 0.0;
        m = 0;
        if (lane < k) {
            const size_t first = b * G;
            int r = 0;
            for (; r + SC_FINISH_ROWS <= G; r += SC_FINISH_ROWS) {
                double e[SC_FINISH_ROWS];
                int c[SC_FINISH_ROWS];
#pragma unroll
                for (int u = 0; u < SC_FINISH_ROWS; ++u) sc_load_partial(first + r + u, lane, e[u], c[u]);
#pragma unroll
                for (int u = 0; u < SC_FINISH_ROWS; ++u) {
                    s += e[u];
                    m += c[u];
                }
            }
            for (; r < G; ++r) {
                double e;
                int c;
                sc_load_partial(first + r, lane, e, c);
                s += e;
                m += c;
            }
        }
        if (lane == 0) __hip_atomic_store(&sc_ticket[b], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // for the next call
    }

    const bool present = m > 0; // lanes >= k hold 0
    const unsigned long long present_m = __ballot(present);
    const int n_object = __popcll(present_m);
    int *slots = slots_all + b * k;
    int *sizes = sizes_all + b * k;
    float *conf = conf_all + b * k;
    if (present) {
        const int j = __popcll(present_m & ((1ull << lane) - 1ull)); // present slots below this one
        slots[j] = lane;
        sizes[j] = m;
        conf[j] = (float)(s / (double)m);
    }
    if (lane >= n_object && lane < k) {
        slots[lane] = -1;
        sizes[lane] = 0;
        conf[lane] = 0.f;
    }
    if (lane == 0) n_object_all[b] = n_object;
}

} // namespace

extern "C" int ogc_slot_confidence(int B, int n, int k, const float *mask, int *hard, int *slots, int *sizes, float *conf,
                                   int *n_object, ogc_stream_t stream) {
    OGC_REQUIRE(B >= 0, "ogc_slot_confidence: negative batch");
    if (B == 0) return OGC_OK;
    OGC_REQUIRE(n >= 1, "ogc_slot_confidence: n = %d, need at least one point per sample", n);
    OGC_REQUIRE(k >= 1 && k <= OGC_SLOT_CONF_MAX_K, "ogc_slot_confidence: k = %d, need 1 <= k <= %d slots", k, OGC_SLOT_CONF_MAX_K);
    OGC_REQUIRE(mask && slots && sizes && conf && n_object, "ogc_slot_confidence: null pointer");
    // a function of (B, n) alone: the order of the fp64 sums must not change from call to call
    const long long tiles = ((long long)n + SC_TILE - 1) / SC_TILE;
    long long tiles_per_wg = 1;
    if (tiles > 1 && tiles * B > SC_ROWS) {
        const long long g_max = SC_ROWS / B > 1 ? SC_ROWS / B : 1;
        tiles_per_wg = (tiles + g_max - 1) / g_max;
    }
    const long long G = (tiles + tiles_per_wg - 1) / tiles_per_wg; // no workgroup without a tile; G > 1 implies B * G <= SC_ROWS
    const bool vec4 = (k & 3) == 0 && ((uintptr_t)mask & 15) == 0; // every row starts on a 16-byte boundary
#define OGC_SLOT_CONF_LAUNCH(VEC4)                                                                                          \
    hipLaunchKernelGGL((slot_confidence_kernel<VEC4>), dim3((unsigned)(G * B)), dim3(SC_THREADS), 0, (hipStream_t)stream, n, k, \
                       (int)G, (int)tiles_per_wg, mask, hard, slots, sizes, conf, n_object)
    if (vec4) OGC_SLOT_CONF_LAUNCH(true);
    else OGC_SLOT_CONF_LAUNCH(false);
#undef OGC_SLOT_CONF_LAUNCH
    OGC_CHECK_LAUNCH("ogc_slot_confidence");
    return OGC_OK;
}

// live_steps.hip — the live-step lists of a level's neighbour lists (the rule, the packing of both lists and LiveIn: live_steps.h).
// The list forms that walk them: gn_fused_bwd.hip (backward), conv1x1.hip (forward).
#include "ogc_common.h"
#include "live_steps.h"

namespace {

// One workgroup per sample.  Count: a wavefront reads 64 consecutive entries (64 / S whole rows) per load and finds each row's last
// column that differs from column 0 with a ballot; the centre's live-step count goes to LDS.  Then a run of consecutive centres
// per thread: sum, scan (as rev_scan_kernel of neighbour_loss.hip), write.
// FWD: the forward list as well (live_steps.h; p * s is a multiple of 64).  The greedy pack is a walk over the groups with one
// state, the slots u = 0 .. 3 used in the current tile; a run of groups maps u to the slots it consumes from there, pads included
// (the state after it is (u + that) & 3), and such maps compose — a thread forms the map of its run of consecutive groups, the
// same scan composes them, and the thread writes its run from the offset the runs in front of it consume from state 0.
constexpr int LIVE_MAX_P = 32768; // centres per sample (one byte of LDS each)
template <bool FWD>
__global__ __launch_bounds__(1024) void live_steps_kernel(int p, int s, const int *__restrict__ idx, int *__restrict__ steps,
                                                          int *__restrict__ n_live, int *__restrict__ fwd = nullptr,
                                                          int *__restrict__ n_fwd = nullptr) {
    __shared__ int part[1024];
    __shared__ int fmap[FWD ? 4 * 1024 : 4]; // FWD: [u][thread] slots consumed from state u
    __shared__ unsigned char cnt[LIVE_MAX_P];
    const int t = threadIdx.x, b = blockIdx.x, T = s >> 4;
    const int lane = t & 63, wave = t >> 6;
    const int *ib = idx + (size_t)b * p * s;
    int *out = steps + (size_t)b * p * T;
    const int row0 = lane & ~(s - 1); // the lane of column 0 of this lane's row
    const unsigned long long row_mask = (s == 64 ? ~0ull : (1ull << s) - 1ull) << row0;
    const int total = p * s;          // (< 2^31: p <= LIVE_MAX_P, s <= 64)
    for (int e0 = wave * 64; e0 < total; e0 += 1024) { // (wave-uniform trips; total is a multiple of s, so rows are whole)
        const bool in = e0 + lane < total;
        const int v = in ? ib[e0 + lane] : 0;
        const int first = __shfl(v, row0);
        const unsigned long long differs = __builtin_amdgcn_ballot_w64(in && v != first) & row_mask;
        const int hi = differs ? 63 - __clzll(differs) - row0 : 0; // the last column that differs from column 0 (0: none)
        if (in && lane == row0) cnt[(e0 + lane) / s] = (unsigned char)(min((hi + 1) >> 4, T - 1) + 1); // s* + 1
    }
    __syncthreads();
    const int per = (p + 1023) / 1024;
    const int c0 = min(t * per, p), c1 = min(c0 + per, p);
    int sum = 0;
    for (int c = c0; c < c1; ++c) sum += cnt[c];
    part[t] = sum;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int v = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int at = t > 0 ? part[t - 1] : 0;
    for (int c = c0; c < c1; ++c) {
        const int sl = cnt[c] - 1;
        for (int st = 0; st <= sl; ++st) out[at++] = (c * T + st) | (st == sl ? (T - 1 - sl) << LIVE_SHIFT : 0);
    }
    if (t == 1023) n_live[b] = part[1023];
    if constexpr (FWD) {
        const int cpg = 4 / T;                 // centres per group: 1 (s = 64) or 2 (s = 32)
        const int groups = p / cpg;            // (p * T is a multiple of 4)
        const int gper = (groups + 1023) / 1024;
        const int g0 = min(t * gper, groups), g1 = min(g0 + gper, groups);
        auto group_size = [&](int g) { return cpg == 1 ? (int)cnt[g] : (int)cnt[2 * g] + (int)cnt[2 * g + 1]; };
        int len[4] = {0, 0, 0, 0};
        for (int g = g0; g < g1; ++g) {
            const int sz = group_size(g);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int used = (u + len[u]) & 3;
                len[u] += (used + sz > 4 ? 4 - used : 0) + sz;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) fmap[u * 1024 + t] = len[u];
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) { // inclusive scan: the runs t - off + 1 .. t, composed left to right
            int left[4] = {0, 0, 0, 0};
            if (t >= off) {
#pragma unroll
                for (int u = 0; u < 4; ++u) left[u] = fmap[u * 1024 + t - off];
            }
            __syncthreads();
            if (t >= off) {
                int mine[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) mine[u] = fmap[((u + left[u]) & 3) * 1024 + t];
#pragma unroll
                for (int u = 0; u < 4; ++u) left[u] += mine[u];
            }
            __syncthreads();
            if (t >= off) {
#pragma unroll
                for (int u = 0; u < 4; ++u) fmap[u * 1024 + t] = left[u];
            }
            __syncthreads();
        }
        int *fo = fwd + (size_t)b * p * T;
        int fat = t > 0 ? fmap[t - 1] : 0; // from state 0
        for (int g = g0; g < g1; ++g) {
            const int used = fat & 3;
            if (used + group_size(g) > 4)
                for (int u = used; u < 4; ++u) fo[fat++] = LIVE_PAD;
            for (int c = g * cpg; c < (g + 1) * cpg; ++c) {
                const int sl = cnt[c] - 1;
                for (int st = 0; st <= sl; ++st) fo[fat++] = (c * T + st) | (st == sl ? (T - 1 - sl) << LIVE_SHIFT : 0);
            }
        }
        if (t == 1023) n_fwd[b] = fmap[1023];
    }
}

// Both entry points.  want_fwd: the forward list is made in the same launch (s in {32, 64}, p * s a multiple of 64); else the
// plain form (s in {16, 32, 64}).  A flag and not `fwd != nullptr`: a null fwd handed to ogc_live_steps_fwd is that entry
// point's null-pointer error, reported after its shape checks as before.
int live_steps_impl(const char *name, int b, int p, int s, const int *idx, int *live, int *n_live, int *fwd, int *n_fwd,
                    bool want_fwd, ogc_stream_t stream) {
    OGC_REQUIRE(b >= 0 && p >= 1, "%s: bad shape", name);
    if (!want_fwd && s != 16 && s != 32 && s != 64) {
        ogc_set_error("%s: nsample=%d must be 16, 32 or 64", name, s);
        return OGC_ERR_UNSUPPORTED;
    }
    if (want_fwd && ((s != 32 && s != 64) || (p * (long long)s) % 64 != 0)) {
        ogc_set_error("%s: needs nsample 32 or 64 and p * nsample %% 64 == 0 (p=%d, nsample=%d)", name, p, s);
        return OGC_ERR_UNSUPPORTED;
    }
    OGC_REQUIRE(idx && live && n_live && (!want_fwd || (fwd && n_fwd)), "%s: null pointer", name);
    if (p > LIVE_MAX_P) {
        ogc_set_error("%s: p=%d centres per sample, at most %d", name, p, LIVE_MAX_P);
        return OGC_ERR_UNSUPPORTED;
    }
    if (b == 0) return OGC_OK;
    if (want_fwd) hipLaunchKernelGGL(live_steps_kernel<true>, dim3(b), dim3(1024), 0, (hipStream_t)stream, p, s, idx, live, n_live, fwd, n_fwd);
    else hipLaunchKernelGGL(live_steps_kernel<false>, dim3(b), dim3(1024), 0, (hipStream_t)stream, p, s, idx, live, n_live);
    OGC_CHECK_LAUNCH(name);
    return OGC_OK;
}

} // namespace

// live (b, p * s / 16), n_live (b): the live-step list of a neighbour list idx (b, p, s) (live_steps.h).
extern "C" int ogc_live_steps(int b, int p, int s, const int *idx, int *live, int *n_live, ogc_stream_t stream) {
    return live_steps_impl("ogc_live_steps", b, p, s, idx, live, n_live, nullptr, nullptr, false, stream);
}

// ogc_live_steps, and in the same launch the forward list fwd (b, p * s / 16), n_fwd (b) (live_steps.h): the same entries packed so
// that no 64-position group crosses a tile of four entries.  s in {32, 64}, p * s a multiple of 64.
extern "C" int ogc_live_steps_fwd(int b, int p, int s, const int *idx, int *live, int *n_live, int *fwd, int *n_fwd,
                                  ogc_stream_t stream) {
    return live_steps_impl("ogc_live_steps_fwd", b, p, s, idx, live, n_live, fwd, n_fwd, true, stream);
}

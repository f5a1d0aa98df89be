// kittisf_prepare.hip — the device stage of the KITTI Scene Flow preparation: disparity and optical-flow maps
// unprojected to two clouds in correspondence, the far and invalid pixels dropped, the instance ids relabelled.  Replaces
// data_prepare/kittisf/process_kittisf.py:43-87 with kittisf_util.py:6-27 (pixel2xyz), :59-63 (disp_2_depth), :72-81 (filter_segm).
//
// Per pixel (row i, column j), all fp32, one rounding per operation (the *_rn intrinsics), exactly the reference's expressions:
//   valid  = d1 > 0 && d2 > 0 && flow[2] == 1
//   depthk = fb / (float(dk) / 256 + 1e-5f)
//   x1 = -((float(j) * (depth1 + p23) - (p02 * depth1 + p03)) / f),  y1 with float(i), p12, p13,  z1 = depth1
//   px2 = float(j) + (float(flow[0]) - 32768) / 64,  py2 = float(i) + (float(flow[1]) - 32768) / 64;  x2, y2, z2 with depth2
//   keep = valid && z1 < depth_thresh && z2 < depth_thresh
// The reference indexes with the boolean mask — a STABLE compaction, and FPS later starts at row 0 —, so the launch structure is
// that of the scan crops (scan_prepare.hip): ordinary launches on the caller's stream, no waiting between workgroups:
//   clear    the 65 536-bit presence table of the raw instance ids, in the stream's workspace;
//   count    a workgroup per tile of OGC_SCAN_CROP_TILE pixels evaluates the predicate, stores the tile's number of kept pixels
//            and sets the table bit of every kept pixel's id: atomicOr into a copy of the table in LDS first (a lane whose left
//            neighbour in the wave sets the same bit leaves it to the neighbour), then one vector atomicOr per non-zero word
//            into the table — the maps are piecewise constant and mostly background, and one global atomic per run of equal
//            ids, all on a handful of addresses, made the call 0.69 ms at the frame size where it now takes 0.027;
//   scatter  adds up the counts of the earlier tiles, RECOMPUTES the predicate (the same device function on the same bits), ranks
//            by wave ballot and writes pc1, pc2, keep_idx and the label.
// Labels (filter_segm): the ids present among the kept points whose semantic (id >> 8) is selected are numbered 1, 2, ... in
// ascending id order, everything else is 0.  No sort: every scatter workgroup loads the table into LDS, thread s masking the
// eight words of semantic s with the selection, and takes a running count over the 2048 words;
//   label(id) = 1 + selected present ids below id = 1 + before[id >> 5] + popcount(word[id >> 5] & bits below id).
// The header png_unfilter.h (plain C++) is exported from here as ogc_png_unfilter: it launches nothing.
#include "ogc_common.h"
#include "png_unfilter.h"

namespace {

constexpr int KP_THREADS = 256;
constexpr int KP_WAVES = KP_THREADS / OGC_WAVE;
constexpr int KP_ROUNDS = OGC_SCAN_CROP_TILE / KP_THREADS;
constexpr int KP_TABLE_WORDS = 65536 / 32; // one bit per raw instance id
static_assert(OGC_SCAN_CROP_TILE % KP_THREADS == 0, "a tile is a whole number of rounds");
static_assert(KP_TABLE_WORDS == KP_THREADS * 8, "thread s of the scatter kernel owns the eight table words of semantic s");

struct Unproject {
    int width;
    const unsigned short *disp1, *disp2, *flow;
    float fb, f, p02, p03, p12, p13, p23, depth_thresh;

    __device__ __forceinline__ float depth(unsigned short d) const {
        return __fdiv_rn(fb, __fadd_rn(__fdiv_rn((float)d, 256.0f), 1e-5f));
    }
    // -((pix * (depth + p23) - (c2 * depth + c3)) / f)
    __device__ __forceinline__ float axis(float pix, float z, float c2, float c3) const {
        return -__fdiv_rn(__fsub_rn(__fmul_rn(pix, __fadd_rn(z, p23)), __fadd_rn(__fmul_rn(c2, z), c3)), f);
    }
    // true: pixel p = i * width + j is kept, a and b are its points in the two clouds
    __device__ __forceinline__ bool operator()(long long p, float (&a)[3], float (&b)[3]) const {
        const unsigned short d1 = disp1[p], d2 = disp2[p];
        const unsigned short fx = flow[p * 3 + 0], fy = flow[p * 3 + 1], fv = flow[p * 3 + 2];
        const int i = (int)((unsigned)p / (unsigned)width), j = (int)((unsigned)p - (unsigned)i * (unsigned)width); // p < 2^31
        const float z1 = depth(d1), z2 = depth(d2);
        const float px2 = __fadd_rn((float)j, __fdiv_rn(__fsub_rn((float)fx, 32768.0f), 64.0f));
        const float py2 = __fadd_rn((float)i, __fdiv_rn(__fsub_rn((float)fy, 32768.0f), 64.0f));
        a[0] = axis((float)j, z1, p02, p03);
        a[1] = axis((float)i, z1, p12, p13);
        a[2] = z1;
        b[0] = axis(px2, z2, p02, p03);
        b[1] = axis(py2, z2, p12, p13);
        b[2] = z2;
        return d1 > 0 && d2 > 0 && fv == 1 && z1 < depth_thresh && z2 < depth_thresh;
    }
};

__global__ __launch_bounds__(KP_THREADS) void kittisf_count_kernel(long long n, Unproject pred, const unsigned short *__restrict__ inst,
                                                                   int *__restrict__ tile_count, unsigned *__restrict__ table) {
    __shared__ int wave_total[KP_WAVES];
    __shared__ unsigned seen[KP_TABLE_WORDS]; // the ids of this tile's kept pixels
    const int tid = threadIdx.x, lane = tid & (OGC_WAVE - 1), wave = tid / OGC_WAVE;
    const long long first = (long long)blockIdx.x * OGC_SCAN_CROP_TILE;
#pragma unroll
    for (int k = 0; k < KP_TABLE_WORDS / KP_THREADS; ++k) seen[k * KP_THREADS + tid] = 0u;
    __syncthreads();
    int kept = 0;
#pragma unroll
    for (int r = 0; r < KP_ROUNDS; ++r) {
        const long long p = first + r * KP_THREADS + tid;
        float a[3], b[3];
        const bool keep = p < n && pred(p, a, b);
        kept += __popcll(__ballot(keep)); // uniform over the wave
        const int id = keep ? (int)inst[p] : -1;
        const int left = __shfl_up(id, 1, OGC_WAVE);
        if (keep && (lane == 0 || left != id)) atomicOr(&seen[id >> 5], 1u << (id & 31));
    }
    if (lane == 0) wave_total[wave] = kept;
    __syncthreads();
    // a tile holds a handful of ids: a few words per workgroup go to the table, and only bits a look at the table does not show
    // yet (a stale look costs one atomic more, nothing else)
#pragma unroll
    for (int k = 0; k < KP_TABLE_WORDS / KP_THREADS; ++k) {
        const int w = k * KP_THREADS + tid;
        const unsigned bits = seen[w];
        if (bits != 0u && (__hip_atomic_load(&table[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bits) != bits) atomicOr(&table[w], bits);
    }
    if (tid == 0) {
        int total = 0;
        for (int w = 0; w < KP_WAVES; ++w) total += wave_total[w];
        tile_count[blockIdx.x] = total;
    }
}

__global__ __launch_bounds__(KP_THREADS) void kittisf_scatter_kernel(long long n, Unproject pred, const unsigned short *__restrict__ inst,
                                                                     const int *__restrict__ select_semantics, int n_select,
                                                                     const int *__restrict__ tile_count,
                                                                     const unsigned *__restrict__ table, float *__restrict__ pc1,
                                                                     float *__restrict__ pc2, int *__restrict__ segm,
                                                                     int *__restrict__ keep_idx, int *__restrict__ count) {
    __shared__ int before_tiles[KP_WAVES];          // partial sums of the counts of the earlier tiles
    __shared__ int wave_total[KP_ROUNDS][KP_WAVES]; // kept pixels of (round, wave) of this tile
    __shared__ unsigned selected[8];                // bit s: semantic s is selected
    __shared__ int wave_ids[KP_WAVES];              // selected present ids of the semantics a wave owns
    __shared__ unsigned word[KP_TABLE_WORDS];       // the presence table, the words of unselected semantics cleared
    __shared__ int before[KP_TABLE_WORDS];          // selected present ids in the words in front of this one
    const int tid = threadIdx.x, lane = tid & (OGC_WAVE - 1), wave = tid / OGC_WAVE;
    const int tile = blockIdx.x;
    const long long first = (long long)tile * OGC_SCAN_CROP_TILE;

    if (tid < 8) selected[tid] = 0u;
    int acc = 0;
    for (int t = tid; t < tile; t += KP_THREADS) acc += tile_count[t];
#pragma unroll
    for (int off = OGC_WAVE / 2; off > 0; off >>= 1) acc += __shfl_down(acc, off, OGC_WAVE);
    if (lane == 0) before_tiles[wave] = acc;
    __syncthreads();
    for (int e = tid; e < n_select; e += KP_THREADS) {
        const int s = select_semantics[e];
        if (s >= 0 && s < 256) atomicOr(&selected[s >> 5], 1u << (s & 31)); // an id's semantic is below 256: others match nothing
    }
    __syncthreads();

    // thread tid owns semantic tid: words tid * 8 .. tid * 8 + 7
    const bool mine = (selected[tid >> 5] >> (tid & 31)) & 1u;
    unsigned w8[8];
    int ids = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        w8[k] = mine ? table[tid * 8 + k] : 0u;
        ids += __popc(w8[k]);
    }
    int incl = ids; // inclusive scan over the wave
#pragma unroll
    for (int off = 1; off < OGC_WAVE; off <<= 1) {
        const int v = __shfl_up(incl, off, OGC_WAVE);
        if (lane >= off) incl += v;
    }
    if (lane == OGC_WAVE - 1) wave_ids[wave] = incl;

    bool keep[KP_ROUNDS];
    float a[KP_ROUNDS][3], b[KP_ROUNDS][3];
    int rank[KP_ROUNDS]; // kept pixels of the same wave and round in front of this one
#pragma unroll
    for (int r = 0; r < KP_ROUNDS; ++r) {
        const long long p = first + r * KP_THREADS + tid;
        keep[r] = p < n && pred(p, a[r], b[r]);
        const unsigned long long m = __ballot(keep[r]);
        rank[r] = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wave_total[r][wave] = __popcll(m);
    }
    __syncthreads();

    int run = incl - ids;
    for (int w = 0; w < wave; ++w) run += wave_ids[w];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        word[tid * 8 + k] = w8[k];
        before[tid * 8 + k] = run;
        run += __popc(w8[k]);
    }
    __syncthreads();

    int row = 0;
    for (int w = 0; w < KP_WAVES; ++w) row += before_tiles[w];
#pragma unroll
    for (int r = 0; r < KP_ROUNDS; ++r) {
#pragma unroll
        for (int w = 0; w < KP_WAVES; ++w) {
            const int c = wave_total[r][w];
            if (w == wave && keep[r]) {
                const long long p = first + r * KP_THREADS + tid;
                const int o = row + rank[r]; // < the number of pixels before this one: inside the n rows
                const int id = (int)inst[p];
                const unsigned bits = word[id >> 5], bit = 1u << (id & 31);
                pc1[(size_t)o * 3 + 0] = a[r][0];
                pc1[(size_t)o * 3 + 1] = a[r][1];
                pc1[(size_t)o * 3 + 2] = a[r][2];
                pc2[(size_t)o * 3 + 0] = b[r][0];
                pc2[(size_t)o * 3 + 1] = b[r][1];
                pc2[(size_t)o * 3 + 2] = b[r][2];
                segm[o] = (bits & bit) ? 1 + before[id >> 5] + __popc(bits & (bit - 1u)) : 0;
                keep_idx[o] = (int)p;
            }
            row += c;
        }
    }
    if (tile == (int)gridDim.x - 1 && tid == 0) *count = row;
}

} // namespace

extern "C" int ogc_kittisf_unproject(int height, int width, const unsigned short *disp1, const unsigned short *disp2,
                                     const unsigned short *flow, const unsigned short *inst, float fb, float f, float p02, float p03,
                                     float p12, float p13, float p23, float depth_thresh, const int *select_semantics, int n_select,
                                     float *pc1, float *pc2, int *segm, int *keep_idx, int *count, ogc_stream_t stream) {
    const char *name = "ogc_kittisf_unproject";
    OGC_REQUIRE(height >= 0 && width >= 0, "%s: negative size (height = %d, width = %d)", name, height, width);
    const long long n = (long long)height * width;
    OGC_REQUIRE(n <= 0x7fffffffLL, "%s: %d x %d pixels are beyond 32-bit indexing", name, height, width);
    OGC_REQUIRE(n_select >= 0 && n_select <= 256, "%s: n_select = %d, must be in 0..256", name, n_select);
    OGC_REQUIRE(count != nullptr, "%s: null pointer (count)", name);
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        if (hipMemsetAsync(count, 0, sizeof(int), s) != hipSuccess) {
            ogc_set_error("%s: could not clear count", name);
            return OGC_ERR_LAUNCH;
        }
        return OGC_OK;
    }
    OGC_REQUIRE(disp1 && disp2 && flow && inst && pc1 && pc2 && segm && keep_idx, "%s: null pointer", name);
    OGC_REQUIRE(n_select == 0 || select_semantics != nullptr, "%s: null pointer (select_semantics)", name);
    const int tiles = ogc_divup(n, OGC_SCAN_CROP_TILE);
    unsigned *table = static_cast<unsigned *>(ogc_workspace(s, ((size_t)KP_TABLE_WORDS + (size_t)tiles) * sizeof(int)));
    if (!table) {
        ogc_set_error("%s: no workspace for the presence table and the tile counts", name);
        return OGC_ERR_LAUNCH;
    }
    int *tile_count = reinterpret_cast<int *>(table + KP_TABLE_WORDS);
    if (ogc_zero_async(table, KP_TABLE_WORDS * sizeof(unsigned), s) != hipSuccess) {
        ogc_set_error("%s: could not clear the presence table", name);
        return OGC_ERR_LAUNCH;
    }
    const Unproject pred{width, disp1, disp2, flow, fb, f, p02, p03, p12, p13, p23, depth_thresh};
    hipLaunchKernelGGL(kittisf_count_kernel, dim3(tiles), dim3(KP_THREADS), 0, s, n, pred, inst, tile_count, table);
    OGC_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(kittisf_scatter_kernel, dim3(tiles), dim3(KP_THREADS), 0, s, n, pred, inst, select_semantics, n_select,
                       tile_count, table, pc1, pc2, segm, keep_idx, count);
    OGC_CHECK_LAUNCH(name);
    return OGC_OK;
}

extern "C" int ogc_png_unfilter(const unsigned char *in, unsigned char *out, int height, int row_bytes, int bpp) {
    int bad_row = -1;
    switch (ogc_png_unfilter_rows(in, out, height, row_bytes, bpp, &bad_row)) {
    case OGC_PNG_OK:
        return OGC_OK;
    case OGC_PNG_NULL:
        ogc_set_error("ogc_png_unfilter: null pointer");
        break;
    case OGC_PNG_SIZE:
        ogc_set_error("ogc_png_unfilter: negative size (height = %d, row_bytes = %d)", height, row_bytes);
        break;
    case OGC_PNG_BPP:
        ogc_set_error("ogc_png_unfilter: bpp = %d, must be 1, 2, 3 or 6", bpp);
        break;
    case OGC_PNG_ROW_BYTES:
        ogc_set_error("ogc_png_unfilter: row_bytes = %d is no multiple of bpp = %d", row_bytes, bpp);
        break;
    default:
        ogc_set_error("ogc_png_unfilter: filter byte above 4 in row %d", bad_row);
        break;
    }
    return OGC_ERR_INVALID_ARG;
}

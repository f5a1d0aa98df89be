// grid_dev.h — what the cell-grid sources share (grid.hip: the build; grid_ball_query.hip, grid_knn.hip: the searches; the probe
// tools/bq_probe.hip): constants, the cell functions, the wave-level helpers of the query kernels, the layout of a grid's buffer
// and the LDS budgets of the launches.  Internal to those files — grid.h is the header for everybody else.  No kernel is defined
// here, so nothing is emitted twice.
#pragma once
#include "ogc_common.h"
#include "grid.h"

namespace ogc_grid {

typedef unsigned long long u64;

constexpr int GRID_MAX_CELLS = 16384;
constexpr int STRIDE_CELLS = GRID_MAX_CELLS + 1; // cell starts per cloud (one past the last cell: the number of points)

// Development probe (tools/bq_probe.hip compiles this file with OGC_GRID_PROBE): cycle stamps of the build's phases
// (workgroup 0) and per-phase cycle sums over all wavefronts of the query.
#ifdef OGC_GRID_PROBE
__device__ unsigned long long ogc_grid_probe[64];
#define OGC_PROBE_BUILD(i) \
    if (blockIdx.x == 0 && threadIdx.x == 0) ogc_grid_probe[i] = __builtin_amdgcn_s_memtime()
#define OGC_PROBE_T(var) const unsigned long long var = __builtin_amdgcn_s_memtime()
#define OGC_PROBE_ADD(i, a, b) \
    if (threadIdx.x == 0 && (blockIdx.x & 63) == 0) atomicAdd(&ogc_grid_probe[i], (b) - (a))
#else
#define OGC_PROBE_BUILD(i)
#define OGC_PROBE_T(var)
#define OGC_PROBE_ADD(i, a, b)
#endif

__device__ __forceinline__ int cell_coord(float x, float mn, float inv_h, int g) {
    // floor((x - mn) * inv_h) clamped to [-2, g + 1]; NaN -> -2 (outside every neighbourhood)
    const float f = floorf((x - mn) * inv_h);
    if (!(f >= -2.0f)) return -2;
    if (f > (float)(g + 1)) return g + 1;
    return (int)f;
}

// max(floor((x - mn) * inv_h), 0) as an int, for a FINITE x: the cell coordinate before the clamp to the grid's upper edge
// (the median keeps the conversion in range; a NaN — a centre that is no point of the grid — gives 0)
__device__ __forceinline__ int cell_floor(float x, float mn, float inv_h) {
    return (int)__builtin_amdgcn_fmed3f(floorf((x - mn) * inv_h), 0.0f, 1.0e9f);
}

// min(max(floor((x - mn) * inv_h), 0), g - 1) in four instructions: subtract, multiply (the same two roundings as cell_floor),
// convert with floor rounding (saturating; NaN -> 0) and an integer median.  Equal to min(cell_floor(x, mn, inv_h), g - 1).
__device__ __forceinline__ int cell_clamped(float x, float mn, float inv_h, int g) {
    const float q = (x - mn) * inv_h;
    int c, r;
    asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(c) : "v"(q));
    asm("v_med3_i32 %0, %1, 0, %2" : "=v"(r) : "v"(c), "v"(g - 1));
    return r;
}

// a point's coordinates along the grid's (fast, mid, slow) axes (GridHdr::fast; wave-uniform selects)
#define OGC_GRID_AXES(H, X, Y, Z, FX, FY, FZ)                                                    \
    const float FX = (H).fast == 0 ? (X) : ((H).fast == 1 ? (Y) : (Z)), FY = (H).fast == 0 ? (Y) : (X), \
                FZ = (H).fast == 2 ? (Y) : (Z)

constexpr int SUB = 8;               // lanes cooperating on one query in the finishing steps
constexpr int QPW = OGC_WAVE / SUB;  // queries (centres) per wavefront

__device__ __forceinline__ int lane_bcast(int v, int src) { return __builtin_amdgcn_readlane(v, src); }
__device__ __forceinline__ float lane_bcast(float v, int src) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}

// The candidate runs of a box of cells [xlo, xhi] x (y0-1 .. y0+1) x (z0-1 .. z0+1): the cells of one (y, z) row are
// contiguous in the cell-sorted array, so the box is NINE runs.  Lane r < 9 fetches run r; the nine (start, offset)
// pairs are then broadcast to scalars so that every lane can map a flat candidate number to an array position.
// (A macro, not a struct: the eighteen scalars must stay in SGPRs — as members of an object passed by reference the
// compiler put them in scratch memory and indexed them per candidate.)
// (SLAB — GridHdr::slab, the fast axis has at most two cells: THREE runs, the cells (any x, XLO .. XHI) of the rows z - 1 ..
// z + 1, where XLO .. XHI is then a range of y; the other six runs are empty)
#define OGC_BOX_SETUP(SLAB, XLO, XHI, Y0, Z0)                                                        \
    {                                                                                                \
        int lo_ = 0, len_ = 0;                                                                       \
        if ((SLAB) && lane < 3) {                                                                    \
            const int z_ = (Z0) + lane - 1;                                                          \
            if (z_ >= 0 && z_ < h.gz && (XLO) <= (XHI)) {                                            \
                lo_ = cs[h.gx * ((XLO) + h.gy * z_)];                                                \
                len_ = cs[h.gx * ((XHI) + h.gy * z_) + h.gx] - lo_;                                  \
            }                                                                                        \
        } else if (!(SLAB) && lane < 9) {                                                            \
            const int y_ = (Y0) + (lane % 3) - 1, z_ = (Z0) + (lane / 3) - 1;                        \
            if (y_ >= 0 && y_ < h.gy && z_ >= 0 && z_ < h.gz && (XLO) <= (XHI)) {                    \
                const int rowc_ = h.gx * (y_ + h.gy * z_);                                           \
                lo_ = cs[rowc_ + (XLO)];                                                             \
                len_ = cs[rowc_ + (XHI) + 1] - lo_;                                                  \
            }                                                                                        \
        }                                                                                            \
        int incl_ = len_;                                                                            \
        _Pragma("unroll") for (int off_ = 1; off_ < 16; off_ <<= 1) {                                \
            const int up_ = __shfl_up(incl_, off_, 64);                                              \
            if (lane >= off_) incl_ += up_;                                                          \
        }                                                                                            \
        const int excl_ = incl_ - len_;                                                              \
        box_total = lane_bcast(incl_, 8);                                                            \
        b0 = lane_bcast(lo_ - excl_, 0);                                                             \
        s1 = lane_bcast(excl_, 1); b1 = lane_bcast(lo_ - excl_, 1);                                  \
        s2 = lane_bcast(excl_, 2); b2 = lane_bcast(lo_ - excl_, 2);                                  \
        s3 = lane_bcast(excl_, 3); b3 = lane_bcast(lo_ - excl_, 3);                                  \
        s4 = lane_bcast(excl_, 4); b4 = lane_bcast(lo_ - excl_, 4);                                  \
        s5 = lane_bcast(excl_, 5); b5 = lane_bcast(lo_ - excl_, 5);                                  \
        s6 = lane_bcast(excl_, 6); b6 = lane_bcast(lo_ - excl_, 6);                                  \
        s7 = lane_bcast(excl_, 7); b7 = lane_bcast(lo_ - excl_, 7);                                  \
        s8 = lane_bcast(excl_, 8); b8 = lane_bcast(lo_ - excl_, 8);                                  \
    }
// the LAST run whose start is <= f (empty runs share their start with the next one)
#define OGC_BOX_POSITION(F)                                                                           \
    ((F) + ((F) >= s8 ? b8 : (F) >= s7 ? b7 : (F) >= s6 ? b6 : (F) >= s5 ? b5 : (F) >= s4 ? b4       \
                     : (F) >= s3 ? b3 : (F) >= s2 ? b2 : (F) >= s1 ? b1 : b0))

// squared distances of ONE candidate to TWO centres, packed (v_pk_*_f32): the reference's fp32 expression per half
__device__ __forceinline__ ogc_v2f sqdist_pair(ogc_v2f qx, ogc_v2f qy, ogc_v2f qz, float x, float y, float z) {
#pragma clang fp contract(off)
    const ogc_v2f cx2 = {x, x}, cy2 = {y, y}, cz2 = {z, z};
    const ogc_v2f dx = qx - cx2, dy = qy - cy2, dz = qz - cz2;
    return ogc_sqsum3(dx, dy, dz);
}

// ---- constants of the four-lanes-per-centre kernels (ball_query_cells_kernel; knn_cells_kernel has the same structure) -------
#ifndef OGC_BQ_STRIP_PAD
#define OGC_BQ_STRIP_PAD 0
#endif
constexpr int CL = 4;                 // lanes per centre
constexpr int CPW = OGC_WAVE / CL;    // centres per wavefront
constexpr int BQ_FAST = 32;           // hits per centre the register sort holds
constexpr int BQ_CAP = 64;            // hit slots per centre (slot BQ_CAP takes the misses; also the general body's lists)
constexpr int BQ_SEG = 20;            // ints per lane of a centre's LDS strip: 16 private hit slots, slot 16 takes misses / overflow
// ints per centre (the compacted list of up to BQ_CAP hits + sentinels lives in the same strip) + BQ_STRIP_PAD.  With 80 ints per
// centre the sixteen strips of a wavefront start in two banks only (80 mod 32 = 16); padding the strips to 84 spreads them over
// eight start banks but costs the eighth wavefront per SIMD (5376 bytes per wavefront: 18.1 against 16.9 us) — the pad stays 0 and
// the MISSES, which are most of the stores, go to one of the four spare slots of a lane's segment by centre pair instead
constexpr int BQ_STRIP_PAD = OGC_BQ_STRIP_PAD;
constexpr int BQ_LIST = CL * BQ_SEG + BQ_STRIP_PAD;
constexpr int BQ_RUN = 128;           // longest run the slab walk takes (a longer one sends the wavefront to the general body)
constexpr int BQ_PAD = BQ_RUN + 32;   // records readable past the end of the cell-sorted array (lanes whose run has ended read on)

// 16-byte store of an output row piece, non-temporal: the rows are 33 MB that nobody in this launch reads again; as ordinary
// stores they sit dirty in the L2s until the end-of-kernel write-back (1.6 us of the operator at the C4 loss shape).
__device__ __forceinline__ void store_row16(int *p, int4 v) {
    typedef int v4i_ __attribute__((ext_vector_type(4)));
    const v4i_ vv = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(vv, reinterpret_cast<v4i_ *>(p));
}

template <int R>
__device__ __forceinline__ int quad_bcast(int v) { // lane R of every group of four lanes
    return __builtin_amdgcn_update_dpp(0, v, R * 0x55, 0xF, 0xF, true);
}

__device__ __forceinline__ u64 shfl_xor_u64(u64 v, int off) {
    const unsigned lo = __shfl_xor((unsigned)v, off, 64), hi = __shfl_xor((unsigned)(v >> 32), off, 64);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 shfl_u64(u64 v, int src) {
    const unsigned lo = __shfl((unsigned)v, src, 64), hi = __shfl((unsigned)(v >> 32), src, 64);
    return ((u64)hi << 32) | lo;
}

// ---- host side --------------------------------------------------------------------------------------------------------------
struct GridLayout { // one buffer: headers | cell starts | cell-sorted records (+ BQ_PAD readable records behind them)
    size_t bytes_hdr, bytes_cs, bytes_pts;
    GridLayout(int b, int n)
        : bytes_hdr((sizeof(GridHdr) * b + 255) / 256 * 256),
          bytes_cs((sizeof(int) * (size_t)b * STRIDE_CELLS + 255) / 256 * 256),
          bytes_pts(sizeof(float4) * ((size_t)b * n + BQ_PAD)) {}
    size_t total() const { return bytes_hdr + bytes_cs + bytes_pts; }
    GridHdr *hdrs(void *p) const { return reinterpret_cast<GridHdr *>(p); }
    int *cell_start(void *p) const { return reinterpret_cast<int *>(static_cast<char *>(p) + bytes_hdr); }
    float4 *sorted_pts(void *p) const { return reinterpret_cast<float4 *>(static_cast<char *>(p) + bytes_hdr + bytes_cs); }
};

// queues the build of b clouds of n points on `s` (grid.hip).  knn_k == 0: cells of edge 1.01 radius; else density-based, with
// points per cell = k / knn_div (33.5: cell edge = half the expected k-th neighbour distance)
void launch_grid_build(int b, int n, float radius, int knn_k, int stride_cells, const float *xyz, GridHdr *hdrs, int *cell_start,
                       float4 *sorted_pts, hipStream_t s, int prefer_cells = 0, float knn_div = 33.5f);

// ---- LDS budgets ------------------------------------------------------------------------------------------------------------
// ball_query_grid_body: [QPW][hit_cap] hit lists, [QPW][nsample] sorted rows, a bitmap over the point indices (overflow path)
inline size_t ball_query_body_lds(int n, int nsample, int hit_cap) {
    return ((size_t)QPW * (hit_cap + nsample) + (size_t)(n + 31) / 32) * sizeof(int);
}
// hit slots per centre of ball_query_grid_kernel: the smallest list that holds a full row keeps the LDS footprint at ~5 KiB per
// wavefront, i.e. the full eight wavefronts per SIMD; a centre with more hits takes the bitmap path
inline int ball_query_hit_cap(int nsample) { return nsample > 64 ? nsample : 64; }
// ball_query_cells_kernel, per wavefront: its sixteen strips, or what the general body needs when it takes a wavefront over
inline size_t ball_query_cells_lds(int n, int nsample) {
    const size_t body = ball_query_body_lds(n, nsample, BQ_CAP), strips = sizeof(int) * CPW * BQ_LIST;
    return body > strips ? body : strips;
}
constexpr int KNN_FLAT_CAP = 192; // positions of the first shell kept as one flat list per query (else: run by run)
// knn_grid_kernel: [QPW][k] kept keys, [QPW][k] sorted keys, [QPW][KNN_FLAT_CAP] positions (eight lanes per query: the most queries)
inline size_t knn_grid_lds(int k) { return (size_t)2 * QPW * k * sizeof(u64) + (size_t)QPW * KNN_FLAT_CAP * sizeof(int); }

} // namespace ogc_grid

// depth_render.hip — the device stage of the OGC-DRSV preparation: a depth render of triangle meshes through a pinhole
// view and the cloud of its hit points, what data_prepare/ogcdrsv/build_ogcdrsv.py obtains from open3d's visualiser.  The contract is
// this package's own and is written out in include/ogc_ops.h (ogc_depth_render); everything is fp64 with one rounding per operation
// (the build passes -ffp-contract=off, the functions below repeat it), and tests/depth_render_cases.py repeats the sequence in numpy.
//
// Launches of ogc_depth_render, all on the caller's stream, none waits for another inside a launch:
//   setup     a thread per face: the device-side checks (status code), camera and screen coordinates, the near rule, the plane, the
//             pixel box clamped to the image, and the face's class: EMPTY (no centre can be covered), SMALL (a box of at most
//             DR_SMALL_PIXELS centres) or LARGE (counted in blocks of 8 x 8 pixels aligned to the image).  A 128-byte record per face.
//   offsets   the running sum of the LARGE faces' block counts: item_start (F + 1), by the tile sums of setup.
//   init      depth = +inf, face = -1.
//   small<0>, large<0>   depth[pixel] = min(depth[pixel], t) by a 64-bit atomicMin on the bit pattern: t > 0, so the bits order like
//             the values.  small: a lane per face walks its box, at most DR_SMALL_PIXELS centres.  large: a wavefront per
//             (face, block) item, a lane per centre; the item's face by bisection of item_start.  So no lane tests more than
//             DR_SMALL_PIXELS centres for a face or one for an item, whatever the sizes of the triangles.
//   small<1>, large<1>   the same walk, the same t from the same record: where t equals the stored depth, face[pixel] =
//             min(face[pixel], index) by a 32-bit unsigned atomicMin (-1 is the largest unsigned word).
// The minimum of a set does not depend on the order of its elements, so both images are the same in every run.  atomicMin is HIP's
// default: relaxed, agent scope, carried out at the memory side of the L2s, so waves on different XCDs meet on one value; the depth
// that pass 1 compares with was written by an earlier launch.  ogc_depth_points is the stable compaction of kittisf_prepare.hip
// (count per tile, then rank by ballot and scatter) over the pixels in row-major order.
#include <math.h>

#include "ogc_common.h"

namespace {

constexpr int DR_THREADS = 256;
constexpr int DR_WAVES = DR_THREADS / OGC_WAVE;
constexpr int DR_SMALL_PIXELS = 32;   // a box of at most this many centres is walked by one lane
constexpr int DR_LARGE_GROUPS = 2048; // workgroups of the item kernels: 8192 wavefronts stride over the items
constexpr int DR_TILE = 1024;         // pixels per workgroup of the compaction
constexpr int DR_ROUNDS = DR_TILE / DR_THREADS;
constexpr int DR_MAX_SIDE = 16384;    // width and height: a face has at most 2048 x 2048 blocks
constexpr int DR_MAX_FACES = 1 << 24;
constexpr unsigned long long DR_INF_BITS = 0x7ff0000000000000ull;

struct View { // OGC_DEPTH_VIEW_DOUBLES doubles in this order
    double e[3], right[3], up[3], back[3], f, cx, cy, near_, far_;
};
static_assert(sizeof(View) == OGC_DEPTH_VIEW_DOUBLES * sizeof(double), "the view is the array the header describes");

struct FaceRec {
    double s[6];        // screen x, y of the three vertices
    double n[3], nc0;   // the plane in camera coordinates: n = cross(c1 - c0, c2 - c0), nc0 = n . c0
    double zmin, zmax;  // the range of the three zc
    int x0, y0, x1, y1; // pixel box, inclusive, inside the image (meaningful when small_ or items)
    int items;          // LARGE: blocks of 8 x 8 pixels the box touches; otherwise 0
    int small_;         // SMALL: 1
    int pad[2];
};
static_assert(sizeof(FaceRec) == 128, "a record is 128 bytes");

__device__ __forceinline__ bool dr_finite(double v) { return fabs(v) <= 1.7976931348623157e308; } // false for NaN

// Is the centre of pixel (x, y) covered by the face, and at which depth?  The contract's sequence, operation by operation.
__device__ __forceinline__ bool dr_hit(const FaceRec &r, const View &v, int x, int y, double &t_out) {
#pragma clang fp contract(off)
    const double qx = (double)x + 0.5, qy = (double)y + 0.5;
    const double ax = r.s[0], ay = r.s[1], bx = r.s[2], by = r.s[3], cx = r.s[4], cy = r.s[5];
    // the closed bounding interval of the screen vertices (finite by setup)
    if (!(qx >= fmin(fmin(ax, bx), cx) && qx <= fmax(fmax(ax, bx), cx) && qy >= fmin(fmin(ay, by), cy) && qy <= fmax(fmax(ay, by), cy)))
        return false;
    const double e0 = (bx - ax) * (qy - ay) - (by - ay) * (qx - ax);
    const double e1 = (cx - bx) * (qy - by) - (cy - by) * (qx - bx);
    const double e2 = (ax - cx) * (qy - cy) - (ay - cy) * (qx - cx);
    const bool covered = (e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0) || (e0 <= 0.0 && e1 <= 0.0 && e2 <= 0.0);
    if (!covered) return false;
    const double gx = (qx - v.cx) / v.f, gy = -((qy - v.cy) / v.f);
    const double ng = (r.n[0] * gx + r.n[1] * gy) + r.n[2];
    if (ng == 0.0) return false;
    double t = r.nc0 / ng;
    if (!dr_finite(t)) return false;
    t = fmin(fmax(t, r.zmin), r.zmax);
    if (!(t >= v.near_ && t <= v.far_)) return false;
    t_out = t;
    return true;
}

__global__ __launch_bounds__(DR_THREADS) void dr_setup_kernel(int V, int F, const double *__restrict__ vertices,
                                                              const int *__restrict__ faces, View v, int W, int H,
                                                              FaceRec *__restrict__ rec, long long *__restrict__ tile_items,
                                                              int *__restrict__ status) {
#pragma clang fp contract(off)
    __shared__ int wave_items[DR_WAVES];
    const int tid = threadIdx.x, lane = tid & (OGC_WAVE - 1), wave = tid / OGC_WAVE;
    const int f = blockIdx.x * DR_THREADS + tid; // F <= 2^24
    int code = 0, items = 0;
    bool dropped = false;
    if (f < F) {
        FaceRec r;
        r.x0 = r.y0 = 0;
        r.x1 = r.y1 = -1;
        r.items = r.small_ = r.pad[0] = r.pad[1] = 0;
#pragma unroll
        for (int k = 0; k < 6; ++k) r.s[k] = 0.0;
        r.n[0] = r.n[1] = r.n[2] = r.nc0 = r.zmin = r.zmax = 0.0;
        const int i0 = faces[(size_t)f * 3 + 0], i1 = faces[(size_t)f * 3 + 1], i2 = faces[(size_t)f * 3 + 2];
        if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) {
            code = 1;
        } else {
            const int idx[3] = {i0, i1, i2};
            double c[3][3]; // camera coordinates (xc, yc, zc) of the three vertices
            bool finite_in = true, finite_cam = true;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double *p = vertices + (size_t)idx[k] * 3;
                const double px = p[0], py = p[1], pz = p[2];
                finite_in = finite_in && dr_finite(px) && dr_finite(py) && dr_finite(pz);
                const double dx = px - v.e[0], dy = py - v.e[1], dz = pz - v.e[2];
                c[k][0] = (v.right[0] * dx + v.right[1] * dy) + v.right[2] * dz;
                c[k][1] = (v.up[0] * dx + v.up[1] * dy) + v.up[2] * dz;
                c[k][2] = -((v.back[0] * dx + v.back[1] * dy) + v.back[2] * dz);
                finite_cam = finite_cam && dr_finite(c[k][0]) && dr_finite(c[k][1]) && dr_finite(c[k][2]);
            }
            if (!finite_in) {
                code = 2;
            } else if (c[0][2] < v.near_ || c[1][2] < v.near_ || c[2][2] < v.near_) {
                dropped = true;
            } else {
                bool ok = finite_cam;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    r.s[2 * k + 0] = v.cx + v.f * (c[k][0] / c[k][2]);
                    r.s[2 * k + 1] = v.cy - v.f * (c[k][1] / c[k][2]);
                    ok = ok && dr_finite(r.s[2 * k + 0]) && dr_finite(r.s[2 * k + 1]);
                }
                const double area = (r.s[2] - r.s[0]) * (r.s[5] - r.s[1]) - (r.s[3] - r.s[1]) * (r.s[4] - r.s[0]);
                ok = ok && !(area == 0.0);
                if (ok) {
                    const double ux = c[1][0] - c[0][0], uy = c[1][1] - c[0][1], uz = c[1][2] - c[0][2];
                    const double wx = c[2][0] - c[0][0], wy = c[2][1] - c[0][1], wz = c[2][2] - c[0][2];
                    r.n[0] = uy * wz - uz * wy;
                    r.n[1] = uz * wx - ux * wz;
                    r.n[2] = ux * wy - uy * wx;
                    r.nc0 = (r.n[0] * c[0][0] + r.n[1] * c[0][1]) + r.n[2] * c[0][2];
                    r.zmin = fmin(fmin(c[0][2], c[1][2]), c[2][2]);
                    r.zmax = fmax(fmax(c[0][2], c[1][2]), c[2][2]);
                    // every centre inside the closed bounding interval lies in this box: floor(round(m - 0.5)) <= ceil(m - 0.5) and
                    // ceil(round(m - 0.5)) >= floor(m - 0.5), rounding being monotone and the integers representable
                    const double x0 = fmax(floor(fmin(fmin(r.s[0], r.s[2]), r.s[4]) - 0.5), 0.0);
                    const double x1 = fmin(ceil(fmax(fmax(r.s[0], r.s[2]), r.s[4]) - 0.5), (double)(W - 1));
                    const double y0 = fmax(floor(fmin(fmin(r.s[1], r.s[3]), r.s[5]) - 0.5), 0.0);
                    const double y1 = fmin(ceil(fmax(fmax(r.s[1], r.s[3]), r.s[5]) - 0.5), (double)(H - 1));
                    if (x0 <= x1 && y0 <= y1) {
                        r.x0 = (int)x0;
                        r.x1 = (int)x1;
                        r.y0 = (int)y0;
                        r.y1 = (int)y1;
                        const long long pixels = (long long)(r.x1 - r.x0 + 1) * (r.y1 - r.y0 + 1);
                        if (pixels <= DR_SMALL_PIXELS)
                            r.small_ = 1;
                        else
                            r.items = ((r.x1 >> 3) - (r.x0 >> 3) + 1) * ((r.y1 >> 3) - (r.y0 >> 3) + 1); // <= 2048 * 2048
                    }
                }
            }
        }
        items = r.items;
        rec[f] = r;
    }
    if (code != 0) atomicMax(&status[0], code);
    const unsigned long long drops = __ballot(dropped);
    if (lane == 0 && drops != 0ull) atomicAdd(&status[2], __popcll(drops));
    // items of this tile of faces: 256 x 2^22 stays below 2^31
    int sum = items;
#pragma unroll
    for (int off = OGC_WAVE / 2; off > 0; off >>= 1) sum += __shfl_down(sum, off, OGC_WAVE);
    if (lane == 0) wave_items[wave] = sum;
    __syncthreads();
    if (tid == 0) {
        long long total = 0;
        for (int w = 0; w < DR_WAVES; ++w) total += wave_items[w];
        tile_items[blockIdx.x] = total;
    }
}

// item_start[f] = items of the faces in front of f; item_start[F] = all items
__global__ __launch_bounds__(DR_THREADS) void dr_offsets_kernel(int F, const FaceRec *__restrict__ rec,
                                                                const long long *__restrict__ tile_items,
                                                                long long *__restrict__ item_start) {
    __shared__ long long before_tiles[DR_WAVES];
    __shared__ int wave_items[DR_WAVES];
    const int tid = threadIdx.x, lane = tid & (OGC_WAVE - 1), wave = tid / OGC_WAVE;
    const int tile = blockIdx.x;
    const int f = tile * DR_THREADS + tid;
    long long acc = 0;
    for (int t = tid; t < tile; t += DR_THREADS) acc += tile_items[t];
#pragma unroll
    for (int off = OGC_WAVE / 2; off > 0; off >>= 1) acc += __shfl_down(acc, off, OGC_WAVE);
    if (lane == 0) before_tiles[wave] = acc;
    const int items = f < F ? rec[f].items : 0;
    int incl = items; // inclusive scan over the wave
#pragma unroll
    for (int off = 1; off < OGC_WAVE; off <<= 1) {
        const int up = __shfl_up(incl, off, OGC_WAVE);
        if (lane >= off) incl += up;
    }
    if (lane == OGC_WAVE - 1) wave_items[wave] = incl;
    __syncthreads();
    long long start = 0;
    for (int w = 0; w < DR_WAVES; ++w) start += before_tiles[w];
    for (int w = 0; w < wave; ++w) start += wave_items[w];
    if (f < F) {
        item_start[f] = start + (incl - items);
        if (f == F - 1) item_start[F] = start + incl;
    }
}

__global__ __launch_bounds__(DR_THREADS) void dr_init_kernel(long long n, unsigned long long *__restrict__ depth, int *__restrict__ face,
                                                             const int *__restrict__ status) {
    if (status[0] != 0) return;
    const long long stride = (long long)gridDim.x * DR_THREADS;
    for (long long p = (long long)blockIdx.x * DR_THREADS + threadIdx.x; p < n; p += stride) {
        depth[p] = DR_INF_BITS;
        face[p] = -1;
    }
}

template <int PASS>
__device__ __forceinline__ void dr_deposit(const FaceRec &r, const View &v, int f, int x, int y, int W, unsigned long long *depth,
                                           unsigned *face) {
    double t;
    if (!dr_hit(r, v, x, y, t)) return;
    const size_t p = (size_t)y * W + x; // inside the image: the box is clamped
    const unsigned long long bits = (unsigned long long)__double_as_longlong(t); // t >= near > 0
    if (PASS == 0)
        atomicMin(&depth[p], bits);
    else if (depth[p] == bits)
        atomicMin(&face[p], (unsigned)f);
}

template <int PASS>
__global__ __launch_bounds__(DR_THREADS) void dr_small_kernel(int F, const FaceRec *__restrict__ rec, View v, int W,
                                                              unsigned long long *depth, unsigned *face, const int *__restrict__ status) {
    if (status[0] != 0) return;
    const int f = blockIdx.x * DR_THREADS + threadIdx.x;
    if (f >= F) return;
    if (rec[f].small_ == 0) return;
    const FaceRec r = rec[f];
    for (int y = r.y0; y <= r.y1; ++y) // at most DR_SMALL_PIXELS centres in all
        for (int x = r.x0; x <= r.x1; ++x) dr_deposit<PASS>(r, v, f, x, y, W, depth, face);
}

template <int PASS>
__global__ __launch_bounds__(DR_THREADS) void dr_large_kernel(int F, const FaceRec *__restrict__ rec,
                                                              const long long *__restrict__ item_start, View v, int W,
                                                              unsigned long long *depth, unsigned *face, const int *__restrict__ status) {
    if (status[0] != 0) return;
    const int lane = threadIdx.x & (OGC_WAVE - 1);
    const long long waves = (long long)gridDim.x * DR_WAVES;
    const long long total = item_start[F];
    for (long long item = (long long)blockIdx.x * DR_WAVES + threadIdx.x / OGC_WAVE; item < total; item += waves) {
        int lo = 0, hi = F; // item_start[lo] <= item < item_start[hi]
        while (hi - lo > 1) {
            const int mid = lo + ((hi - lo) >> 1);
            if (item_start[mid] <= item)
                lo = mid;
            else
                hi = mid;
        }
        const FaceRec r = rec[lo]; // the same address in every lane
        const int k = (int)(item - item_start[lo]);
        const int nbx = (r.x1 >> 3) - (r.x0 >> 3) + 1;
        const int x = (((r.x0 >> 3) + k % nbx) << 3) + (lane & 7);
        const int y = (((r.y0 >> 3) + k / nbx) << 3) + (lane >> 3);
        if (x >= r.x0 && x <= r.x1 && y >= r.y0 && y <= r.y1) dr_deposit<PASS>(r, v, lo, x, y, W, depth, face);
    }
}

// ---- the cloud: covered pixels in row-major order ------------------------------------------------------------------------------
__global__ __launch_bounds__(DR_THREADS) void dr_count_kernel(long long n, const int *__restrict__ face, int *__restrict__ tile_count,
                                                              const int *__restrict__ status) {
    __shared__ int wave_total[DR_WAVES];
    if (status[0] != 0) return;
    const int tid = threadIdx.x, lane = tid & (OGC_WAVE - 1), wave = tid / OGC_WAVE;
    const long long first = (long long)blockIdx.x * DR_TILE;
    int kept = 0;
#pragma unroll
    for (int r = 0; r < DR_ROUNDS; ++r) {
        const long long p = first + r * DR_THREADS + tid;
        kept += __popcll(__ballot(p < n && face[p] >= 0)); // uniform over the wave
    }
    if (lane == 0) wave_total[wave] = kept;
    __syncthreads();
    if (tid == 0) {
        int total = 0;
        for (int w = 0; w < DR_WAVES; ++w) total += wave_total[w];
        tile_count[blockIdx.x] = total;
    }
}

__global__ __launch_bounds__(DR_THREADS) void dr_scatter_kernel(long long n, int W, View v, const double *__restrict__ depth,
                                                                const int *__restrict__ face, const int *__restrict__ tile_count,
                                                                float *__restrict__ points, int *__restrict__ pixel,
                                                                int *__restrict__ face_out, int *__restrict__ status) {
#pragma clang fp contract(off)
    __shared__ int before_tiles[DR_WAVES];
    __shared__ int wave_total[DR_ROUNDS][DR_WAVES];
    if (status[0] != 0) return;
    const int tid = threadIdx.x, lane = tid & (OGC_WAVE - 1), wave = tid / OGC_WAVE;
    const int tile = blockIdx.x;
    const long long first = (long long)tile * DR_TILE;
    int acc = 0;
    for (int t = tid; t < tile; t += DR_THREADS) acc += tile_count[t];
#pragma unroll
    for (int off = OGC_WAVE / 2; off > 0; off >>= 1) acc += __shfl_down(acc, off, OGC_WAVE);
    if (lane == 0) before_tiles[wave] = acc;
    int fidx[DR_ROUNDS], rank[DR_ROUNDS];
#pragma unroll
    for (int r = 0; r < DR_ROUNDS; ++r) {
        const long long p = first + r * DR_THREADS + tid;
        fidx[r] = p < n ? face[p] : -1;
        const unsigned long long m = __ballot(fidx[r] >= 0);
        rank[r] = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wave_total[r][wave] = __popcll(m);
    }
    __syncthreads();
    int row = 0;
    for (int w = 0; w < DR_WAVES; ++w) row += before_tiles[w];
#pragma unroll
    for (int r = 0; r < DR_ROUNDS; ++r) {
#pragma unroll
        for (int w = 0; w < DR_WAVES; ++w) {
            const int c = wave_total[r][w];
            if (w == wave && fidx[r] >= 0) {
                const long long p = first + r * DR_THREADS + tid;
                const int o = row + rank[r]; // < the number of pixels before this one: inside the n rows
                const int y = (int)((unsigned)p / (unsigned)W), x = (int)((unsigned)p - (unsigned)y * (unsigned)W); // p < 2^31
                const double qx = (double)x + 0.5, qy = (double)y + 0.5;
                const double gx = (qx - v.cx) / v.f, gy = -((qy - v.cy) / v.f);
                const double t = depth[p];
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    points[(size_t)o * 3 + k] = (float)(v.e[k] + t * ((gx * v.right[k] + gy * v.up[k]) - v.back[k]));
                pixel[o] = (int)p;
                face_out[o] = fidx[r];
            }
            row += c;
        }
    }
    if (tile == (int)gridDim.x - 1 && tid == 0) status[1] = row;
}

// the view as the kernels take it; false with the error set when it is not one
bool dr_view(const char *name, const double *view, View &v) {
    if (!view) {
        ogc_set_error("%s: null pointer (view)", name);
        return false;
    }
    for (int k = 0; k < OGC_DEPTH_VIEW_DOUBLES; ++k)
        if (!(fabs(view[k]) <= 1.7976931348623157e308)) {
            ogc_set_error("%s: view[%d] is not finite", name, k);
            return false;
        }
    for (int k = 0; k < 3; ++k) {
        v.e[k] = view[k];
        v.right[k] = view[3 + k];
        v.up[k] = view[6 + k];
        v.back[k] = view[9 + k];
    }
    v.f = view[12];
    v.cx = view[13];
    v.cy = view[14];
    v.near_ = view[15];
    v.far_ = view[16];
    if (!(v.f > 0.0 && v.near_ > 0.0 && v.near_ <= v.far_)) {
        ogc_set_error("%s: the view needs f > 0 and 0 < near <= far (f = %g, near = %g, far = %g)", name, v.f, v.near_, v.far_);
        return false;
    }
    return true;
}

size_t dr_align(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

} // namespace

extern "C" long long ogc_depth_render_ws_bytes(int F) {
    if (F < 0 || F > DR_MAX_FACES) return -1;
    const size_t tiles = (size_t)ogc_divup(F, DR_THREADS);
    return (long long)(dr_align((size_t)F * sizeof(FaceRec)) + dr_align(((size_t)F + 1) * sizeof(long long)) +
                       dr_align(tiles * sizeof(long long)) + 256);
}

// The launches of ogc_depth_render; with `ev`, four events around its three stages: setup (status, records, offsets, the empty
// image), the depth pass and the face pass.
static int dr_render(const char *name, int V, int F, const double *vertices, const int *faces, const double *view, int width, int height,
                     double *depth, int *face, int *status, void *ws, long long ws_bytes, hipStream_t s, hipEvent_t *ev) {
    OGC_REQUIRE(V >= 0 && F >= 0, "%s: negative size (V = %d, F = %d)", name, V, F);
    OGC_REQUIRE(width >= 1 && height >= 1 && width <= DR_MAX_SIDE && height <= DR_MAX_SIDE,
                "%s: the image is %d x %d, each side must be in 1..%d", name, width, height, DR_MAX_SIDE);
    if (F > DR_MAX_FACES) {
        ogc_set_error("%s: F = %d, at most %d faces per call", name, F, DR_MAX_FACES);
        return OGC_ERR_UNSUPPORTED;
    }
    OGC_REQUIRE(V <= 0x7fffffff / 3, "%s: V = %d beyond 32-bit indexing of the coordinates", name, V);
    View v;
    if (!dr_view(name, view, v)) return OGC_ERR_INVALID_ARG;
    OGC_REQUIRE(depth && face && status, "%s: null pointer (depth, face or status)", name);
    OGC_REQUIRE(F == 0 || (faces && (V == 0 || vertices)), "%s: null pointer (vertices or faces)", name);
    OGC_REQUIRE(F == 0 || (ws && ws_bytes >= ogc_depth_render_ws_bytes(F) && ((uintptr_t)ws & 255) == 0),
                "%s: the workspace needs %lld bytes, 256-byte aligned (%lld given)", name, ogc_depth_render_ws_bytes(F), ws_bytes);
    if (ev) (void)hipEventRecord(ev[0], s);
    if (ogc_zero_async(status, 3 * sizeof(int), s) != hipSuccess) {
        ogc_set_error("%s: could not clear the status", name);
        return OGC_ERR_LAUNCH;
    }
    const long long n = (long long)width * height;
    const int tiles = ogc_divup(F, DR_THREADS);
    char *base = static_cast<char *>(ws);
    FaceRec *rec = reinterpret_cast<FaceRec *>(base);
    long long *item_start = reinterpret_cast<long long *>(base + dr_align((size_t)F * sizeof(FaceRec)));
    long long *tile_items =
        reinterpret_cast<long long *>(base + dr_align((size_t)F * sizeof(FaceRec)) + dr_align(((size_t)F + 1) * sizeof(long long)));
    if (F > 0) {
        hipLaunchKernelGGL(dr_setup_kernel, dim3(tiles), dim3(DR_THREADS), 0, s, V, F, vertices, faces, v, width, height, rec, tile_items,
                           status);
        OGC_CHECK_LAUNCH(name);
        hipLaunchKernelGGL(dr_offsets_kernel, dim3(tiles), dim3(DR_THREADS), 0, s, F, rec, tile_items, item_start);
        OGC_CHECK_LAUNCH(name);
    }
    unsigned long long *bits = reinterpret_cast<unsigned long long *>(depth);
    unsigned *uface = reinterpret_cast<unsigned *>(face);
    const int init_groups = ogc_divup(n, DR_THREADS) < 2048 ? ogc_divup(n, DR_THREADS) : 2048;
    hipLaunchKernelGGL(dr_init_kernel, dim3(init_groups), dim3(DR_THREADS), 0, s, n, bits, face, status);
    OGC_CHECK_LAUNCH(name);
    if (ev) (void)hipEventRecord(ev[1], s);
    if (F > 0) {
        hipLaunchKernelGGL(dr_small_kernel<0>, dim3(tiles), dim3(DR_THREADS), 0, s, F, rec, v, width, bits, uface, status);
        OGC_CHECK_LAUNCH(name);
        hipLaunchKernelGGL(dr_large_kernel<0>, dim3(DR_LARGE_GROUPS), dim3(DR_THREADS), 0, s, F, rec, item_start, v, width, bits, uface,
                           status);
        OGC_CHECK_LAUNCH(name);
    }
    if (ev) (void)hipEventRecord(ev[2], s);
    if (F > 0) {
        hipLaunchKernelGGL(dr_small_kernel<1>, dim3(tiles), dim3(DR_THREADS), 0, s, F, rec, v, width, bits, uface, status);
        OGC_CHECK_LAUNCH(name);
        hipLaunchKernelGGL(dr_large_kernel<1>, dim3(DR_LARGE_GROUPS), dim3(DR_THREADS), 0, s, F, rec, item_start, v, width, bits, uface,
                           status);
        OGC_CHECK_LAUNCH(name);
    }
    if (ev) (void)hipEventRecord(ev[3], s);
    return OGC_OK;
}

extern "C" int ogc_depth_render(int V, int F, const double *vertices, const int *faces, const double *view, int width, int height,
                                double *depth, int *face, int *status, void *ws, long long ws_bytes, ogc_stream_t stream) {
    return dr_render("ogc_depth_render", V, F, vertices, faces, view, width, height, depth, face, status, ws, ws_bytes, (hipStream_t)stream,
                     nullptr);
}

extern "C" int ogc_depth_render_timed(int V, int F, const double *vertices, const int *faces, const double *view, int width, int height,
                                      double *depth, int *face, int *status, void *ws, long long ws_bytes, float *stage_ms,
                                      ogc_stream_t stream) {
    const char *name = "ogc_depth_render_timed";
    OGC_REQUIRE(stage_ms != nullptr, "%s: null pointer (stage_ms)", name);
    hipEvent_t ev[4];
    int made = 0;
    while (made < 4 && hipEventCreate(&ev[made]) == hipSuccess) ++made;
    int rc = OGC_ERR_LAUNCH;
    if (made < 4) {
        ogc_set_error("%s: could not create the events", name);
    } else {
        rc = dr_render(name, V, F, vertices, faces, view, width, height, depth, face, status, ws, ws_bytes, (hipStream_t)stream, ev);
        if (rc == OGC_OK) {
            bool ok = hipEventSynchronize(ev[3]) == hipSuccess;
            for (int k = 0; k < 3 && ok; ++k) ok = hipEventElapsedTime(&stage_ms[k], ev[k], ev[k + 1]) == hipSuccess;
            if (!ok) {
                ogc_set_error("%s: could not read the events", name);
                rc = OGC_ERR_LAUNCH;
            }
        }
    }
    for (int k = 0; k < made; ++k) (void)hipEventDestroy(ev[k]);
    return rc;
}

extern "C" int ogc_depth_points(int width, int height, const double *view, const double *depth, const int *face, float *points,
                                int *pixel, int *face_out, int *status, ogc_stream_t stream) {
    const char *name = "ogc_depth_points";
    OGC_REQUIRE(width >= 1 && height >= 1 && width <= DR_MAX_SIDE && height <= DR_MAX_SIDE,
                "%s: the image is %d x %d, each side must be in 1..%d", name, width, height, DR_MAX_SIDE);
    View v;
    if (!dr_view(name, view, v)) return OGC_ERR_INVALID_ARG;
    OGC_REQUIRE(depth && face && points && pixel && face_out && status, "%s: null pointer", name);
    hipStream_t s = (hipStream_t)stream;
    const long long n = (long long)width * height;
    const int tiles = ogc_divup(n, DR_TILE);
    int *tile_count = static_cast<int *>(ogc_workspace(s, (size_t)tiles * sizeof(int)));
    if (!tile_count) {
        ogc_set_error("%s: no workspace for the tile counts", name);
        return OGC_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(dr_count_kernel, dim3(tiles), dim3(DR_THREADS), 0, s, n, face, tile_count, status);
    OGC_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(dr_scatter_kernel, dim3(tiles), dim3(DR_THREADS), 0, s, n, width, v, depth, face, tile_count, points, pixel, face_out,
                       status);
    OGC_CHECK_LAUNCH(name);
    return OGC_OK;
}

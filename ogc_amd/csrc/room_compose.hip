// room_compose.hip — the scene composition of the OGC-DR preparation, fp64: where the objects of a room stand in every
// frame.  Replaces the pose and location loops of data_prepare/ogcdr/build_ogcdr.py:130-320 and :438-470 with a counter-based form:
// every draw is a function of (seed, attempt, object, frame, failure count, stream), so the sequential rejection rule "first accepted
// attempt" is evaluated 64 attempts at a time and the lowest accepted index taken from the ballot.  include/ogc_ops.h holds the
// definition; tests/ogcdr_compose_cases.py repeats it in numpy with sequential loops.
//
//   ogc_room_compose      one workgroup per trial scene.  Per frame try: thread k turns object k (one Philox block or two, the
//                         degree sine / cosine below, one 3 x 3 product); all wavefronts walk the vertices of the trial's objects
//                         for the six extremes of every object under its rotation (wave shuffles, then one combine through LDS);
//                         wavefront 0 places the objects in index order, the boxes placed so far held one per lane.
//   ogc_mesh_apply_poses  one thread per vertex and frame: R v + t.
// Everything is one rounding per operation: the file is compiled with -ffp-contract=off and says so again per function.
#include <math.h>

#include "ogc_common.h"
#include "philox.h"

namespace {

constexpr int RC_THREADS = 256;
constexpr int RC_WAVES = RC_THREADS / OGC_WAVE;
constexpr int RC_CHECK_THREADS = 1024;
constexpr int RC_MAX_OBJECTS = OGC_ROOM_MAX_OBJECTS;
constexpr int AP_THREADS = 256;

struct RoomConst { // OGC_ROOM_DOUBLES doubles and OGC_ROOM_INTS ints in this order
    double ground, wall, y_lo, y_hi, mot_y_lo, mot_y_hi, mot_xz_lo, mot_xz_hi, prob_y, shift_lo, shift_hi;
    int n_frame, max_iter, max_retry;
};

// sine and cosine of an angle in degrees, defined by this sequence alone (include/ogc_ops.h): the quadrant is taken off exactly, the
// rest, |r| <= 45, goes through the Taylor polynomials of degree 17 and 16 with coefficients rounded to double.
__device__ __forceinline__ void sincos_deg(double a, double &sn, double &cs) {
#pragma clang fp contract(off)
    constexpr double S[8] = {-1.0 / 6.0, 1.0 / 120.0, -1.0 / 5040.0, 1.0 / 362880.0, -1.0 / 39916800.0, 1.0 / 6227020800.0,
                             -1.0 / 1307674368000.0, 1.0 / 355687428096000.0};
    constexpr double C[8] = {-1.0 / 2.0, 1.0 / 24.0, -1.0 / 720.0, 1.0 / 40320.0, -1.0 / 3628800.0, 1.0 / 479001600.0,
                             -1.0 / 87178291200.0, 1.0 / 20922789888000.0};
    const double q = rint(a / 90.0);
    const double r = a - 90.0 * q;
    const double t = r * 0x1.1df46a2529d39p-6; // the double nearest pi / 180
    const double s = t * t;
    double ps = S[7], pc = C[7];
#pragma unroll
    for (int k = 6; k >= 0; --k) {
        ps = S[k] + s * ps;
        pc = C[k] + s * pc;
    }
    const double st = t + t * (s * ps), ct = 1.0 + s * pc;
    switch ((int)((long long)q & 3)) {
    case 0: sn = st; cs = ct; break;
    case 1: sn = ct; cs = -st; break;
    case 2: sn = -st; cs = -ct; break;
    default: sn = -ct; cs = st; break;
    }
}

// scipy's Rotation.from_euler on one lower-case axis (0 x, 1 y, 2 z), row-major
__device__ __forceinline__ void axis_rotation(int axis, double sn, double cs, double (&r)[9]) {
    if (axis == 0) {
        r[0] = 1.0; r[1] = 0.0; r[2] = 0.0; r[3] = 0.0; r[4] = cs; r[5] = -sn; r[6] = 0.0; r[7] = sn; r[8] = cs;
    } else if (axis == 1) {
        r[0] = cs; r[1] = 0.0; r[2] = sn; r[3] = 0.0; r[4] = 1.0; r[5] = 0.0; r[6] = -sn; r[7] = 0.0; r[8] = cs;
    } else {
        r[0] = cs; r[1] = -sn; r[2] = 0.0; r[3] = sn; r[4] = cs; r[5] = 0.0; r[6] = 0.0; r[7] = 0.0; r[8] = 1.0;
    }
}

__device__ __forceinline__ double wave_min_f64(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmin(v, __shfl_xor(v, d));
    return v;
}

__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmax(v, __shfl_xor(v, d));
    return v;
}

// two xz boxes meet: build_ogcdr.py:181-189 (check_intersection_interval), the strict <
__device__ __forceinline__ bool boxes_meet(double alx, double alz, double ahx, double ahz, double blx, double blz, double bhx, double bhz) {
#pragma clang fp contract(off)
    const bool x = fabs((alx + ahx) / 2.0 - (blx + bhx) / 2.0) < ((ahx - alx) + (bhx - blx)) / 2.0;
    const bool z = fabs((alz + ahz) / 2.0 - (blz + bhz) / 2.0) < ((ahz - alz) + (bhz - blz)) / 2.0;
    return x && z;
}

// the offsets, checked by one workgroup ahead of the composition: status[t] = {4, 0} for every trial if they are not what the header
// asks for, {0, 0} otherwise.  After it the composition's reads through the offsets stay inside vertices, poses and attempt.
__global__ __launch_bounds__(RC_CHECK_THREADS) void room_check_kernel(int T, int O, int V, const int *__restrict__ vert_offsets,
                                                                      const int *__restrict__ obj_offsets, int *__restrict__ status) {
    const int tid = threadIdx.x;
    int bad = 0;
    if (tid == 0 && (vert_offsets[0] != 0 || vert_offsets[O] != V || obj_offsets[0] != 0 || obj_offsets[T] != O)) bad = 1;
    for (int o = tid; o < O; o += RC_CHECK_THREADS)
        if (vert_offsets[o + 1] <= vert_offsets[o]) bad = 1; // descending, or an object without vertices
    for (int t = tid; t < T; t += RC_CHECK_THREADS) {
        const long long n = (long long)obj_offsets[t + 1] - obj_offsets[t];
        if (n < 0 || n > RC_MAX_OBJECTS) bad = 1;
    }
    bad = __syncthreads_or(bad);
    for (int t = tid; t < T; t += RC_CHECK_THREADS) {
        status[2 * t] = bad ? 4 : 0;
        status[2 * t + 1] = 0;
    }
}

__global__ __launch_bounds__(RC_THREADS) void room_compose_kernel(const double *__restrict__ vertices, const int *__restrict__ vert_offsets,
                                                                  const int *__restrict__ obj_offsets, const double *__restrict__ room,
                                                                  const long long *__restrict__ seeds, RoomConst c,
                                                                  double *__restrict__ poses, int *__restrict__ attempt,
                                                                  int *__restrict__ fails_out, int *__restrict__ status) {
#pragma clang fp contract(off)
    __shared__ double rot_prev[RC_MAX_OBJECTS][9], rot_cur[RC_MAX_OBJECTS][9]; // the rotation of the last accepted frame, of this try
    __shared__ double t_prev[RC_MAX_OBJECTS][3], t_cur[RC_MAX_OBJECTS][3];
    __shared__ double part[RC_WAVES][RC_MAX_OBJECTS][6];                       // per wavefront: min x y z, max x y z
    __shared__ double ext[RC_MAX_OBJECTS][6];
    __shared__ int accepted[RC_MAX_OBJECTS];
    __shared__ int placed;

    const int trial = blockIdx.x, tid = threadIdx.x, lane = tid & (OGC_WAVE - 1), wave = tid / OGC_WAVE;
    if (status[2 * trial] != 0) return; // the offsets were refused
    const int o0 = obj_offsets[trial], n = obj_offsets[trial + 1] - o0;
    const int v0 = vert_offsets[o0], v1 = vert_offsets[o0 + n];

    int bad = 0;
    for (long long e = 3ll * v0 + tid; e < 3ll * v1; e += RC_THREADS)
        if (!isfinite(vertices[e])) bad = 1;
    if (tid < 2 && !isfinite(room[2 * trial + tid])) bad = 1;
    if (__syncthreads_or(bad)) {
        if (tid == 0) status[2 * trial] = 3;
        return;
    }

    const unsigned long long seed = (unsigned long long)seeds[trial];
    const uint32_t key0 = (uint32_t)(seed & 0xffffffffu), key1 = (uint32_t)(seed >> 32);
    const double room_x = room[2 * trial], room_z = room[2 * trial + 1];
    const double low_x = -room_x / 2.0 + c.wall, low_z = -room_z / 2.0 + c.wall; // the least corner a box may have

    int fails = 0;
    for (int f = 0; f < c.n_frame; ++f) {
        for (;;) { // the tries of this frame
            const uint32_t where = (uint32_t)(f * 256 + fails);
            if (tid < n) { // the turn of object tid
                const Philox4 a = philox4x32_10(0u, (uint32_t)tid, where, 0u, key0, key1);
                const double u_a = uniform53(a.w[0], a.w[1]), u_b = uniform53(a.w[2], a.w[3]);
                double sn, cs, r[9];
                if (f == 0) {
                    sincos_deg(c.y_lo + u_a * (c.y_hi - c.y_lo), sn, cs);
                    axis_rotation(1, sn, cs, r);
#pragma unroll
                    for (int e = 0; e < 9; ++e) rot_cur[tid][e] = r[e];
                } else {
                    int axis = 1;
                    double angle;
                    if (u_a < c.prob_y) {
                        angle = c.mot_y_lo + u_b * (c.mot_y_hi - c.mot_y_lo);
                    } else {
                        const Philox4 b = philox4x32_10(1u, (uint32_t)tid, where, 0u, key0, key1);
                        angle = c.mot_xz_lo + u_b * (c.mot_xz_hi - c.mot_xz_lo);
                        axis = uniform53(b.w[0], b.w[1]) < 0.5 ? 0 : 2;
                    }
                    sincos_deg(angle, sn, cs);
                    axis_rotation(axis, sn, cs, r);
#pragma unroll
                    for (int i = 0; i < 3; ++i)
#pragma unroll
                        for (int j = 0; j < 3; ++j)
                            rot_cur[tid][3 * i + j] = (r[3 * i] * rot_prev[tid][j] + r[3 * i + 1] * rot_prev[tid][3 + j]) + r[3 * i + 2] * rot_prev[tid][6 + j];
                }
            }
            __syncthreads();

            for (int k = 0; k < n; ++k) { // the extremes of object k under its rotation
                double R[9];
#pragma unroll
                for (int e = 0; e < 9; ++e) R[e] = rot_cur[k][e];
                double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
                const int b = vert_offsets[o0 + k], e = vert_offsets[o0 + k + 1];
                for (int v = b + tid; v < e; v += RC_THREADS) {
                    const double x = vertices[(size_t)v * 3], y = vertices[(size_t)v * 3 + 1], z = vertices[(size_t)v * 3 + 2];
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        const double p = (R[3 * i] * x + R[3 * i + 1] * y) + R[3 * i + 2] * z;
                        mn[i] = fmin(mn[i], p);
                        mx[i] = fmax(mx[i], p);
                    }
                }
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    mn[i] = wave_min_f64(mn[i]);
                    mx[i] = wave_max_f64(mx[i]);
                }
                if (lane == 0) {
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        part[wave][k][i] = mn[i];
                        part[wave][k][3 + i] = mx[i];
                    }
                }
            }
            __syncthreads();
            if (tid < 6 * n) {
                const int k = tid / 6, i = tid % 6;
                double v = part[0][k][i];
#pragma unroll
                for (int w = 1; w < RC_WAVES; ++w) v = i < 3 ? fmin(v, part[w][k][i]) : fmax(v, part[w][k][i]);
                ext[k][i] = v + 0.0; // a zero extreme counts as +0, whichever vertex gave it
            }
            __syncthreads();

            if (wave == 0) { // the places, in index order; lane j keeps the box of object j of this try
                double box_lx = 0.0, box_lz = 0.0, box_hx = 0.0, box_hz = 0.0;
                int ok = 1;
                for (int k = 0; k < n; ++k) {
                    const double min_x = ext[k][0], min_y = ext[k][1], min_z = ext[k][2], max_x = ext[k][3], max_z = ext[k][5];
                    double b_x, b_z, lo_x = 0.0, lo_z = 0.0, len_x = 0.0, len_z = 0.0, up_x = 0.0, up_z = 0.0;
                    if (f == 0) {
                        b_x = max_x - min_x;
                        b_z = max_z - min_z;
                        len_x = (room_x - b_x) - 2.0 * c.wall;
                        len_z = (room_z - b_z) - 2.0 * c.wall;
                    } else {
                        lo_x = min_x + t_prev[k][0];
                        lo_z = min_z + t_prev[k][2];
                        b_x = (max_x + t_prev[k][0]) - lo_x;
                        b_z = (max_z + t_prev[k][2]) - lo_z;
                        up_x = (room_x / 2.0 - c.wall) - b_x;
                        up_z = (room_z / 2.0 - c.wall) - b_z;
                    }
                    int found = -1;
                    double loc_x = 0.0, loc_z = 0.0, d_x = 0.0, d_z = 0.0;
                    for (int base = 0; base < c.max_iter; base += OGC_WAVE) {
                        const int i = base + lane;
                        bool good = i < c.max_iter;
                        const Philox4 p = philox4x32_10((uint32_t)i, (uint32_t)k, where, 1u, key0, key1);
                        const double u_x = uniform53(p.w[0], p.w[1]), u_z = uniform53(p.w[2], p.w[3]);
                        double l_x, l_z, s_x = 0.0, s_z = 0.0;
                        if (f == 0) {
                            l_x = low_x + u_x * len_x;
                            l_z = low_z + u_z * len_z;
                        } else {
                            const Philox4 g = philox4x32_10((uint32_t)i, (uint32_t)k, where, 2u, key0, key1);
                            s_x = c.shift_lo + u_x * (c.shift_hi - c.shift_lo);
                            s_z = c.shift_lo + u_z * (c.shift_hi - c.shift_lo);
                            if (!(uniform53(g.w[0], g.w[1]) < 0.5)) s_x = -s_x;
                            if (!(uniform53(g.w[2], g.w[3]) < 0.5)) s_z = -s_z;
                            l_x = lo_x + s_x;
                            l_z = lo_z + s_z;
                            if (l_x < low_x || l_x > up_x || l_z < low_z || l_z > up_z) good = false;
                        }
                        const double h_x = l_x + b_x, h_z = l_z + b_z;
                        for (int j = 0; j < k; ++j) // every lane takes part in the shuffles: k is the same in all of them
                            if (boxes_meet(l_x, l_z, h_x, h_z, __shfl(box_lx, j), __shfl(box_lz, j), __shfl(box_hx, j), __shfl(box_hz, j)))
                                good = false;
                        const unsigned long long mask = __ballot(good);
                        if (mask != 0ull) {
                            const int src = __ffsll((long long)mask) - 1;
                            found = base + src;
                            loc_x = __shfl(l_x, src);
                            loc_z = __shfl(l_z, src);
                            d_x = __shfl(s_x, src);
                            d_z = __shfl(s_z, src);
                            break;
                        }
                    }
                    if (found < 0) {
                        ok = 0;
                        break;
                    }
                    if (lane == k) {
                        box_lx = loc_x;
                        box_lz = loc_z;
                        box_hx = loc_x + b_x;
                        box_hz = loc_z + b_z;
                    }
                    if (lane == 0) {
                        t_cur[k][0] = f == 0 ? loc_x - min_x : t_prev[k][0] + d_x;
                        t_cur[k][1] = c.ground - min_y;
                        t_cur[k][2] = f == 0 ? loc_z - min_z : t_prev[k][2] + d_z;
                        accepted[k] = found;
                    }
                }
                if (lane == 0) placed = ok;
            }
            __syncthreads();
            if (placed) break;
            if (f == 0 || fails + 1 > c.max_retry) { // nothing else reads `placed` before the next try has passed three barriers
                if (tid == 0) {
                    status[2 * trial] = f == 0 ? 1 : 2;
                    status[2 * trial + 1] = f;
                }
                return;
            }
            ++fails;
        }

        if (tid < n) { // the frame stands: it is the next frame's start and object tid's pose
            double *P = poses + ((size_t)(o0 + tid) * c.n_frame + f) * 16;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    rot_prev[tid][3 * i + j] = rot_cur[tid][3 * i + j];
                    P[4 * i + j] = rot_cur[tid][3 * i + j];
                }
                t_prev[tid][i] = t_cur[tid][i];
                P[4 * i + 3] = t_cur[tid][i];
            }
            P[12] = 0.0; P[13] = 0.0; P[14] = 0.0; P[15] = 1.0;
            attempt[(size_t)(o0 + tid) * c.n_frame + f] = accepted[tid];
        }
        if (tid == 0) fails_out[(size_t)trial * c.n_frame + f] = fails;
        __syncthreads();
    }
}

__global__ __launch_bounds__(AP_THREADS) void mesh_apply_poses_kernel(int V, int O, int n_frame, const double *__restrict__ vertices,
                                                                      const int *__restrict__ vert_offsets, const double *__restrict__ poses,
                                                                      double *__restrict__ out) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * AP_THREADS + threadIdx.x;
    if (i >= (long long)V * n_frame) return;
    const int f = (int)(i / V), v = (int)(i % V);
    const int o = ogc_owner(vert_offsets, O, v);
    const double *P = poses + ((size_t)o * n_frame + f) * 16;
    const double x = vertices[(size_t)v * 3], y = vertices[(size_t)v * 3 + 1], z = vertices[(size_t)v * 3 + 2];
#pragma unroll
    for (int r = 0; r < 3; ++r) out[(size_t)i * 3 + r] = ((P[4 * r] * x + P[4 * r + 1] * y) + P[4 * r + 2] * z) + P[4 * r + 3];
}

} // namespace

extern "C" int ogc_room_compose(int T, int O, int V, const double *vertices, const int *vert_offsets, const int *obj_offsets,
                                const double *room, const long long *seeds, const double *constants, const int *limits, double *poses,
                                int *attempt, int *fails, int *status, ogc_stream_t stream) {
    const char *name = "ogc_room_compose";
    OGC_REQUIRE(T >= 0 && O >= 0 && V >= 0, "%s: negative size (T = %d, O = %d, V = %d)", name, T, O, V);
    OGC_REQUIRE(V <= 0x7fffffff / 3, "%s: V = %d, 3 * V must fit 32-bit indexing", name, V);
    OGC_REQUIRE(T <= 0x7fffffff / 2, "%s: T = %d, 2 * T must fit 32-bit indexing", name, T);
    OGC_REQUIRE(constants && limits, "%s: null pointer (constants or limits)", name);
    for (int k = 0; k < OGC_ROOM_DOUBLES; ++k)
        OGC_REQUIRE(fabs(constants[k]) <= 1.7976931348623157e308, "%s: constants[%d] is not finite", name, k);
    static_assert(OGC_ROOM_DOUBLES == 11 && OGC_ROOM_INTS == 3, "the constants are the two arrays the header describes");
    const RoomConst c = {constants[0], constants[1], constants[2], constants[3], constants[4], constants[5], constants[6], constants[7],
                         constants[8], constants[9], constants[10], limits[0], limits[1], limits[2]};
    OGC_REQUIRE(c.n_frame >= 1 && c.n_frame <= OGC_ROOM_MAX_FRAMES, "%s: n_frame = %d outside [1, %d]", name, c.n_frame, OGC_ROOM_MAX_FRAMES);
    OGC_REQUIRE(c.max_iter >= 1 && c.max_iter <= OGC_ROOM_MAX_ITER, "%s: max_iter = %d outside [1, %d]", name, c.max_iter, OGC_ROOM_MAX_ITER);
    OGC_REQUIRE(c.max_retry >= 0 && c.max_retry <= OGC_ROOM_MAX_RETRY, "%s: max_retry = %d outside [0, %d]", name, c.max_retry, OGC_ROOM_MAX_RETRY);
    if (T == 0) return OGC_OK;
    OGC_REQUIRE((vertices || V == 0) && vert_offsets && obj_offsets && room && seeds, "%s: null pointer (vertices, offsets, room or seeds)", name);
    OGC_REQUIRE(((poses && attempt) || O == 0) && fails && status, "%s: null pointer (poses, attempt, fails or status)", name);
    hipLaunchKernelGGL(room_check_kernel, dim3(1), dim3(RC_CHECK_THREADS), 0, (hipStream_t)stream, T, O, V, vert_offsets, obj_offsets, status);
    OGC_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(room_compose_kernel, dim3((unsigned)T), dim3(RC_THREADS), 0, (hipStream_t)stream, vertices, vert_offsets, obj_offsets,
                       room, seeds, c, poses, attempt, fails, status);
    OGC_CHECK_LAUNCH(name);
    return OGC_OK;
}

extern "C" int ogc_mesh_apply_poses(int V, int O, int n_frame, const double *vertices, const int *vert_offsets, const double *poses,
                                    double *out, ogc_stream_t stream) {
    const char *name = "ogc_mesh_apply_poses";
    OGC_REQUIRE(V >= 0 && O >= 0 && n_frame >= 0, "%s: negative size (V = %d, O = %d, n_frame = %d)", name, V, O, n_frame);
    OGC_REQUIRE((long long)V * n_frame <= 0x7fffffffLL / 3, "%s: V * n_frame = %lld, 3 * V * n_frame must fit 32-bit indexing", name,
                (long long)V * n_frame);
    if (V == 0 || n_frame == 0) return OGC_OK;
    OGC_REQUIRE(O >= 1, "%s: %d vertices need an object (O = %d)", name, V, O);
    OGC_REQUIRE(vertices && vert_offsets && poses && out, "%s: null pointer (vertices, vert_offsets, poses or out)", name);
    hipLaunchKernelGGL(mesh_apply_poses_kernel, dim3((unsigned)ogc_divup((long long)V * n_frame, AP_THREADS)), dim3(AP_THREADS), 0,
                       (hipStream_t)stream, V, O, n_frame, vertices, vert_offsets, poses, out);
    OGC_CHECK_LAUNCH(name);
    return OGC_OK;
}

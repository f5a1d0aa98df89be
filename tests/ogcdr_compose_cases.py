"""Helpers of the scene-composition tests (no tests here): the float64 mirror of ogc_room_compose and ogc_mesh_apply_poses as
include/ogc_ops.h defines them, with SEQUENTIAL attempt loops in Python floats — IEEE doubles, one rounding per
operation —, the mirror of the degree sine / cosine, and the case builders the CPU and the GPU files share."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ogcdr_prepare_cases import philox4x32_10, uniform53  # noqa: E402

K_DEG = float.fromhex("0x1.1df46a2529d39p-6")     # the double nearest pi / 180
SIN_COEF = [(-1.0) ** k / float(math.factorial(2 * k + 1)) for k in range(1, 9)]    # an exact integer divided: rounded once
COS_COEF = [(-1.0) ** k / float(math.factorial(2 * k)) for k in range(1, 9)]

# the reference's constants (build_ogcdr.py:51-67) under the names mesh_ops.compose_rooms takes
DEFAULTS = dict(ground_level=-0.5 + 0.01, wall_thickness=0.01, y_angle_lo=0.0, y_angle_hi=360.0, mot_y_angle_lo=-10.0, mot_y_angle_hi=10.0,
                mot_xz_angle_lo=-10.0, mot_xz_angle_hi=10.0, prob_rotation_y=0.6, mot_transl_lo=0.02, mot_transl_hi=0.04,
                n_frame=4, max_iter=1000, max_retry=20)
MAX_OBJECTS = 32


def sincos_deg(a):
    """The defined sine and cosine of a degrees -> (sin, cos): Python floats for a number, float64 arrays for an array."""
    a = np.asarray(a, dtype=np.float64)
    q = np.rint(a / 90.0)
    r = a - 90.0 * q
    t = r * K_DEG
    s = t * t
    ps, pc = SIN_COEF[7], COS_COEF[7]
    for k in range(6, -1, -1):
        ps = SIN_COEF[k] + s * ps
        pc = COS_COEF[k] + s * pc
    st = t + t * (s * ps)
    ct = 1.0 + s * pc
    k = q.astype(np.int64) % 4
    sn, cs = np.choose(k, [st, ct, -st, -ct]), np.choose(k, [ct, -st, -ct, st])
    return (float(sn), float(cs)) if a.ndim == 0 else (sn, cs)


def axis_rotation(axis, sn, cs):
    """scipy's Rotation.from_euler on one lower-case axis -> (3, 3) float64."""
    if axis == 0:
        return np.array([[1.0, 0.0, 0.0], [0.0, cs, -sn], [0.0, sn, cs]])
    if axis == 1:
        return np.array([[cs, 0.0, sn], [0.0, 1.0, 0.0], [-sn, 0.0, cs]])
    return np.array([[cs, -sn, 0.0], [sn, cs, 0.0], [0.0, 0.0, 1.0]])


def compose_rotation(r, R):
    """r R with every entry ((r_i0 * R_0j + r_i1 * R_1j) + r_i2 * R_2j)."""
    return (r[:, 0:1] * R[0:1, :] + r[:, 1:2] * R[1:2, :]) + r[:, 2:3] * R[2:3, :]


def rotate(R, vertices):
    """(V, 3): per axis ((R_i0 * x + R_i1 * y) + R_i2 * z)."""
    x, y, z = vertices[:, 0:1], vertices[:, 1:2], vertices[:, 2:3]
    return (R[None, :, 0] * x + R[None, :, 1] * y) + R[None, :, 2] * z


def extremes(R, vertices):
    p = rotate(R, vertices)
    return p.min(0) + 0.0, p.max(0) + 0.0       # a zero extreme counts as +0


class Draws:
    """The uniforms of one (trial seed, object, frame * 256 + fails, stream), drawn 1024 attempts at a time when first asked for."""

    def __init__(self, seed, obj, where, stream):
        seed = int(seed) & 0xffffffffffffffff
        self.key, self.obj, self.where, self.stream, self.blocks = (seed & 0xffffffff, seed >> 32), obj, where, stream, {}

    def __call__(self, attempt):
        block = attempt >> 10
        if block not in self.blocks:
            i = np.arange(block << 10, (block + 1) << 10, dtype=np.uint64)
            fill = np.zeros(1024, dtype=np.uint64)
            w = philox4x32_10((i, fill + np.uint64(self.obj), fill + np.uint64(self.where), fill + np.uint64(self.stream)), self.key)
            self.blocks[block] = (uniform53(w[0], w[1]).tolist(), uniform53(w[2], w[3]).tolist())
        first, second = self.blocks[block]
        return first[attempt & 1023], second[attempt & 1023]


def boxes_meet(a, b):
    """a, b: (lo_x, lo_z, hi_x, hi_z) -> check_intersection_interval, the strict <."""
    in_x = abs((a[0] + a[2]) / 2.0 - (b[0] + b[2]) / 2.0) < ((a[2] - a[0]) + (b[2] - b[0])) / 2.0
    in_z = abs((a[1] + a[3]) / 2.0 - (b[1] + b[3]) / 2.0) < ((a[3] - a[1]) + (b[3] - b[1])) / 2.0
    return in_x and in_z


def offsets_refused(vert_offsets, obj_offsets, n_vertex):
    vo, oo = np.asarray(vert_offsets, dtype=np.int64), np.asarray(obj_offsets, dtype=np.int64)
    n_object = len(vo) - 1
    return bool(vo[0] != 0 or vo[-1] != n_vertex or oo[0] != 0 or oo[-1] != n_object or (np.diff(vo) <= 0).any()
                or (np.diff(oo) < 0).any() or (np.diff(oo) > MAX_OBJECTS).any())


def compose_trial(meshes, room, seed, c):
    """One trial: meshes a list of (V_k, 3) float64, room (2,), seed -> (code, frame, poses (n, n_frame, 4, 4), attempt (n, n_frame),
    fails (n_frame,)); what a non-zero code leaves in the other three is not part of the contract."""
    n, n_frame = len(meshes), c["n_frame"]
    poses, attempt, fails_at = np.zeros((n, n_frame, 4, 4)), np.zeros((n, n_frame), dtype=np.int32), np.zeros(n_frame, dtype=np.int32)
    if not all(np.isfinite(m).all() for m in meshes) or not np.isfinite(room).all():
        return 3, 0, poses, attempt, fails_at
    room = [float(room[0]), float(room[1])]
    wall, ground = float(c["wall_thickness"]), float(c["ground_level"])
    low = [-room[0] / 2.0 + wall, -room[1] / 2.0 + wall]
    rot_prev, t_prev = [None] * n, [None] * n
    fails = 0
    for f in range(n_frame):
        while True:
            where = f * 256 + fails
            rot, t_cur, boxes, accepted, ok = [], [], [], [], True
            for k in range(n):
                draw = Draws(seed, k, where, 0)
                u_a, u_b = draw(0)
                if f == 0:
                    rot.append(axis_rotation(1, *sincos_deg(c["y_angle_lo"] + u_a * (c["y_angle_hi"] - c["y_angle_lo"]))))
                else:
                    if u_a < c["prob_rotation_y"]:
                        axis, angle = 1, c["mot_y_angle_lo"] + u_b * (c["mot_y_angle_hi"] - c["mot_y_angle_lo"])
                    else:
                        angle = c["mot_xz_angle_lo"] + u_b * (c["mot_xz_angle_hi"] - c["mot_xz_angle_lo"])
                        axis = 0 if draw(1)[0] < 0.5 else 2
                    rot.append(compose_rotation(axis_rotation(axis, *sincos_deg(angle)), rot_prev[k]))
            for k in range(n):
                mn, mx = extremes(rot[k], meshes[k])
                mn, mx = mn.tolist(), mx.tolist()
                place, sign = Draws(seed, k, where, 1), Draws(seed, k, where, 2)
                if f == 0:
                    b = [mx[0] - mn[0], mx[2] - mn[2]]
                    length = [(room[0] - b[0]) - 2.0 * wall, (room[1] - b[1]) - 2.0 * wall]
                else:
                    lo = [mn[0] + t_prev[k][0], mn[2] + t_prev[k][2]]
                    b = [(mx[0] + t_prev[k][0]) - lo[0], (mx[2] + t_prev[k][2]) - lo[1]]
                    up = [(room[0] / 2.0 - wall) - b[0], (room[1] / 2.0 - wall) - b[1]]
                found = -1
                for i in range(c["max_iter"]):              # the sequential rule: the first attempt that is accepted
                    u = place(i)
                    if f == 0:
                        d = [0.0, 0.0]
                        loc = [low[0] + u[0] * length[0], low[1] + u[1] * length[1]]
                    else:
                        g = sign(i)
                        d = [c["mot_transl_lo"] + u[e] * (c["mot_transl_hi"] - c["mot_transl_lo"]) for e in range(2)]
                        d = [d[e] if g[e] < 0.5 else -d[e] for e in range(2)]
                        loc = [lo[0] + d[0], lo[1] + d[1]]
                        if loc[0] < low[0] or loc[0] > up[0] or loc[1] < low[1] or loc[1] > up[1]:
                            continue
                    box = (loc[0], loc[1], loc[0] + b[0], loc[1] + b[1])
                    if any(boxes_meet(box, other) for other in boxes):
                        continue
                    found = i
                    break
                if found < 0:
                    ok = False
                    break
                boxes.append(box)
                accepted.append(found)
                t_y = ground - mn[1]
                t_cur.append([loc[0] - mn[0], t_y, loc[1] - mn[2]] if f == 0 else [t_prev[k][0] + d[0], t_y, t_prev[k][2] + d[1]])
            if ok:
                break
            if f == 0:
                return 1, 0, poses, attempt, fails_at
            if fails + 1 > c["max_retry"]:
                return 2, f, poses, attempt, fails_at
            fails += 1
        for k in range(n):
            poses[k, f] = np.eye(4)
            poses[k, f, :3, :3], poses[k, f, :3, 3] = rot[k], t_cur[k]
            attempt[k, f] = accepted[k]
        rot_prev, t_prev = rot, t_cur
        fails_at[f] = fails
    return 0, 0, poses, attempt, fails_at


def compose_mirror(vertices, vert_offsets, obj_offsets, room, seeds, **constants):
    """The mirror of ogc_room_compose -> dict(poses (O, n_frame, 4, 4), attempt (O, n_frame), fails (T, n_frame), status (T, 2))."""
    c = dict(DEFAULTS, **constants)
    n_object, n_trial, n_frame = len(vert_offsets) - 1, len(obj_offsets) - 1, c["n_frame"]
    out = dict(poses=np.zeros((n_object, n_frame, 4, 4)), attempt=np.zeros((n_object, n_frame), dtype=np.int32),
               fails=np.zeros((n_trial, n_frame), dtype=np.int32), status=np.zeros((n_trial, 2), dtype=np.int32))
    if offsets_refused(vert_offsets, obj_offsets, len(vertices)):
        out["status"][:, 0] = 4
        return out
    for t in range(n_trial):
        o0, o1 = int(obj_offsets[t]), int(obj_offsets[t + 1])
        meshes = [vertices[int(vert_offsets[o]):int(vert_offsets[o + 1])] for o in range(o0, o1)]
        code, frame, poses, attempt, fails = compose_trial(meshes, np.asarray(room[t]), int(seeds[t]), c)
        out["status"][t] = code, frame
        out["poses"][o0:o1], out["attempt"][o0:o1], out["fails"][t] = poses, attempt, fails
    return out


def apply_poses_mirror(vertices, vert_offsets, poses):
    """The mirror of ogc_mesh_apply_poses -> (n_frame, V, 3) float64: ((R_i0 * x + R_i1 * y) + R_i2 * z) + t_i."""
    out = np.zeros((poses.shape[1], len(vertices), 3))
    for o in range(len(vert_offsets) - 1):
        lo, hi = int(vert_offsets[o]), int(vert_offsets[o + 1])
        for f in range(poses.shape[1]):
            out[f, lo:hi] = rotate(poses[o, f, :3, :3], vertices[lo:hi]) + poses[o, f, :3, 3][None]
    return out


def compare_composed(got, want):
    """Bit equality of everything the contract fixes: the status of every trial, and poses, attempt and fails of the composed ones.
    got, want: dicts as compose_mirror returns, plus obj_offsets under that key in `want`."""
    assert np.array_equal(got["status"], want["status"])
    oo = want["obj_offsets"]
    for t in np.nonzero(want["status"][:, 0] == 0)[0]:
        o0, o1 = int(oo[t]), int(oo[t + 1])
        assert np.array_equal(got["fails"][t], want["fails"][t]), t
        assert np.array_equal(got["attempt"][o0:o1], want["attempt"][o0:o1]), t
        assert np.array_equal(got["poses"][o0:o1].view(np.uint64), want["poses"][o0:o1].view(np.uint64)), t


# ---- case builders ----------------------------------------------------------------------------------------------------------------

def box_object(rs, scale_lo, scale_hi):
    """A box of 8 vertices around the origin with a slim footprint: the longest edge drawn in [scale_lo, scale_hi] along x, the z
    edge 0.3 .. 0.8 of it, the height 0.2 .. 0.4 of it."""
    s = scale_lo + rs.rand() * (scale_hi - scale_lo)
    size = np.array([s, s * (0.2 + 0.2 * rs.rand()), s * (0.3 + 0.5 * rs.rand())])
    return np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)], dtype=np.float64) * size


def cloud_object(rs, count, scale):
    """`count` vertices inside a slim box of longest edge `scale`: the reduction's edges (1, 257, 1000 vertices)."""
    return (rs.rand(count, 3) - 0.5) * np.array([scale, 0.3 * scale, 0.5 * scale])


def draw_room(rs):
    """build_ogcdr.py:432-434: one axis is 1, the other 0.6 .. 1."""
    short_is_z = rs.rand() > 0.5
    short = rs.rand() * 0.4 + 0.6
    return [1.0, short] if short_is_z else [short, 1.0]


def pack(trials, seed0):
    """trials: a list of (meshes, room) -> dict of the arrays ogc_room_compose takes, numpy."""
    meshes = [m for t in trials for m in t[0]]
    return dict(vertices=np.ascontiguousarray(np.concatenate(meshes, 0)) if meshes else np.zeros((0, 3)),
                vert_offsets=np.cumsum([0] + [len(m) for m in meshes]).astype(np.int32),
                obj_offsets=np.cumsum([0] + [len(t[0]) for t in trials]).astype(np.int32),
                room=np.array([t[1] for t in trials], dtype=np.float64).reshape(len(trials), 2),
                seeds=(np.arange(len(trials), dtype=np.int64) * 7919 + seed0))


def box_batch(n_trial, n_object, scale_lo, scale_hi, seed):
    rs = np.random.RandomState(seed)
    return pack([([box_object(rs, scale_lo, scale_hi) for _ in range(n_object)], draw_room(rs)) for _ in range(n_trial)], seed * 1000003)

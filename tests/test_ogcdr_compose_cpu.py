"""The scene composition of the OGC-DR preparation without a GPU: the defined degree sine / cosine against long-double
truth, the invariants of scenes composed by the float64 mirror (tests/ogcdr_compose_cases.py), the host draws, split sizes and seeds
of the driver (ogc_amd/data_prepare/build_ogcdr.py), and the bindings."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ogcdr_compose_cases as cc  # noqa: E402

from ogc_amd.data_prepare import build_ogcdr  # noqa: E402

PI_HI, PI_LO = float.fromhex("0x1.921fb54442d18p+1"), float.fromhex("0x1.1a62633145c07p-53")     # pi split in two doubles


def true_sincos(angles):
    """sin and cos of degrees in np.longdouble.  The quadrant is taken off in exact arithmetic first (as the definition does), so the
    long-double argument is at most pi / 4 and its error far below the bound under test."""
    a = np.asarray(angles, dtype=np.float64)
    q = np.rint(a / 90.0)
    r = (a - 90.0 * q).astype(np.longdouble)            # exact in float64 already
    t = r * ((np.longdouble(PI_HI) + np.longdouble(PI_LO)) / np.longdouble(180))
    s, c = np.sin(t), np.cos(t)
    k = q.astype(np.int64) % 4
    return np.choose(k, [s, c, -s, -c]), np.choose(k, [c, -s, -c, s])


def test_defined_sine_and_cosine_are_within_two_to_the_minus_52_of_the_truth():
    assert np.finfo(np.longdouble).nmant >= 63, "the truth needs a long double wider than float64"
    rs = np.random.RandomState(5)
    angles = np.concatenate([rs.rand(400000) * 360.0, rs.rand(400000) * 20.0 - 10.0, np.arange(-720, 1441) * 0.5])
    got_s, got_c = cc.sincos_deg(angles)
    want_s, want_c = true_sincos(angles)
    err = max(np.abs(got_s.astype(np.longdouble) - want_s).max(), np.abs(got_c.astype(np.longdouble) - want_c).max())
    assert all(cc.sincos_deg(float(a)) == (s, c) for a, s, c in zip(angles[::9973], got_s[::9973], got_c[::9973]))    # number == array
    print("largest error of the defined sine / cosine: %.3f x 2^-53" % float(err * 2.0 ** 53))
    assert err <= 2.0 ** -52
    # the quadrant's exact values
    for a, s, c in ((0.0, 0.0, 1.0), (90.0, 1.0, 0.0), (180.0, 0.0, -1.0), (270.0, -1.0, 0.0), (360.0, 0.0, 1.0), (-90.0, -1.0, 0.0)):
        assert cc.sincos_deg(a) == (s, c)
    # the remainder is exact: a - 90 q is representable wherever the composition asks
    q = np.rint(angles / 90.0)
    assert np.array_equal((angles - 90.0 * q).astype(np.longdouble), angles.astype(np.longdouble) - 90 * q.astype(np.longdouble))


def test_axis_rotations_are_scipys_from_euler():
    from scipy.spatial.transform import Rotation
    for axis, letter in enumerate("xyz"):
        for angle in (-10.0, 3.7, 123.4, 359.0):
            want = Rotation.from_euler(letter, [angle], degrees=True).as_matrix()[0]
            assert np.abs(cc.axis_rotation(axis, *cc.sincos_deg(angle)) - want).max() < 1e-15


@pytest.fixture(scope="module")
def composed():
    batch = cc.box_batch(40, 3, 0.25, 0.45, 21)
    return batch, cc.compose_mirror(batch["vertices"], batch["vert_offsets"], batch["obj_offsets"], batch["room"], batch["seeds"])


def test_composed_scenes_keep_the_invariants(composed):
    batch, out = composed
    c = cc.DEFAULTS
    good = np.nonzero(out["status"][:, 0] == 0)[0]
    assert len(good) >= 10 and (out["fails"][good] >= 1).any()
    frames = cc.apply_poses_mirror(batch["vertices"], batch["vert_offsets"], out["poses"])
    for t in good:
        room = batch["room"][t]
        inner = room / 2.0 - c["wall_thickness"]
        o0, o1 = batch["obj_offsets"][t], batch["obj_offsets"][t + 1]
        for f in range(c["n_frame"]):
            boxes = []
            for o in range(o0, o1):
                v = frames[f, batch["vert_offsets"][o]:batch["vert_offsets"][o + 1]]
                assert abs(v[:, 1].min() - c["ground_level"]) <= 1e-12
                lo, hi = v[:, [0, 2]].min(0), v[:, [0, 2]].max(0)
                assert (lo >= -inner - 1e-12).all() and (hi <= inner + 1e-12).all()
                for other_lo, other_hi in boxes:
                    assert ((lo >= other_hi - 1e-12) | (other_lo >= hi - 1e-12)).any()
                boxes.append((lo, hi))
                pose = out["poses"][o, f]
                assert np.array_equal(pose[3], [0.0, 0.0, 0.0, 1.0])
                assert np.abs(pose[:3, :3] @ pose[:3, :3].T - np.eye(3)).max() < 1e-14
                if f > 0:
                    last = out["poses"][o, f - 1]
                    shift = np.abs(pose[[0, 2], 3] - last[[0, 2], 3])
                    assert (shift >= 0.02 - 1e-12).all() and (shift <= 0.04 + 1e-12).all()
                    relative = pose[:3, :3] @ last[:3, :3].T
                    angle = np.degrees(np.arccos(np.clip((np.trace(relative) - 1.0) / 2.0, -1.0, 1.0)))
                    assert angle <= 10.0 + 1e-6
                else:
                    assert pose[1, 0] == 0.0 and pose[1, 2] == 0.0 and pose[1, 1] == 1.0         # frame 0 turns about y
        assert (np.diff(out["fails"][t]) >= 0).all() and out["fails"][t, 0] == 0 and out["fails"][t].max() <= c["max_retry"]


def test_one_seed_one_scene_and_the_attempt_is_the_first_accepted():
    batch = cc.box_batch(6, 3, 0.25, 0.45, 22)
    args = (batch["vertices"], batch["vert_offsets"], batch["obj_offsets"], batch["room"])
    a, b = cc.compose_mirror(*args, batch["seeds"]), cc.compose_mirror(*args, batch["seeds"])
    other = cc.compose_mirror(*args, batch["seeds"] + 1)
    assert all(np.array_equal(a[k], b[k]) for k in a) and not np.array_equal(a["poses"], other["poses"])
    # a trial alone gives what it gives in the batch: trials do not interact
    alone = cc.compose_mirror(batch["vertices"][:24], batch["vert_offsets"][:4], batch["obj_offsets"][:2], batch["room"][:1], batch["seeds"][:1])
    assert np.array_equal(alone["poses"], a["poses"][:3]) and np.array_equal(alone["status"], a["status"][:1])
    # max_iter cuts exactly at the accepted attempt
    t = int(np.nonzero(a["status"][:, 0] == 0)[0][0])
    top = int(a["attempt"][batch["obj_offsets"][t]:batch["obj_offsets"][t + 1]].max())
    one = [batch["vertices"][24 * t:24 * t + 24], np.array([0, 8, 16, 24]), np.array([0, 3]), batch["room"][t:t + 1], batch["seeds"][t:t + 1]]
    assert cc.compose_mirror(*one, max_iter=top + 1)["status"][0, 0] == 0
    if top > 0:
        assert cc.compose_mirror(*one, max_iter=top)["status"][0, 0] != 0


def test_refusals_of_the_mirror():
    batch = cc.box_batch(2, 2, 0.2, 0.3, 23)
    args = [batch[k] for k in ("vertices", "vert_offsets", "obj_offsets", "room", "seeds")]
    bad = [a.copy() for a in args]
    bad[0][9, 1] = np.inf                                           # a vertex of trial 0
    clean, refused = cc.compose_mirror(*args), cc.compose_mirror(*bad)
    assert refused["status"][0].tolist() == [3, 0] and np.array_equal(refused["status"][1], clean["status"][1])
    bad = [a.copy() for a in args]
    bad[3][1, 0] = np.nan                                           # the room of trial 1
    assert cc.compose_mirror(*bad)["status"][1].tolist() == [3, 0]
    for index, value in ((1, [0, 8, 8, 24, 32]), (1, [1, 8, 16, 24, 32]), (2, [0, 5, 4]), (2, [0, 2, 3]), (2, [1, 2, 4])):
        bad = [a.copy() for a in args]
        bad[index] = np.array(value, dtype=np.int32)
        assert cc.compose_mirror(*bad)["status"][:, 0].tolist() == [4, 4]


def test_split_sizes_seeds_and_host_draws_of_the_driver():
    assert build_ogcdr.split_sizes(1000) == [750, 50, 200] and build_ogcdr.split_sizes(4) == [3, 0, 0]
    assert build_ogcdr.split_sizes(7) == [int(.75 * 7), int(.05 * 7), int(.2 * 7)]
    assert build_ogcdr.CLASSES == ("02828884", "02933112", "03001627", "03211117", "03636649", "04256520", "04379243")
    assert build_ogcdr.N_OBJECTS == (8, 7, 6, 5, 4) and len(build_ogcdr.SCALE_INTERVALS) == 5
    assert build_ogcdr.trial_seed(0, 0, 0, 0) == 0 and build_ogcdr.trial_seed(3, 2, 1, 5) == (3 << 32) | (2 << 28) | (1 << 26) | 5
    assert build_ogcdr.trial_seed((7 << 32) | 3, 0, 0, 1) == (3 << 32) | 1            # the low 32 bits of the seed
    seeds = {build_ogcdr.trial_seed(1, t, s, j) for t in range(5) for s in range(3) for j in (0, 1, (1 << 26) - 1)}
    assert len(seeds) == 45
    with pytest.raises(ValueError):
        build_ogcdr.trial_seed(0, 0, 0, 1 << 26)
    model_files = {"b": ["m0", "m1", "m2"], "a": ["n0"]}
    rs = build_ogcdr.trial_rng(5, 1, 2, 9)
    meta = build_ogcdr.draw_trial(rs, model_files, 6, 1)
    # the frozen legacy stream, in the reference's order: two choices per object, the scales, the axis, its length, the wall height
    want = np.random.RandomState([5, 1, 2, 9])
    names = []
    for _ in range(6):
        cl = ["a", "b"][want.randint(2)]
        names.append("%s/%s" % (cl, model_files[cl][want.randint(len(model_files[cl]))]))
    assert meta["objects"] == names and meta["classes"] == [n.split("/")[0] for n in names]
    assert meta["scales"] == [0.2 + want.rand() * (0.35 - 0.2) for _ in range(6)]
    short_is_z, short = want.rand() > 0.5, want.rand() * (1. - 0.6) + 0.6
    assert meta["xz_ground_range"].tolist() == ([1., short] if short_is_z else [short, 1.])
    assert meta["wall_height"] == 0.2 + want.rand() * (0.4 - 0.2)
    again = build_ogcdr.draw_trial(build_ogcdr.trial_rng(5 + (1 << 32), 1, 2, 9), model_files, 6, 1)
    assert again["objects"] == meta["objects"] and again["scales"] == meta["scales"]
    assert build_ogcdr.draw_trial(build_ogcdr.trial_rng(5, 1, 2, 10), model_files, 6, 1)["scales"] != meta["scales"]


def test_canonical_vertices_keep_the_reference_quirk():
    v = np.array([[1.0, 2.0, 3.0], [3.0, 2.5, 3.5], [2.0, 2.2, 4.0]])
    out = build_ogcdr.canonical_vertices(v, 0.3)
    assert np.array_equal(out, v / 2.0 * 0.3 - np.array([4.0, 4.5, 7.0]) / 2)       # the centre of the UNSCALED box is taken off
    assert abs((out.max(0) - out.min(0)).max() - 0.3) < 1e-15


def test_entry_points_are_exported_bound_and_refuse_before_launching():
    from ogc_amd import _lib, pointnet2_cuda
    from ogc_amd.csrc import build as b
    from ogc_amd.data_prepare import mesh_ops
    assert "room_compose.hip" in b.SOURCES and "philox.h" in b.HEADERS
    csrc = os.path.dirname(b.__file__)
    for name in ("surface_candidates.hip", "room_compose.hip"):             # one copy of the generator: the header's
        source = open(os.path.join(csrc, name)).read()
        assert '#include "philox.h"' in source and "struct Philox4" not in source and "0xD2511F53" not in source
    lib = ctypes.CDLL(b.build())
    lib.ogc_last_error.restype = ctypes.c_char_p
    for name in ("ogc_room_compose", "ogc_mesh_apply_poses"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert callable(pointnet2_cuda.room_compose_wrapper) and callable(pointnet2_cuda.mesh_apply_poses_wrapper)
    assert list(mesh_ops.COMPOSE_DOUBLES) + list(mesh_ops.COMPOSE_INTS) == list(cc.DEFAULTS)
    assert [mesh_ops.COMPOSE_DOUBLES[k] for k in mesh_ops.COMPOSE_DOUBLES] == [cc.DEFAULTS[k] for k in mesh_ops.COMPOSE_DOUBLES]
    fn = lib.ogc_room_compose
    fn.argtypes, fn.restype = _lib.SIGNATURES["ogc_room_compose"], ctypes.c_int
    doubles = (ctypes.c_double * 11)(*[cc.DEFAULTS[k] for k in mesh_ops.COMPOSE_DOUBLES])

    def call(T, O, V, limits, constants=doubles, pointer=None):
        rc = fn(T, O, V, pointer, pointer, pointer, pointer, pointer, constants, (ctypes.c_int * 3)(*limits), pointer, pointer, pointer,
                pointer, None)
        return rc, lib.ogc_last_error().decode()
    assert call(0, 0, 0, (4, 1000, 20))[0] == 0                       # T == 0 is a no-op
    for T, O, V in ((-1, 0, 0), (0, -1, 0), (0, 0, -1)):
        assert call(T, O, V, (4, 1000, 20))[0] == -1
    for limits, word in (((9, 1000, 20), "n_frame"), ((0, 1000, 20), "n_frame"), ((4, 65537, 20), "max_iter"), ((4, 0, 20), "max_iter"),
                         ((4, 1000, 256), "max_retry"), ((4, 1000, -1), "max_retry")):
        rc, text = call(0, 0, 0, limits)
        assert rc == -1 and word in text, (limits, text)
    assert call(0, 0, 0, (8, 65536, 255))[0] == 0                     # the limits themselves are taken
    rc, text = call(0, 0, 0, (4, 1000, 20), (ctypes.c_double * 11)(*([0.0] * 8 + [float("nan")] + [0.0] * 2)))
    assert rc == -1 and "constants[8]" in text
    assert call(0, 0, 0, (4, 1000, 20), None)[0] == -1
    rc, text = call(1, 1, 8, (4, 1000, 20))                           # T > 0 with null buffers
    assert rc == -1 and "null pointer" in text
    ap = lib.ogc_mesh_apply_poses
    ap.argtypes, ap.restype = _lib.SIGNATURES["ogc_mesh_apply_poses"], ctypes.c_int
    assert ap(0, 0, 4, None, None, None, None, None) == 0 and ap(8, 1, 0, None, None, None, None, None) == 0
    assert ap(-1, 1, 4, None, None, None, None, None) == -1 and ap(8, 1, 4, None, None, None, None, None) == -1
    assert ap(8, 0, 4, None, None, None, None, None) == -1 and ap(1 << 30, 1, 4, None, None, None, None, None) == -1

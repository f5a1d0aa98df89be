"""Writes tests/golden/waymo_select.npz: inputs and expected integers for the selection of moving Waymo samples
(ogc_amd/csrc/moving_stats.hip, ogc_amd/data_prepare/scan_ops.py::moving_stats, ogc_amd/data_prepare/select_mov.py).  CPU only.

    python tests/golden/make_waymo_select_golden.py --reference <root of the reference tree>

The expected integers are what the reference's own functions give — `detect_moving` and `convert_id_to_pair` of
data_prepare/waymo/select_mov.py (it has a main guard) and `WaymoOpenDataset.filter_segm` of datasets/dataset_waymo.py — under
the lines of select_mov.py:74-96 restated in `reference_sample`.  `moving_mirror` is this repository's own statement of the same
three integers in numpy, the fp64 residual in the order include/ogc_ops.h documents; `selected` is the selection rule.  At
generation time the mirror must EQUAL the reference on every case.  The GPU tests apply the mirror to inputs they draw
themselves; they never read the reference.

The drawn cases are decided: a static point carries the fp32-rounded rigid flow (residual below 1e-4), a moving point 0.5 m or
more on top, so no point lies near the threshold and the order of a sum cannot matter.  The `edge` case sits ON the threshold
where every order gives the same bits: R = I, t = 0, one non-zero flow component d and moving_thresh = float(d).
"""
import argparse
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
GROUND_Y = 0.3
# name, N, seed, ignore_class_ids, ignore_npoint_thresh, kind
CASES = (("mixed", 300, 31, (2, 3), 25, "moving"), ("no_filter", 257, 32, (), 0, "moving"), ("static", 300, 33, (2, 3), 20, "static"),
         ("background", 120, 34, (2, 3), 50, "background"), ("class_only", 64, 35, (2, 3), 0, "class_only"),
         ("all_small", 90, 36, (), 50, "moving"), ("empty", 0, 37, (2, 3), 50, "static"), ("edge", 4, 38, (), 0, "edge"))


# ---- the mirror ------------------------------------------------------------------------------------------------------------
def filtered_labels(segm, semantic_segm, ignore_class_ids, ignore_npoint_thresh):
    """The reader's filter: label 0 where the class is ignored or the object has fewer than ignore_npoint_thresh points."""
    ids, sizes = np.unique(segm, return_counts=True)
    ignore = np.isin(semantic_segm, np.asarray(list(ignore_class_ids), dtype=np.int64)) | np.isin(segm, ids[sizes < ignore_npoint_thresh])
    return np.where(ignore, 0, segm)


def residual_norm(pc, flow, motion):
    """‖R p + t − p − flow‖ per point, fp64 from the fp32 inputs: ((r_i0 x + r_i1 y) + r_i2 z) + t_i − p_i − f_i, then
    sqrt((d0² + d1²) + d2²)."""
    assert pc.dtype == np.float32 and flow.dtype == np.float32
    m = np.asarray(motion, dtype=np.float64).reshape(12)
    p, f = pc.astype(np.float64), flow.astype(np.float64)
    d = [((((m[3 * i] * p[:, 0] + m[3 * i + 1] * p[:, 1]) + m[3 * i + 2] * p[:, 2]) + m[9 + i]) - p[:, i]) - f[:, i] for i in range(3)]
    return np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


def moving_mirror(pc, flow, segm, semantic_segm, motion, ignore_class_ids=(), ignore_npoint_thresh=0, ground_y=GROUND_Y, moving_thresh=0.2):
    """-> (n_distinct, n_fg, n_mov) of one sample: pc, flow (N, 3) float32, segm, semantic_segm (N,) ints, motion (12,) float64."""
    n_distinct = int(np.unique(filtered_labels(segm, semantic_segm, ignore_class_ids, ignore_npoint_thresh)).shape[0])
    fg = pc[:, 1] >= np.float32(ground_y)
    n_mov = int((residual_norm(pc[fg], flow[fg], motion) > moving_thresh).sum())
    return n_distinct, int(fg.sum()), n_mov


def selected(n_distinct, n_fg, n_mov, ratio_thresh=0.2):
    """select_mov.py:78, 94-96 from the integers: not pure background, and the ratio of moving points above the threshold."""
    return bool(n_distinct != 1 and n_fg > 0 and np.float32(n_mov) / n_fg > ratio_thresh)


def motion_row(pose1, pose2):
    """select_mov.py:85-88: the relative motion of the sensor from frame 1 to frame 2 as (12,) float64, rotation then translation."""
    rot1, transl1, rot2, transl2 = pose1[0:3, 0:3], pose1[0:3, 3], pose2[0:3, 0:3], pose2[0:3, 3]
    return np.concatenate([(rot2.T @ rot1).reshape(9), rot2.T @ (transl1 - transl2)]).astype(np.float64)


# ---- decided inputs ----------------------------------------------------------------------------------------------------------
def random_motion(rs):
    yaw = (rs.rand() - 0.5) * 0.1
    c, s = np.cos(yaw), np.sin(yaw)
    rot = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
    return np.concatenate([rot.reshape(9), [(rs.rand() - 0.5) * 0.4, 0.0, 0.5 + rs.rand()]])


def draw_sample(n, rs, kind="moving", n_label=6):
    """A decided sample of n points: labels 0 .. n_label - 1 (0 the ground, about half of the points, mostly below y = 0.3),
    classes 0 / 1 / 2 / 3; `moving`: the objects of odd label carry 0.5 to 1 m on top of the rigid flow; `static`: nobody does;
    `background`: one label, 0; `class_only`: one label, 3, a few of its points of class 2.
    -> pc, flow float32, segm, semantic_segm int32, motion (12,) float64."""
    motion = random_motion(rs)
    segm = (rs.randint(n_label, size=n) * (rs.rand(n) < 0.5)).astype(np.int32)
    if kind == "background":
        segm[:] = 0
    semantic = np.where(segm > 0, 1 + segm % 3, 0).astype(np.int32)
    if kind == "class_only":
        segm[:] = 3
        semantic[:] = 1
        semantic[::7] = 2
    pc = ((rs.rand(n, 3) - 0.5) * np.array([60.0, 0.0, 60.0])).astype(np.float32)
    pc[:, 1] = np.where(segm > 0, 0.35 + 2.0 * rs.rand(n), -0.2 + 0.6 * rs.rand(n)).astype(np.float32)
    p = pc.astype(np.float64)
    rigid = p @ motion[:9].reshape(3, 3).T + motion[9:] - p
    extra = np.zeros((n, 3))
    if kind == "moving":
        angle, length = rs.rand(n) * 2 * np.pi, 0.5 + 0.5 * rs.rand(n)
        extra = np.stack([length * np.cos(angle), np.zeros(n), length * np.sin(angle)], 1) * (segm % 2 == 1)[:, None]
    return pc, (rigid + extra).astype(np.float32), segm, semantic, motion


def edge_sample(d=np.float32(0.2), axis=0, sign=1.0):
    """Four foreground points, R = I, t = 0, one flow component each: 0, d / 2, d and the float32 above d, times `sign`, in component
    `axis`; with moving_thresh = float(d) exactly the last one is moving.  -> pc, flow, segm, semantic_segm, motion, moving_thresh."""
    d = np.float32(d)
    pc = np.array([[1.0, 0.5, 2.0], [-3.0, 0.75, 4.0], [5.0, 1.0, -6.0], [7.0, 1.5, 8.0]], dtype=np.float32)
    flow = np.zeros((4, 3), dtype=np.float32)
    flow[:, axis] = np.float32(sign) * np.array([0.0, d / np.float32(2), d, np.nextafter(d, np.float32(np.inf))], dtype=np.float32)
    motion = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])
    return pc, flow, np.array([0, 1, 1, 2], dtype=np.int32), np.array([0, 1, 1, 1], dtype=np.int32), motion, float(d)


def assert_decided(pc, flow, motion, moving_thresh=0.2, margin=1e-6):
    """No point's residual lies within `margin` of the threshold; static ones are below 1e-4 (the callers draw them so)."""
    r = residual_norm(pc, flow, motion)
    assert not np.any(np.abs(r - moving_thresh) <= margin), "a point within %g of the threshold" % margin
    assert np.all((r < 1e-4) | (r > moving_thresh + 0.25))


def case_inputs(name):
    _, n, seed, ignore, thresh, kind = next(c for c in CASES if c[0] == name)
    if kind == "edge":
        pc, flow, segm, semantic, motion, moving_thresh = edge_sample()
    else:
        pc, flow, segm, semantic, motion = draw_sample(n, np.random.RandomState(seed), kind)
        moving_thresh = 0.2
        assert_decided(pc, flow, motion, moving_thresh)
    return pc, flow, segm, semantic, motion, ignore, thresh, moving_thresh


# ---- the reference ---------------------------------------------------------------------------------------------------------
def load_reference(reference_root):
    """(select_mov module, dataset_waymo module) of the reference; the native operators its utils import are stood in for."""
    sys.path.insert(0, HERE)
    sys.path.insert(0, ROOT)
    from make_golden import install_shims
    install_shims()
    try:
        import tqdm  # noqa: F401
    except ImportError:
        sys.modules["tqdm"] = types.ModuleType("tqdm")
    sys.path.insert(0, reference_root)
    sys.path.insert(0, os.path.join(reference_root, "data_prepare", "waymo"))
    import importlib.util

    import select_mov
    spec = importlib.util.spec_from_file_location("ref_dataset_waymo", os.path.join(reference_root, "datasets", "dataset_waymo.py"))
    dataset_waymo = importlib.util.module_from_spec(spec)       # by path: an installed package may be called `datasets` too
    spec.loader.exec_module(dataset_waymo)
    return select_mov, dataset_waymo


def reference_sample(select_mov, dataset_waymo, pc, flow, segm, semantic, motion, ignore, thresh, moving_thresh, ratio_thresh=0.2):
    """select_mov.py:74-96 on arrays in place of files -> (n_distinct, n_fg, n_mov, selected)."""
    reader = object.__new__(dataset_waymo.WaymoOpenDataset)
    reader.ignore_class_ids, reader.ignore_npoint_thresh = list(ignore), thresh
    segms, _ = reader.filter_segm([segm.copy()], [semantic.copy()])
    pc, segm, flow = pc.astype(np.float32), segms[0].astype(np.int32), flow.astype(np.float32)        # dataset_waymo.py:166
    n_distinct = np.unique(segm).shape[0]
    rot, transl = motion[:9].reshape(3, 3), motion[9:]
    not_ground = (pc[:, 1] >= 0.3)
    pc_fg, flow_fg = pc[not_ground], flow[not_ground]
    n_mov_point = select_mov.detect_moving(pc_fg, flow_fg, rot, transl, thresh=moving_thresh)
    with np.errstate(invalid="ignore", divide="ignore"):
        n_mov_point_ratio = n_mov_point / pc_fg.shape[0]
    chosen = (n_distinct != 1) and bool(n_mov_point_ratio > ratio_thresh)
    return int(n_distinct), int(pc_fg.shape[0]), int(n_mov_point), chosen


def build(reference_root):
    select_mov, dataset_waymo = load_reference(reference_root)
    out, meta = {}, {"ground_y": GROUND_Y, "ratio_thresh": 0.2, "numpy": np.__version__, "cases": {}}
    for name, n, _, ignore, thresh, kind in CASES:
        pc, flow, segm, semantic, motion, ignore, thresh, moving_thresh = case_inputs(name)
        assert pc.shape == (n, 3) and n <= 300
        want = reference_sample(select_mov, dataset_waymo, pc, flow, segm, semantic, motion, ignore, thresh, moving_thresh)
        got = moving_mirror(pc, flow, segm, semantic, motion, ignore, thresh, GROUND_Y, moving_thresh)
        assert got == want[:3], "the mirror and the reference differ on %s: %s, %s" % (name, got, want)
        assert selected(*got) == want[3], "the selection rules differ on %s" % name
        for key, value in (("pc", pc), ("flow", flow), ("segm", segm), ("semantic_segm", semantic), ("motion", motion),
                           ("stats", np.array(got, dtype=np.int32))):
            out["%s_%s" % (name, key)] = value
        meta["cases"][name] = {"n": n, "ignore_class_ids": list(ignore), "ignore_npoint_thresh": thresh, "moving_thresh": moving_thresh,
                               "selected": want[3], "kind": kind}
        print("case %-10s N = %3d: n_distinct %d, n_fg %3d, n_mov %3d, selected %s: mirror == reference" % ((name, n) + want))
    stats = {name: out[name + "_stats"].tolist() for name in meta["cases"]}
    assert stats["edge"][1:] == [4, 1] and stats["background"][0] == 1 and stats["class_only"][0] == 2 and stats["all_small"][0] == 1
    assert stats["static"][2] == 0 and stats["empty"] == [0, 0, 0] and meta["cases"]["mixed"]["selected"]
    ids = [["a", 0], ["a", 3], ["b", 1], ["b", 0], ["c", 7]]
    pairs = select_mov.convert_id_to_pair([tuple(i) for i in ids])
    meta["frame_ids"], meta["pairs"] = ids, [list(p) for p in pairs]
    return out, meta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference tree (its data_prepare/waymo/select_mov.py is imported)")
    args = ap.parse_args()
    out, meta = build(args.reference)
    path = os.path.join(HERE, "waymo_select.npz")
    np.savez_compressed(path, meta=json.dumps(meta), **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()

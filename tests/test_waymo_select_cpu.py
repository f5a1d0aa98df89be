"""The device-free side of the Waymo sample selection: the numpy mirror of tests/golden/make_waymo_select_golden.py
against the fixture its generator pinned to the reference's own functions, convert_id_to_pair, filter_empty on a written root, the
refusals of scan_ops.moving_stats that need no device, and the two new entries of the C ABI."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def mirror():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_waymo_select_golden
    return make_waymo_select_golden


@pytest.fixture(scope="module")
def golden():
    data = np.load(os.path.join(HERE, "golden", "waymo_select.npz"))
    return data, json.loads(str(data["meta"]))


def test_mirror_equals_the_fixture(mirror, golden):
    data, meta = golden
    assert set(meta["cases"]) == {c[0] for c in mirror.CASES}
    for name, case in meta["cases"].items():
        arrays = [data["%s_%s" % (name, key)] for key in ("pc", "flow", "segm", "semantic_segm", "motion")]
        assert arrays[0].dtype == arrays[1].dtype == np.float32 and arrays[2].dtype == arrays[3].dtype == np.int32
        assert arrays[4].dtype == np.float64 and arrays[0].shape == (case["n"], 3)
        got = mirror.moving_mirror(*arrays, case["ignore_class_ids"], case["ignore_npoint_thresh"], meta["ground_y"], case["moving_thresh"])
        assert list(got) == data[name + "_stats"].tolist(), name
        assert mirror.selected(*got, meta["ratio_thresh"]) == case["selected"], name
        # the generator's inputs are drawn again here: the fixture holds what the script says it holds
        for a, b in zip(arrays, mirror.case_inputs(name)[:5]):
            assert a.dtype == b.dtype and np.array_equal(a, b), name
    stats = {name: data[name + "_stats"].tolist() for name in meta["cases"]}
    assert stats["edge"] == [3, 4, 1] and stats["empty"] == [0, 0, 0] and stats["background"][0] == 1 and stats["class_only"][0] == 2
    assert [meta["cases"][n]["selected"] for n in ("mixed", "static", "background", "edge")] == [True, False, False, True]


def test_selection_rule_is_the_float32_ratio(mirror):
    from ogc_amd.data_prepare.select_mov import is_selected
    for row in ((2, 5, 1), (2, 5, 2), (1, 5, 5), (0, 0, 0), (3, 10, 2), (3, 10, 3), (2, 1000003, 200001)):
        assert is_selected(*row, 0.2) == mirror.selected(*row, 0.2)
    assert is_selected(2, 5, 1, 0.2) == bool(np.float32(1) / 5 > 0.2)       # the reference's expression at a ratio ON the threshold
    assert is_selected(2, 5, 2, 0.2) and not is_selected(1, 5, 5, 0.2) and not is_selected(0, 0, 0, 0.2)


def test_convert_id_to_pair(golden):
    from ogc_amd.data_prepare.select_mov import convert_id_to_pair
    _, meta = golden
    pairs = convert_id_to_pair([tuple(i) for i in meta["frame_ids"]])
    assert [list(p) for p in pairs] == meta["pairs"] == [["a", 3, 2], ["b", 1, 0], ["c", 7, 6]]
    assert convert_id_to_pair([]) == [] and convert_id_to_pair([("s", 0)]) == []


def test_relative_motion_is_the_mirrors(mirror):
    from ogc_amd.data_prepare.select_mov import relative_motion
    rs = np.random.RandomState(3)
    poses = []
    for _ in range(2):
        q, _ = np.linalg.qr(rs.randn(3, 3))
        pose = np.eye(4)
        pose[:3, :3], pose[:3, 3] = q, rs.randn(3) * 10
        poses.append(pose)
    got = relative_motion(*poses)
    assert got.dtype == np.float64 and got.shape == (12,) and np.array_equal(got, mirror.motion_row(*poses))


def test_filter_empty(tmp_path, capsys):
    from ogc_amd.data_prepare import filter_empty
    from ogc_amd.datasets import WaymoSingleFrameDataset
    from ogc_amd.utils.synthetic import write_waymo_moving_root
    root = str(tmp_path / "full")
    made = write_waymo_moving_root(root, 3, 4, 160, 128, seed=9400)
    assert made["short_frame"] == ("seq_0000", 2) and made["moving"] == ["seq_0000", "seq_0002"]
    everything = [(name, t) for name in made["names"] for t in range(4)]
    for interval in (1, 5):
        out = str(tmp_path / ("train_sup_%d.json" % interval))
        res = filter_empty.main(["--data_root", root, "--split_file", made["mapping"], "--out", out, "--n_sample_point", "128",
                                 "--sampled_interval", str(interval)])
        printed = capsys.readouterr().out
        want = [i for i in everything[::interval] if i != ("seq_0000", 2)]
        assert res["kept"] == want and json.load(open(out)) == [list(i) for i in want]
        if interval == 1:
            assert res["ignored"] == [("seq_0000", 2)] and "seq_0000 2 112\n" in printed       # 128 - 128 // 8 points
        else:
            assert res["ignored"] == [] and want == [("seq_0000", 0), ("seq_0001", 1), ("seq_0002", 2)]
        reader = WaymoSingleFrameDataset(root, made["mapping"], downsampled=False, select_frame=out)
        assert reader.data_ids == want
    # with a higher count every frame is short: the list is empty, and every frame is printed
    res = filter_empty.main(["--data_root", root, "--split_file", made["mapping"], "--out", str(tmp_path / "none.json"),
                             "--n_sample_point", "100000", "--sampled_interval", "1"])
    assert res["kept"] == [] and len(res["ignored"]) == 12 and len(capsys.readouterr().out.strip().split("\n")) == 13


def test_moving_root_has_what_the_chain_needs(tmp_path):
    """write_waymo_moving_root: boxes that translate by at least 0.5 m with the motion in the stored flow, static sequences, a frame
    under the sample count and an object below ignore_npoint_thresh."""
    from ogc_amd.data_prepare.select_mov import relative_motion
    from ogc_amd.utils.synthetic import write_waymo_moving_root
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_waymo_select_golden as mirror
    root = str(tmp_path / "full")
    made = write_waymo_moving_root(root, 2, 3, 400, 256, seed=9410)
    for name in made["names"]:
        d = os.path.join(root, "data", name)
        speed = np.linalg.norm(made["velocity"][name], axis=1)
        assert (np.all(speed[1:4] >= 0.5) and np.all(speed[4:] == 0)) if name in made["moving"] else np.all(speed == 0)
        for t in (1, 2):
            pc, flow, segm = (np.load(os.path.join(d, "%s.npy" % f)) for f in ("pc_%04d" % t, "flow_%04d_%04d" % (t, t - 1), "segm_%04d" % t))
            assert pc.dtype == np.float32 and flow.dtype == np.float64 and segm.dtype == np.int32
            assert (pc.shape[0] == 224) if (name, t) == made["short_frame"] else (pc.shape[0] >= 256)
            sizes = dict(zip(*np.unique(segm, return_counts=True)))
            assert sizes.get(5, 0) == 12 or (name, t) == made["short_frame"]
            motion = relative_motion(np.load(os.path.join(d, "pose_%04d.npy" % t)), np.load(os.path.join(d, "pose_%04d.npy" % (t - 1))))
            r = mirror.residual_norm(pc, flow.astype(np.float32), motion)
            moves = speed[segm] > 0
            assert np.all(r[~moves] < 1e-4) and np.all(r[moves] >= 0.5 - 1e-4) and (moves.any() == (name in made["moving"]))


def test_moving_stats_refusals_without_a_device():
    from ogc_amd.data_prepare.scan_ops import MOVING_STATS_LABEL_CAP, moving_counts, moving_stats
    assert MOVING_STATS_LABEL_CAP >= 4096
    pc, flow = torch.zeros(4, 3), torch.zeros(4, 3)
    segm, semantic = torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    offsets, motion = torch.tensor([0, 4], dtype=torch.int32), torch.zeros(1, 12, dtype=torch.float64)
    with pytest.raises(TypeError):
        moving_stats(pc.numpy(), flow, segm, semantic, offsets, motion)
    with pytest.raises(TypeError):
        moving_stats(pc.double(), flow, segm, semantic, offsets, motion)
    with pytest.raises(TypeError):
        moving_stats(pc, flow, segm.long(), semantic, offsets, motion)
    with pytest.raises(TypeError):
        moving_stats(pc, flow, segm, semantic, offsets.long(), motion)
    with pytest.raises(TypeError):
        moving_stats(pc, flow, segm, semantic, offsets, motion.float())
    for fn in (moving_stats, moving_counts):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(pc, flow, segm, semantic, offsets, motion)


def test_abi_entries():
    from ogc_amd import _lib
    from ogc_amd.csrc import build as b
    text = open(os.path.join(ROOT, "include", "ogc_ops.h")).read()
    text = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    protos = dict(re.findall(r"\b(ogc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text))
    for name in ("ogc_moving_stats", "ogc_moving_stats_label_cap"):
        params = [p.strip() for p in protos[name].split(",") if p.strip() not in ("", "void")]
        assert len(_lib.SIGNATURES[name]) == len(params)
    assert len(_lib.SIGNATURES["ogc_moving_stats"]) == 15 and _lib.SIGNATURES["ogc_moving_stats_label_cap"] == []
    lib = ctypes.CDLL(b.build())
    assert hasattr(lib, "ogc_moving_stats")
    lib.ogc_moving_stats_label_cap.restype = ctypes.c_int
    cap = lib.ogc_moving_stats_label_cap()
    assert cap >= 4096 and cap == int(re.search(r"#define OGC_MOVING_STATS_LABEL_CAP (\d+)", text).group(1))
    from ogc_amd.pointnet2_cuda import MOVING_STATS_LABEL_CAP
    assert cap == MOVING_STATS_LABEL_CAP

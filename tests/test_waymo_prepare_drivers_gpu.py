"""The end of the Waymo preparation chain — filter_empty -> downsample_waymo -> select_mov (ogc_amd/data_prepare) — each driver in
a fresh child process on a synthetic full-resolution root of 3 sequences x 4 frames x ~600 points
(ogc_amd/utils/synthetic.py::write_waymo_moving_root), sampled to 256 points: the downsampled files against the gather by
furthest_point_sample's indices done here, the frame lists against the mirror of tests/golden/make_waymo_select_golden.py applied to
the written files, and the package's reader on the result."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
N_SAMPLE, N_POINTS, N_FRAMES = 256, 600, 4
IGNORE, THRESH = (2, 3), 8           # at 256 points per frame an object holds some tens of points: 8 drops the small object only
SHORT = ("seq_0000", 2)


def run_driver(name, *args):
    res = subprocess.run([sys.executable, "-m", "ogc_amd.data_prepare." + name] + [str(a) for a in args], cwd=ROOT,
                         env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-3000:]
    return res


@pytest.fixture(scope="module")
def mirror():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_waymo_select_golden
    return make_waymo_select_golden


@pytest.fixture(scope="module")
def chain(tmp_path_factory):
    """The three drivers run once: downsample_waymo --synthetic 3 writes the full root first; a second downsample_waymo run takes
    stored `predicted` flows to their own tree."""
    base = tmp_path_factory.mktemp("waymo_chain")
    full, down, lists = str(base / "full"), str(base / "down"), str(base / "lists")
    split_file = os.path.join(full, "train.txt")
    os.makedirs(full)
    res_down = run_driver("downsample_waymo", "--data_root", full, "--save_root", down, "--split_file", split_file,
                          "--n_sample_point", N_SAMPLE, "--synthetic", 3, "--synthetic_points", N_POINTS)
    names = open(split_file).read().split()
    stored = {}
    for name in names:
        d = os.path.join(full, "flow_preds", "pred", name)
        os.makedirs(d)
        for t in range(1, N_FRAMES):
            n = np.load(os.path.join(full, "data", name, "pc_%04d.npy" % t)).shape[0]
            stored[name, t] = np.random.RandomState(90 + t + 10 * len(stored)).randn(n, 3).astype(np.float32)
            np.save(os.path.join(d, "flow_%04d_%04d.npy" % (t, t - 1)), stored[name, t])
    res_pred = run_driver("downsample_waymo", "--data_root", full, "--save_root", down, "--split_file", split_file,
                          "--n_sample_point", N_SAMPLE, "--predflow_path", "pred")
    sup = os.path.join(lists, "train_sup.json")
    res_filter = run_driver("filter_empty", "--data_root", full, "--split_file", split_file, "--out", sup, "--n_sample_point", N_SAMPLE,
                            "--sampled_interval", 1)
    res_select = run_driver("select_mov", "--data_root", down, "--pose_root", full, "--split_file", os.path.join(down, "train.txt"),
                            "--sup_frames", sup, "--out_dir", lists, "--ignore_class_ids", *IGNORE, "--ignore_npoint_thresh", THRESH,
                            "--batch", 4)
    return {"full": full, "down": down, "lists": lists, "names": names, "stored": stored, "sup": sup,
            "res": {"down": res_down, "pred": res_pred, "filter": res_filter, "select": res_select}}


def fps_indices(pc):
    from ogc_amd.pointnet2.pointnet2 import furthest_point_sample
    idx = furthest_point_sample(torch.from_numpy(pc)[None].cuda().contiguous(), N_SAMPLE)[0].long().cpu().numpy()
    assert len(set(idx.tolist())) == N_SAMPLE
    return idx


def test_downsampled_files_are_the_gather_by_the_fps_indices(chain):
    full, down, names = chain["full"], chain["down"], chain["names"]
    assert names == ["seq_0000", "seq_0001", "seq_0002"]
    assert open(os.path.join(down, "train.txt")).read() == open(os.path.join(full, "train.txt")).read()
    assert sorted(os.listdir(os.path.join(down, "data"))) == names
    for name in names:
        src, dst = os.path.join(full, "data", name), os.path.join(down, "data", name)
        files = ["%s_%04d.npy" % (w, t) for w in ("pc", "segm", "semantic_segm") for t in range(N_FRAMES)]
        files += ["flow_%04d_%04d.npy" % (t, t - 1) for t in range(1, N_FRAMES)]
        assert sorted(os.listdir(dst)) == sorted(files)                                # every frame once, no pose, no ground mask
        for t in range(N_FRAMES):
            pc = np.load(os.path.join(src, "pc_%04d.npy" % t))
            short = (name, t) == SHORT
            assert (pc.shape[0] == N_SAMPLE - N_SAMPLE // 8) if short else (pc.shape[0] > 2 * N_SAMPLE)
            idx = np.arange(pc.shape[0]) if short else fps_indices(pc)
            what = ["pc_%04d" % t, "segm_%04d" % t, "semantic_segm_%04d" % t] + (["flow_%04d_%04d" % (t, t - 1)] if t else [])
            for w in what:
                a, b = np.load(os.path.join(src, w + ".npy")), np.load(os.path.join(dst, w + ".npy"))
                assert a.dtype == b.dtype and b.shape[0] == idx.shape[0] and np.array_equal(a[idx], b), (name, w)
            if t:
                a = chain["stored"][name, t]
                b = np.load(os.path.join(down, "flow_preds", "pred", name, "flow_%04d_%04d.npy" % (t, t - 1)))
                assert b.dtype == np.float32 and np.array_equal(a[idx], b)
        assert sorted(os.listdir(os.path.join(down, "flow_preds", "pred", name))) == ["flow_%04d_%04d.npy" % (t, t - 1) for t in range(1, N_FRAMES)]
    for key in ("down", "pred"):
        res = chain["res"][key]
        assert "12 frames of 9 pairs written" in res.stdout and "1 short" in res.stdout
        assert "frame seq_0000 2 written whole, it has %d points, fewer than %d" % (N_SAMPLE - N_SAMPLE // 8, N_SAMPLE) in res.stderr
    assert json.load(open(os.path.join(down, "short_frames.json"))) == [[SHORT[0], SHORT[1], N_SAMPLE - N_SAMPLE // 8]]


def test_frame_lists(chain, mirror):
    from ogc_amd.datasets import WaymoOpenDataset, WaymoSingleFrameDataset
    full, down, lists, names = chain["full"], chain["down"], chain["lists"], chain["names"]
    frames = [[n, t] for n in names for t in range(N_FRAMES) if (n, t) != SHORT]
    assert json.load(open(chain["sup"])) == frames and "seq_0000 2 %d\n" % (N_SAMPLE - N_SAMPLE // 8) in chain["res"]["filter"].stdout
    pairs = [[n, t, t - 1] for n, t in frames if t > 0]
    assert json.load(open(os.path.join(lists, "train_sup_paired.json"))) == pairs and len(pairs) == 8
    # the pair (3, 2) of seq_0000 has the short frame as its second frame: the reader could not stack it
    dropped = ["seq_0000", 3, 2]
    res = chain["res"]["select"]
    assert "pair seq_0000 3 2 dropped, its frames have %d and %d points" % (N_SAMPLE, N_SAMPLE - N_SAMPLE // 8) in res.stderr
    assert "1 pairs dropped" in res.stderr
    want, small_seen = [], False
    for name, t, u in pairs:
        if [name, t, u] == dropped:
            continue
        d = os.path.join(down, "data", name)
        pc, segm, semantic = (np.load(os.path.join(d, "%s_%04d.npy" % (w, t))) for w in ("pc", "segm", "semantic_segm"))
        flow = np.load(os.path.join(d, "flow_%04d_%04d.npy" % (t, u))).astype(np.float32)
        poses = [np.load(os.path.join(full, "data", name, "pose_%04d.npy" % v)) for v in (t, u)]
        motion = mirror.motion_row(*poses)
        mirror.assert_decided(pc, flow, motion, 0.2, margin=1e-6)
        sizes = np.unique(segm, return_counts=True)[1]
        small_seen |= bool((sizes < THRESH).any()) and bool((sizes >= THRESH).sum() >= 2)
        if mirror.selected(*mirror.moving_mirror(pc, flow, segm, semantic, motion, IGNORE, THRESH, 0.3, 0.2), 0.2):
            want.append([name, t, u])
    assert small_seen                                          # the size rule had something to drop and something to keep
    got = json.load(open(os.path.join(lists, "train_unsup.json")))
    assert got == want
    assert 0 < len(got) < len(pairs) - 1 and {p[0] for p in got} == {"seq_0000", "seq_0002"}       # seq_0001 is static
    assert res.stdout.strip().split("\n")[-1] == "%d %d" % (len(pairs), len(got))
    reader = WaymoOpenDataset(down, os.path.join(down, "train.txt"), downsampled=True, select_frame=os.path.join(lists, "train_unsup.json"),
                              ignore_class_ids=IGNORE, ignore_npoint_thresh=THRESH)
    assert len(reader) == len(got)
    for sid in range(len(reader)):
        pcs, segms, flows, valids = reader[sid]
        assert pcs.shape == flows.shape == (2, N_SAMPLE, 3) and segms.shape == valids.shape == (2, N_SAMPLE)
        assert len(set(segms[0].tolist())) > 1
    single = WaymoSingleFrameDataset(down, os.path.join(down, "train.txt"), downsampled=True, select_frame=chain["sup"])
    assert len(single) == len(frames) and single[0][0].shape == (1, N_SAMPLE, 3)

"""WaymoOpenDataset (ogc_amd/datasets.py) on the synthetic root of ogc_amd/utils/synthetic.py::write_waymo_root, and the host-side
pieces of the Waymo flow-prediction driver (ogc_amd/test_flow_waymo.py) against their numpy formulas.  CPU only."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

N_SEQ, N_FRAMES, N_POINTS = 2, 4, 1500


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    from ogc_amd.utils.synthetic import write_waymo_root
    root = str(tmp_path_factory.mktemp("waymo"))
    mapping, poses = write_waymo_root(root, N_SEQ, N_FRAMES, N_POINTS, seed=2000, split="val")
    return root, mapping, poses


def _frame(root, seq, t, what="pc"):
    return np.load(os.path.join(root, "data", "seq_%04d" % seq, "%s_%04d.npy" % (what, t)))


def test_round_trip_of_the_synthetic_root(root, capsys):
    from ogc_amd.datasets import WaymoOpenDataset
    path, mapping, poses = root
    assert mapping == os.path.join(path, "val.txt") and sorted(poses) == ["seq_0000", "seq_0001"]
    ds = WaymoOpenDataset(path, mapping)
    assert capsys.readouterr().out == ""                        # no printing on load
    assert ds.data_ids == [("seq_%04d" % s, t, t - 1) for s in range(N_SEQ) for t in range(1, N_FRAMES)]
    assert len(ds) == N_SEQ * (N_FRAMES - 1)
    sizes = set()
    for sid, (name, t, u) in enumerate(ds.data_ids):
        pcs, segms, flows, valids = ds[sid]
        s = int(name[-4:])
        assert np.array_equal(pcs[0], _frame(path, s, t)) and np.array_equal(pcs[1], _frame(path, s, u))
        assert np.array_equal(segms[0], _frame(path, s, t, "segm")) and np.array_equal(segms[1], _frame(path, s, u, "segm"))
        stored = np.load(os.path.join(path, "data", name, "flow_%04d_%04d.npy" % (t, u)))
        assert np.array_equal(flows[0], stored) and np.array_equal(flows[1], stored)    # backward flow only
        assert pcs[0].dtype == np.float32 and flows[0].dtype == np.float32 and flows[0].shape == pcs[0].shape
        assert all(v.all() and v.dtype == np.int32 for v in valids)
        sizes.update(p.shape[0] for p in pcs)
    assert len(sizes) > 1, "the frames must differ in their numbers of points"


def test_listed_sequences_that_are_absent_are_passed_over(root, tmp_path):
    from ogc_amd.datasets import WaymoOpenDataset
    mapping = str(tmp_path / "split.txt")
    with open(mapping, "w") as f:
        f.write("seq_0001.tfrecord\nnot_there.tfrecord\n")
    ds = WaymoOpenDataset(root[0], mapping)
    assert ds.n_skipped == 1 and ds.data_ids == [("seq_0001", t, t - 1) for t in range(1, N_FRAMES)]


def test_sampled_interval_and_select_frame(root, tmp_path):
    from ogc_amd.datasets import WaymoOpenDataset
    path, mapping, _ = root
    every = WaymoOpenDataset(path, mapping).data_ids
    assert WaymoOpenDataset(path, mapping, sampled_interval=2).data_ids == every[::2]
    chosen = [["seq_0001", 3, 2], ["seq_0000", 1, 0]]
    select = str(tmp_path / "select.json")
    with open(select, "w") as f:
        json.dump(chosen, f)
    ds = WaymoOpenDataset(path, mapping, select_frame=select)
    assert ds.data_ids == [("seq_0001", 3, 2), ("seq_0000", 1, 0)]
    assert np.array_equal(ds[0][0][0], _frame(path, 1, 3)) and np.array_equal(ds[1][0][1], _frame(path, 0, 0))


def test_filter_segm_by_class_and_by_size(root):
    from ogc_amd.datasets import WaymoOpenDataset
    path, mapping, _ = root
    segm, semantic = _frame(path, 0, 1, "segm"), _frame(path, 0, 1, "semantic_segm")
    assert set(np.unique(semantic)) == {0, 1, 2}
    _, segms, _, valids = WaymoOpenDataset(path, mapping, ignore_class_ids=[2])[0]
    assert np.array_equal(valids[0], (semantic != 2).astype(np.int32))
    assert np.array_equal(segms[0], np.where(semantic == 2, 0, segm))
    ids, sizes = np.unique(segm, return_counts=True)
    thresh = int(np.sort(sizes)[2]) + 1                                     # three objects are smaller than this
    small = np.isin(segm, ids[sizes < thresh])
    assert 0 < small.sum() < segm.size
    _, segms, _, valids = WaymoOpenDataset(path, mapping, ignore_npoint_thresh=thresh)[0]
    assert np.array_equal(valids[0], 1 - small.astype(np.int32)) and np.array_equal(segms[0], np.where(small, 0, segm))
    _, segms, _, valids = WaymoOpenDataset(path, mapping, ignore_class_ids=[2], ignore_npoint_thresh=thresh)[0]
    assert np.array_equal(valids[0], 1 - np.logical_or(small, semantic == 2).astype(np.int32))
    assert np.array_equal(_frame(path, 0, 1, "segm"), segm)                 # the files are not touched


@pytest.fixture(scope="module")
def equal_root(root, tmp_path_factory):
    """The same sequences cut to 1000 points per frame: what the down-sampled data set looks like."""
    path, _, _ = root
    out = str(tmp_path_factory.mktemp("waymo_equal"))
    for s in range(N_SEQ):
        d = os.path.join(out, "data", "seq_%04d" % s)
        os.makedirs(d)
        for t in range(N_FRAMES):
            for what in ("pc", "segm", "semantic_segm"):
                np.save(os.path.join(d, "%s_%04d.npy" % (what, t)), _frame(path, s, t, what)[:1000])
            if t >= 1:
                name = "flow_%04d_%04d.npy" % (t, t - 1)
                np.save(os.path.join(d, name), np.load(os.path.join(path, "data", "seq_%04d" % s, name))[:1000])
    shutil.copy(os.path.join(path, "val.txt"), os.path.join(out, "val.txt"))
    return out


def test_downsampled_path_stacks_and_compresses(equal_root):
    from ogc_amd.datasets import WaymoOpenDataset
    mapping = os.path.join(equal_root, "val.txt")
    pcs, segms, flows, valids = WaymoOpenDataset(equal_root, mapping, downsampled=True, ignore_class_ids=[2])[1]
    assert pcs.shape == (2, 1000, 3) and pcs.dtype == np.float32
    assert segms.shape == (2, 1000) and segms.dtype == np.int32
    assert flows.shape == (2, 1000, 3) and flows.dtype == np.float32
    assert valids.shape == (2, 1000) and valids.dtype == np.float32
    raw = np.stack([_frame(equal_root, 0, 2, "segm"), _frame(equal_root, 0, 1, "segm")])
    semantic = np.stack([_frame(equal_root, 0, 2, "semantic_segm"), _frame(equal_root, 0, 1, "semantic_segm")])
    kept = np.where(semantic == 2, 0, raw)
    assert np.array_equal(valids, (semantic != 2).astype(np.float32))
    assert np.array_equal(segms, np.unique(kept, return_inverse=True)[1].reshape(2, -1))     # consecutive ids from 0
    assert segms.max() == len(np.unique(kept)) - 1 < raw.max()
    assert np.array_equal(pcs[0], _frame(equal_root, 0, 2))
    centred = WaymoOpenDataset(equal_root, mapping, downsampled=True, decentralize=True)[1][0]
    np.testing.assert_allclose(centred, pcs - pcs.mean(1).mean(0), atol=1e-5)
    args = {"scale_low": 0.95, "scale_high": 1.05, "degree_range": [0, 180, 0], "shift_range": [1, 0.1, 1]}
    aug = WaymoOpenDataset(equal_root, mapping, downsampled=True, aug_transform=True, aug_transform_args=args)[1]
    assert aug[0].shape == (4, 1000, 3) and aug[1].shape == (4, 1000) and aug[2].shape == (4, 1000, 3) and aug[3].shape == (4, 1000)


def test_saved_predictions_come_back_through_predflow_path(equal_root):
    from ogc_amd.datasets import WaymoOpenDataset
    mapping = os.path.join(equal_root, "val.txt")
    ds = WaymoOpenDataset(equal_root, mapping)
    save_root = os.path.join(equal_root, "flow_preds", "some_model")
    rs = np.random.RandomState(3)
    preds = [rs.randn(1, 1000, 3).astype(np.float32) for _ in range(len(ds))]
    for sid, pred in enumerate(preds):
        ds._save_predflow(torch.from_numpy(pred), save_root=save_root, batch_size=1, n_frame=1, offset=sid)
    name, t, u = ds.data_ids[4]
    assert os.path.isfile(os.path.join(save_root, name, "flow_%04d_%04d.npy" % (t, u)))
    back = WaymoOpenDataset(equal_root, mapping, predflow_path="some_model")
    for sid, pred in enumerate(preds):
        _, _, flows, _ = back[sid]
        assert np.array_equal(flows[0], pred[0]) and np.array_equal(flows[1], pred[0])
    with pytest.raises(FileNotFoundError):
        WaymoOpenDataset(equal_root, mapping, predflow_path="nobody")[0]


def test_guaranteed_gaps_of_the_synthetic_ground(root):
    from ogc_amd.utils.synthetic import WAYMO_SHEET
    path, _, poses = root
    a, b, c = WAYMO_SHEET
    by_height_differs = 0
    for s in range(N_SEQ):
        for t in range(N_FRAMES):
            pc, ground = _frame(path, s, t).astype(np.float64), _frame(path, s, t, "ground").astype(bool)
            pose = _frame(path, s, t, "pose")
            assert pose.shape == (4, 4) and np.array_equal(pose, poses["seq_%04d" % s][t])
            world = pc @ pose[:3, :3].T + pose[:3, 3]
            above = world[:, 1] - (a * world[:, 0] + b * world[:, 2] + c)
            assert np.abs(above[ground]).max() <= 0.1 and above[~ground].min() >= 0.6 - 1e-5
            assert 0.3 < ground.mean() < 0.8
            assert np.array_equal(ground, _frame(path, s, t, "segm") == 0)
            by_height_differs += int(((pc[:, 1] < 0.3) != ground).sum())
            assert pc[~ground, 1].min() > 0.3               # ... but only by missing ground, never by taking an object
    assert by_height_differs > 100, "a height threshold alone must mislabel part of the tilted ground"


def test_stored_flow_is_the_rigid_flow_of_the_poses(root):
    from ogc_amd.test_flow_waymo import ego_motion_from_poses
    path, _, poses = root
    pc = _frame(path, 1, 2).astype(np.float64)
    p1, p2 = poses["seq_0001"][2], poses["seq_0001"][1]
    rot, transl = p2[:3, :3].T @ p1[:3, :3], p2[:3, :3].T @ (p1[:3, 3] - p2[:3, 3])
    T = ego_motion_from_poses(p1, p2)
    assert T.dtype == torch.float64 and T.shape == (4, 4)
    assert np.array_equal(T[:3, :3].numpy(), rot) and np.array_equal(T[:3, 3].numpy(), transl)
    assert np.array_equal(T[3].numpy(), [0.0, 0.0, 0.0, 1.0])
    flow = np.load(os.path.join(path, "data", "seq_0001", "flow_0002_0001.npy"))
    np.testing.assert_allclose(flow, pc @ rot.T + transl - pc, atol=1e-5)
    assert np.linalg.norm(flow, axis=1).mean() > 0.3        # the sensor moves


def test_register_bound_is_the_numpy_formula():
    from ogc_amd.test_flow_waymo import register_bound
    rs = np.random.RandomState(5)
    pc = ((rs.rand(4000, 3) - 0.5) * np.array([140.0, 6.0, 140.0])).astype(np.float32)
    angle = 0.3
    rot = np.array([[np.cos(angle), 0, np.sin(angle)], [0, 1, 0], [-np.sin(angle), 0, np.cos(angle)]])
    transl = np.array([0.5, 0.1, -2.0])
    moved = np.einsum("ij,nj->ni", rot, pc) + transl
    want = ((moved[:, 2] > np.abs(moved[:, 0])) & (np.square(moved).sum(1) < 60 * 60) & (np.abs(moved[:, 0]) < 50)
            & (moved[:, 2] < 35))
    got = register_bound(torch.from_numpy(pc), None, torch.from_numpy(rot), torch.from_numpy(transl), True)
    assert got.dtype == torch.bool and np.array_equal(got.numpy(), want) and 0 < want.sum() < want.size
    # each of the four conditions removes points of its own
    assert ((moved[:, 2] > np.abs(moved[:, 0])) & ~want).any() and (np.square(moved).sum(1) >= 3600).any()
    assert register_bound(torch.from_numpy(pc), None, rot, transl, False).all()

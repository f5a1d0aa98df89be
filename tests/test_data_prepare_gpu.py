"""The three preparation drivers (ogc_amd/data_prepare/process_*.py), each run once in a fresh child process on a synthetic raw
root of 2-3 frames of about 3000 points (ogc_amd/utils/synthetic.py::write_*_raw_root), n_sample_point = 512 for the camera sets:
names, shapes and dtypes of the output, labels against the truth the roots were constructed with, the saved points against
crop -> FPS done step by step here, Waymo's flows against the rigid flow of the poses, and the package's own readers on the
output."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_POINTS, N_SAMPLE = 3000, 512


def run_driver(name, *args):
    res = subprocess.run([sys.executable, "-m", "ogc_amd.data_prepare." + name] + [str(a) for a in args], cwd=ROOT,
                         env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-3000:]
    return res


def crop_and_sample(scan, calib, width=1242, height=375):
    """crop -> FPS with the public operators: (pc (N_SAMPLE, 3) numpy, the rows of the scan they come from)."""
    from ogc_amd.data_prepare.scan_ops import crop_camera
    from ogc_amd.pointnet2.pointnet2 import furthest_point_sample
    pc, keep_idx = crop_camera(torch.from_numpy(scan).cuda(), calib, width, height)
    fps_idx = furthest_point_sample(pc[None].contiguous(), N_SAMPLE)[0].long()
    return pc[fps_idx].cpu().numpy(), keep_idx.long()[fps_idx].cpu().numpy()


@pytest.fixture(scope="module")
def kittidet(tmp_path_factory):
    from ogc_amd.utils.synthetic import write_kittidet_raw_root
    root = str(tmp_path_factory.mktemp("kittidet"))
    frames = write_kittidet_raw_root(root, 3, N_POINTS)
    # a fourth frame whose crop leaves too few points: the first 600 rows of frame 0
    base = os.path.join(root, "training")
    np.fromfile(os.path.join(base, "velodyne", "000000.bin"), dtype=np.float32)[:600 * 4].tofile(os.path.join(base, "velodyne", "000003.bin"))
    for sub, ext in (("calib", "txt"), ("label_2", "txt"), ("image_2", "png")):
        with open(os.path.join(base, sub, "000000." + ext), "rb") as src, open(os.path.join(base, sub, "000003." + ext), "wb") as dst:
            dst.write(src.read())
    return root, frames, run_driver("process_kittidet", root, "--n_sample_point", N_SAMPLE)


def test_kittidet_driver(kittidet):
    from ogc_amd.datasets import KITTIDetectionDataset
    root, frames, res = kittidet
    assert sorted(os.listdir(os.path.join(root, "downsampled"))) == ["000000", "000001", "000002"]
    assert "3 frames written" in res.stdout and "1 skipped" in res.stdout and "frame 000003 skipped" in res.stderr
    for i, frame in enumerate(frames):
        d = os.path.join(root, "downsampled", "%06d" % i)
        assert sorted(os.listdir(d)) == ["pc.npy", "segm.npy"]
        pc, segm = np.load(os.path.join(d, "pc.npy")), np.load(os.path.join(d, "segm.npy"))
        assert pc.shape == (N_SAMPLE, 3) and pc.dtype == np.float32 and segm.shape == (N_SAMPLE,) and segm.dtype == np.int32
        scan = np.fromfile(os.path.join(root, "training", "velodyne", "%06d.bin" % i), dtype=np.float32).reshape(-1, 4)
        want_pc, rows = crop_and_sample(scan, frame["calib"])
        assert np.array_equal(pc.view(np.int32), want_pc.view(np.int32))
        assert np.array_equal(segm, frame["labels"][rows])               # the id is the label line + 1: no map needed
        assert set(segm.tolist()) <= {0, 2, 4, 5} and len(set(segm.tolist())) >= 3
    mapping = os.path.join(root, "val.txt")
    with open(mapping, "w") as f:
        f.write("000000\n000001\n000002\n")
    reader = KITTIDetectionDataset(root, mapping)
    assert len(reader) == 3
    pcs, segms, flows, valids = reader[1]
    assert pcs.shape == (2, N_SAMPLE, 3) and np.array_equal(pcs[0], np.load(os.path.join(root, "downsampled", "000001", "pc.npy")))
    assert segms.shape == (2, N_SAMPLE) and segms.max() == len(set(segms[0].tolist())) - 1


@pytest.fixture(scope="module")
def semantickitti(tmp_path_factory):
    from ogc_amd.utils.synthetic import write_semantickitti_raw_root
    root = str(tmp_path_factory.mktemp("semantickitti"))
    written = write_semantickitti_raw_root(root, 2, N_POINTS, sequences=(0, 3))
    return root, written, run_driver("process_semantickitti", root, "--n_sample_point", N_SAMPLE)


def test_semantickitti_driver(semantickitti):
    from ogc_amd.datasets import SemanticKITTIDataset
    root, written, res = semantickitti
    assert sorted(os.listdir(os.path.join(root, "downsampled"))) == ["00_000000", "00_000001", "03_000000", "03_000001"]
    assert "4 frames written" in res.stdout and "0 skipped" in res.stdout
    for sequence, record in written.items():
        for i, words in enumerate(record["labels"]):
            d = os.path.join(root, "downsampled", "%02d_%06d" % (sequence, i))
            pc, segm = np.load(os.path.join(d, "pc.npy")), np.load(os.path.join(d, "segm.npy"))
            assert pc.shape == (N_SAMPLE, 3) and pc.dtype == np.float32 and segm.shape == (N_SAMPLE,) and segm.dtype == np.int64
            scan = np.fromfile(os.path.join(root, "sequences", "%02d" % sequence, "velodyne", "%06d.bin" % i),
                               dtype=np.float32).reshape(-1, 4)
            want_pc, rows = crop_and_sample(scan, record["calib"])
            assert np.array_equal(pc.view(np.int32), want_pc.view(np.int32))
            truth = words[rows]
            kept = sorted(w for w in set(truth.tolist()) if (w & 0xFFFF) in (10, 18, 252, 258))
            assert len(kept) >= 2 and (truth & 0xFFFF == 30).any()
            assert np.array_equal(segm, np.array([kept.index(w) + 1 if w in kept else 0 for w in truth.tolist()]))
    reader = SemanticKITTIDataset(root, sequence_list=[3])
    assert reader.data_ids == ["03_000000", "03_000001"]
    pcs, segms, _, _ = reader[0]
    assert pcs.shape == (2, N_SAMPLE, 3) and segms.shape == (2, N_SAMPLE)


@pytest.fixture(scope="module")
def waymo(tmp_path_factory):
    from ogc_amd.utils.synthetic import write_waymo_raw_root
    root, save = str(tmp_path_factory.mktemp("waymo_raw")), str(tmp_path_factory.mktemp("waymo_out"))
    written = write_waymo_raw_root(root, 2, 3, N_POINTS, box_dtype="float32")
    res = run_driver("process_waymo", "--data_root", root, "--save_root", save, "--split_file", os.path.join(root, "train.txt"),
                     "--cfg_file", os.path.join(ROOT, "config", "waymo_prepare.yaml"))
    return root, save, written, res


def test_waymo_driver(waymo):
    from ogc_amd.data_prepare.scan_ops import crop_front
    from ogc_amd.datasets import WaymoOpenDataset
    from ogc_amd.utils.synthetic import WAYMO_CLASSES, WAYMO_RAW_BOXES
    root, save, written, res = waymo
    assert "6 frames written" in res.stdout and "skipped (unavailable) sequences 1" in res.stdout
    assert sorted(os.listdir(os.path.join(save, "data"))) == sorted(written)
    classes = np.array([0] + [WAYMO_CLASSES.index(n) + 1 if n in WAYMO_CLASSES and counted else 0 for n, counted in WAYMO_RAW_BOXES])
    worst = 0.0
    for seq, frames in written.items():
        d = os.path.join(save, "data", seq)
        assert sorted(os.listdir(d)) == sorted(["%s_%04d.npy" % (w, t) for w in ("pc", "segm", "semantic_segm", "pose") for t in range(3)]
                                              + ["flow_0001_0000.npy", "flow_0002_0001.npy"])
        id_of_box = {}
        for t, frame in enumerate(frames):
            pc, segm, semantic, pose = (np.load(os.path.join(d, "%s_%04d.npy" % (w, t))) for w in ("pc", "segm", "semantic_segm", "pose"))
            scan = np.load(os.path.join(root, "waymo_processed_data", seq, "%04d.npy" % t))
            want_pc, keep_idx = crop_front(torch.from_numpy(scan).cuda())
            want_pc, keep_idx = want_pc.cpu().numpy(), keep_idx.cpu().numpy()
            m = keep_idx.shape[0]
            assert 0 < m < scan.shape[0]
            assert pc.shape == (m, 3) and pc.dtype == np.float32 and np.array_equal(pc, want_pc[:, [1, 2, 0]])
            assert segm.shape == (m,) and segm.dtype == np.int32 and semantic.shape == (m,) and semantic.dtype == np.int32
            assert pose.shape == (4, 4) and pose.dtype == np.float64
            perm = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])
            assert np.array_equal(pose[:3, :3], perm @ frame["pose"][:3, :3] @ perm.T) and np.array_equal(pose[:3, 3], perm @ frame["pose"][:3, 3])
            # labels: the constructed truth up to the id map, one map for the whole sequence
            truth = frame["box"][keep_idx]
            assert np.array_equal(semantic, classes[truth]) and np.array_equal(segm > 0, classes[truth] > 0)
            for b in set(truth[classes[truth] > 0].tolist()):
                got = set(segm[truth == b].tolist())
                assert len(got) == 1
                assert id_of_box.setdefault(b, got.pop()) == segm[truth == b][0]
            if t > 0:
                flow = np.load(os.path.join(d, "flow_%04d_%04d.npy" % (t, t - 1)))
                assert flow.shape == (m, 3) and flow.dtype == np.float64
                p1, p0 = frames[t]["pose"], frames[t - 1]["pose"]
                rot, transl = p0[:3, :3].T @ p1[:3, :3], p0[:3, :3].T @ (p1[:3, 3] - p0[:3, 3])
                lidar = want_pc.astype(np.float64)
                rigid = (lidar @ rot.T + transl - lidar)[:, [1, 2, 0]]
                static = frame["static"][keep_idx]
                worst = max(worst, float(np.abs(flow[static] - rigid[static]).max()))
                assert (~static).any() and np.abs(flow[~static] - rigid[~static]).max() > 0.1     # the moving box has its own flow
        # a bijection into 1 .. 5, the five boxes that label (a box whose points the crop removed takes its id with it)
        assert len(set(id_of_box.values())) == len(id_of_box) >= 3 and set(id_of_box.values()) <= set(range(1, 6))
    print("WAYMO_PREPARE largest |flow - rigid flow of the poses| over static points: %.3e m" % worst)
    assert worst < 1e-6
    reader = WaymoOpenDataset(save, os.path.join(root, "train.txt"))
    assert len(reader) == 4 and reader.n_skipped == 1
    name, t, u = reader.data_ids[0]
    pcs, segms, flows, _ = reader[0]
    d = os.path.join(save, "data", name)
    assert (t, u) == (1, 0) and np.array_equal(pcs[0], np.load(os.path.join(d, "pc_0001.npy"))) and pcs[1].shape[1] == 3
    assert np.array_equal(flows[0], np.load(os.path.join(d, "flow_0001_0000.npy"))) and segms[0].shape == (pcs[0].shape[0],)

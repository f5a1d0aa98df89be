"""The two KITTI Scene Flow preparation drivers (ogc_amd/data_prepare/process_kittisf.py, downsample_kittisf.py), each run in a
fresh child process on a synthetic raw root of 48 x 160 frames (ogc_amd/utils/synthetic.py::write_kittisf_raw_root): processed/
against the mirror of tests/golden/make_kittisf_prepare_golden.py applied to the decoded files, in bits and dtypes; data/ against
the gather by furthest_point_sample's indices done here; the package's reader on the output; the --predflow_path variant; a frame
with too few points."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
N_SAMPLE = 1024
SUBS = ("disp_occ_0", "disp_occ_1", "flow_occ", "instance")


def run_driver(name, *args):
    res = subprocess.run([sys.executable, "-m", "ogc_amd.data_prepare." + name] + [str(a) for a in args], cwd=ROOT,
                         env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-3000:]
    return res


@pytest.fixture(scope="module")
def mirror():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_kittisf_prepare_golden
    return make_kittisf_prepare_golden


@pytest.fixture(scope="module")
def processed(tmp_path_factory):
    """process_kittisf --synthetic 3, after a fourth frame was put there whose second disparity map is mostly empty."""
    from ogc_amd.data_prepare.png16 import read_png, write_png
    from ogc_amd.utils.synthetic import write_kittisf_raw_root
    root = str(tmp_path_factory.mktemp("kittisf_raw"))
    write_kittisf_raw_root(root, 1, 48, 160, seed=9399)                  # frame 0 of another seed, moved to 000003 below
    base = os.path.join(root, "training")
    for sub in SUBS + ("calib_cam_to_cam",):
        ext = ".txt" if sub == "calib_cam_to_cam" else "_10.png"
        os.rename(os.path.join(base, sub, "000000" + ext), os.path.join(base, sub, "000003" + ext))
    disp2 = read_png(os.path.join(base, "disp_occ_1", "000003_10.png"))
    disp2[8:] = 0                                                        # 8 rows of 160 pixels are left: fewer than 1024 points
    write_png(os.path.join(base, "disp_occ_1", "000003_10.png"), disp2)
    res = run_driver("process_kittisf", root, "--synthetic", 3)
    return root, res


def test_process_kittisf_equals_the_mirror(processed, mirror):
    from ogc_amd.data_prepare.kitti_io import read_kittisf_calib
    from ogc_amd.data_prepare.png16 import read_png
    root, res = processed
    assert "4 frames written" in res.stdout
    assert sorted(os.listdir(os.path.join(root, "processed"))) == ["000000", "000001", "000002", "000003"]
    base = os.path.join(root, "training")
    for i in range(4):
        d = os.path.join(root, "processed", "%06d" % i)
        assert sorted(os.listdir(d)) == ["pc1.npy", "pc2.npy", "segm.npy"]
        maps = [read_png(os.path.join(base, sub, "%06d_10.png" % i)) for sub in SUBS]
        assert [m.shape for m in maps] == [(48, 160), (48, 160), (48, 160, 3), (48, 160)] and all(m.dtype == np.uint16 for m in maps)
        P = read_kittisf_calib(os.path.join(base, "calib_cam_to_cam", "%06d.txt" % i))
        assert np.array_equal(P, mirror.p_rect())
        want = mirror.unproject_mirror(*maps, P)
        pc1, pc2, segm = (np.load(os.path.join(d, name + ".npy")) for name in ("pc1", "pc2", "segm"))
        assert pc1.dtype == pc2.dtype == np.float32 and segm.dtype == np.int64
        assert pc1.shape == pc2.shape == want[0].shape and segm.shape == want[2].shape
        assert (want[0].shape[0] > 2 * N_SAMPLE) if i < 3 else (0 < want[0].shape[0] < N_SAMPLE)
        assert np.array_equal(pc1.view(np.int32), want[0].view(np.int32)) and np.array_equal(pc2.view(np.int32), want[1].view(np.int32))
        assert np.array_equal(segm, want[2]) and (i == 3 or len(set(segm.tolist())) >= 3)


def check_downsampled(root, save_root, res, flow_dir, full_flows):
    """data/ of `save_root` against pc[idx], segm[idx], flow[idx] with idx from furthest_point_sample; `full_flows(id, view)` is
    the full-resolution flow a view's file must be gathered from."""
    from ogc_amd.pointnet2.pointnet2 import furthest_point_sample
    ids = ["000000", "000001", "000002"]
    assert "3 scenes written" in res.stdout and "1 skipped" in res.stdout
    assert "scene 000003 skipped" in res.stderr and "fewer than %d" % N_SAMPLE in res.stderr
    assert sorted(os.listdir(os.path.join(save_root, "data"))) == ids
    split = os.path.join(save_root, "all.txt")
    assert open(split).read() == "\n".join(ids) + "\n"
    for data_id in ids:
        src = os.path.join(root, "processed", data_id)
        pcs = [np.load(os.path.join(src, "pc%d.npy" % v)) for v in (1, 2)]
        segm = np.load(os.path.join(src, "segm.npy"))
        d = os.path.join(save_root, "data", data_id)
        names = ["pc", "segm"] + ([] if flow_dir else ["flow"])
        assert sorted(os.listdir(d)) == sorted("%s%d.npy" % (n, v) for n in names for v in (1, 2))
        for v in (0, 1):
            idx = furthest_point_sample(torch.from_numpy(pcs[v])[None].cuda().contiguous(), N_SAMPLE)[0].long().cpu().numpy()
            assert len(set(idx.tolist())) == N_SAMPLE
            pc, sg = np.load(os.path.join(d, "pc%d.npy" % (v + 1))), np.load(os.path.join(d, "segm%d.npy" % (v + 1)))
            flow = np.load(os.path.join(flow_dir, data_id, "flow%d.npy" % (v + 1)) if flow_dir else os.path.join(d, "flow%d.npy" % (v + 1)))
            assert pc.dtype == np.float32 and pc.shape == (N_SAMPLE, 3) and np.array_equal(pc.view(np.int32), pcs[v][idx].view(np.int32))
            assert sg.dtype == np.int32 and np.array_equal(sg, segm[idx])     # label 0 is present: the compression is the identity
            assert flow.dtype == np.float32 and np.array_equal(flow.view(np.int32), full_flows(data_id, v)[idx].view(np.int32))


def check_reader(save_root, predflow_path=None):
    from ogc_amd.datasets import KITTISceneFlowDataset
    ids = ["000000", "000001", "000002"]
    reader = KITTISceneFlowDataset(save_root, os.path.join(save_root, "all.txt"), downsampled=True, view_sels=[[0, 1], [1, 0]],
                                   predflow_path=predflow_path)
    assert len(reader) == 6
    for sid in range(len(reader)):
        pcs, segms, flows, valids = reader[sid]
        assert pcs.shape == flows.shape == (2, N_SAMPLE, 3) and segms.shape == valids.shape == (2, N_SAMPLE)
        d = os.path.join(save_root, "data", ids[sid // 2])
        f = os.path.join(save_root, "flow_preds", predflow_path, ids[sid // 2]) if predflow_path else d
        assert np.array_equal(pcs[0], np.load(os.path.join(d, "pc%d.npy" % (sid % 2 + 1))))
        assert np.array_equal(pcs[1], np.load(os.path.join(d, "pc%d.npy" % (2 - sid % 2))))
        assert np.array_equal(flows[0], np.load(os.path.join(f, "flow%d.npy" % (sid % 2 + 1))))
        assert np.array_equal(flows[1], np.load(os.path.join(f, "flow%d.npy" % (2 - sid % 2))))


def test_downsample_kittisf(processed, tmp_path):
    root, _ = processed
    save_root = str(tmp_path / "down")
    res = run_driver("downsample_kittisf", root, "--save_root", save_root, "--n_sample_point", N_SAMPLE)

    def full_flows(data_id, v):
        src = os.path.join(root, "processed", data_id)
        pcs = [np.load(os.path.join(src, "pc%d.npy" % k)) for k in (1, 2)]
        assert (0 in np.load(os.path.join(src, "segm.npy")))
        return pcs[1 - v] - pcs[v]
    check_downsampled(root, save_root, res, None, full_flows)
    assert not os.path.exists(os.path.join(save_root, "flow_preds"))
    check_reader(save_root)


def test_downsample_kittisf_with_predicted_flows(processed, tmp_path):
    root, _ = processed
    stored = {}
    for i in range(4):
        n = np.load(os.path.join(root, "processed", "%06d" % i, "pc1.npy")).shape[0]
        d = os.path.join(root, "flow_preds", "pred", "%06d" % i)
        os.makedirs(d, exist_ok=True)
        for v in (0, 1):
            stored["%06d" % i, v] = np.random.RandomState(50 + 2 * i + v).randn(n, 3).astype(np.float32)
            np.save(os.path.join(d, "flow%d.npy" % (v + 1)), stored["%06d" % i, v])
    save_root = str(tmp_path / "down_pred")
    res = run_driver("downsample_kittisf", root, "--save_root", save_root, "--predflow_path", "pred", "--n_sample_point", N_SAMPLE)
    check_downsampled(root, save_root, res, os.path.join(save_root, "flow_preds", "pred"), lambda data_id, v: stored[data_id, v])
    # the reader takes the predicted flows IN PLACE of the ground-truth ones, which it still loads (as the reference's does): the
    # run without --predflow_path puts them there, and leaves points and labels as they are
    before = {n: np.load(os.path.join(save_root, "data", "000001", n)) for n in ("pc1.npy", "pc2.npy", "segm1.npy", "segm2.npy")}
    run_driver("downsample_kittisf", root, "--save_root", save_root, "--n_sample_point", N_SAMPLE)
    assert all(np.array_equal(v, np.load(os.path.join(save_root, "data", "000001", n))) for n, v in before.items())
    check_reader(save_root, "pred")

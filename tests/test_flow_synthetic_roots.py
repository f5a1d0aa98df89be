"""The two four-frame synthetic writers of ogc_amd/utils/synthetic.py (write_ogcdr_root, write_sapien_root) and the down-sampled
twin of the KITTI-SF scans (write_kitti_downsampled_root): the existing readers load what they wrote, and the flow the readers
compute from the stored motions moves every object rigidly onto its place in the other frame.  CPU only."""
import json
import os

import numpy as np

VIEW_SELS = [[0, 1], [1, 0], [1, 2], [2, 1], [2, 3], [3, 2]]


def _nearest(a, b):
    """distance from every point of a to its nearest point of b"""
    return np.sqrt(((a[:, None, :].astype(np.float64) - b[None].astype(np.float64)) ** 2).sum(-1)).min(1)


def _check_samples(ds, n_scenes, n_points, same_order):
    assert len(ds) == n_scenes * len(VIEW_SELS)
    moved = 0.0
    for sid in range(len(ds)):
        pcs, segms, flows, valids = ds[sid]
        assert pcs.shape == (2, n_points, 3) and pcs.dtype == np.float32 and flows.shape == (2, n_points, 3)
        assert flows.dtype == np.float32 and segms.shape == (2, n_points) and segms.dtype == np.int32 and valids.min() == 1.0
        assert len(np.unique(segms[0])) >= 3                                  # several objects
        for v in (0, 1):
            landed = pcs[v] + flows[v]
            if same_order:
                assert np.abs(landed - pcs[1 - v]).max() < 1e-5              # onto the same point of the other frame
            else:
                assert _nearest(landed, pcs[1 - v]).max() < 1e-5             # onto SOME point of the other frame: a permutation
            # rigid per object: distances inside an object are kept
            for label in np.unique(segms[v]):
                sel = np.nonzero(segms[v] == label)[0][:16]
                before = np.linalg.norm(pcs[v][sel][:, None] - pcs[v][sel][None], axis=-1)
                after = np.linalg.norm(landed[sel][:, None] - landed[sel][None], axis=-1)
                assert np.abs(before - after).max() < 1e-5
        moved = max(moved, float(np.linalg.norm(flows[0], axis=1).max()))
    assert moved > 0.02                                                       # the flow is not trivial


def test_ogcdr_root_is_read_by_the_data_set(tmp_path):
    from ogc_amd.datasets import OGCDynamicRoomDataset
    from ogc_amd.utils.synthetic import write_ogcdr_root
    root = str(tmp_path / "ogcdr")
    ids = write_ogcdr_root(root, 2, 192, split="val")
    assert len(ids) == 2 and open(os.path.join(root, "data", "val.lst")).read().split() == ids
    for t in range(4):
        assert np.load(os.path.join(root, "data", ids[0], "pose_%02d.npy" % t)).shape == (3, 4, 4)
    ds = OGCDynamicRoomDataset(data_root=root, split="val", view_sels=VIEW_SELS)
    _check_samples(ds, 2, 192, same_order=False)
    # the background (label 0, the smallest id) stays where it is
    pcs, segms, flows, _ = ds[0]
    assert (segms[0] == 0).any() and np.abs(flows[0][segms[0] == 0]).max() == 0.0
    assert np.abs(flows[0][segms[0] != 0]).max() > 0.0


def test_sapien_root_is_read_by_the_data_set(tmp_path):
    from ogc_amd.datasets import SapienDataset
    from ogc_amd.utils.synthetic import write_sapien_root
    root = str(tmp_path / "mbs-shapepart")
    ids = write_sapien_root(root, 2, 160, split="val")
    assert ids == [0, 1] and json.load(open(os.path.join(root, "meta.json"))) == {"val": [0, 1]}
    stored = np.load(os.path.join(root, "data", "000001.npz"), allow_pickle=True)
    assert stored["pc"].shape == (4, 160, 3) and stored["segm"].shape == (4, 160) and stored["segm"].min() >= 1
    assert sorted(map(str, stored["trans"].item())) == ["1", "2", "3", "cam"]
    _check_samples(SapienDataset(data_root=root, split="val", view_sels=VIEW_SELS), 2, 160, same_order=True)


def test_downsampled_twin_of_the_kitti_scans(tmp_path):
    from ogc_amd.datasets import KITTISceneFlowDataset
    from ogc_amd.utils.synthetic import write_kitti_downsampled_root, write_kitti_processed_root
    full, down = str(tmp_path / "kittisf"), str(tmp_path / "kittisf_downsampled")
    mapping, motions = write_kitti_processed_root(full, 2, 512, split="kitti142")
    mapping_down, ids = write_kitti_downsampled_root(full, down, 128, predflow="stored", split="kitti142")
    assert open(mapping).read() == open(mapping_down).read() and len(ids) == 2
    plain = KITTISceneFlowDataset(data_root=down, mapping_path=mapping_down, downsampled=True, view_sels=[[0, 1], [1, 0]])
    pred = KITTISceneFlowDataset(data_root=down, mapping_path=mapping_down, downsampled=True, view_sels=[[0, 1], [1, 0]],
                                 predflow_path="stored")
    for sid in range(4):
        pcs, segms, flows, _ = plain[sid]
        assert pcs.shape == (2, 128, 3) and np.array_equal(flows, pred[sid][2])       # the stored flow is the scan's own
        T = motions[sid // 2] if sid % 2 == 0 else np.linalg.inv(motions[sid // 2])
        rigid = pcs[0].astype(np.float64) @ T[:3, :3].T + T[:3, 3] - pcs[0]
        assert np.abs(flows[0] - rigid).max() < 1e-4                                   # the ego-motion of the scan

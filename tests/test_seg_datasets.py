"""The two single-frame data sets and `_save_predsegm` of ogc_amd/datasets.py (CPU only).

The readers run on trees written by utils/synthetic.py::write_labelled_root and are checked against the reference's sample
contract (datasets/dataset_kittidet.py:73-114, dataset_semantickitti.py:53-85): the frame duplicated to two views, zero flows,
labels compressed per frame, centring on the frame's own mean, valids of ones.  `_save_predsegm` of all five classes must write
the files the reference's own classes write — tests/golden/seg_datasets.json, made from them by
tests/golden/make_seg_datasets_golden.py — with int64 arg-max contents, from a soft mask and from hard labels alike."""
import json
import os

import numpy as np
import pytest
import torch

from ogc_amd import datasets
from ogc_amd.utils.synthetic import SYNTHETIC_SEQUENCES, write_labelled_root

HERE = os.path.dirname(os.path.abspath(__file__))
N_POINTS, N_OBJECTS, N_SCENES = 256, 5, 4


def _check_sample(sample, pc, segm, decentralize):
    pcs, segms, flows, valids = sample
    assert pcs.shape == (2, N_POINTS, 3) and pcs.dtype == np.float32
    assert segms.shape == (2, N_POINTS) and segms.dtype == np.int32
    assert flows.shape == (2, N_POINTS, 3) and flows.dtype == np.float32 and not flows.any()
    assert valids.shape == (2, N_POINTS) and valids.dtype == np.float32 and (valids == 1).all()
    assert np.array_equal(pcs[0], pcs[1]) and np.array_equal(segms[0], segms[1])
    want_pc = pc - pc.mean(0) if decentralize else pc
    assert np.array_equal(pcs[0], want_pc.astype(np.float32))
    # labels on disk are 2 * object + 1: compressed per frame they are the ranks of the labels present
    present = np.unique(segm)
    assert present.min() >= 1 and (present % 2 == 1).all()
    assert np.array_equal(segms[0], np.searchsorted(present, segm).astype(np.int32))
    assert segms[0].max() == len(present) - 1


@pytest.mark.parametrize("decentralize", (False, True))
def test_kittidet_reader(tmp_path, decentralize):
    mapping, ids = write_labelled_root(str(tmp_path), "kittidet", N_SCENES, N_POINTS, N_OBJECTS, seed=11, split="val")
    assert mapping == os.path.join(str(tmp_path), "val.txt") and ids == ["%06d" % i for i in range(N_SCENES)]
    ds = datasets.KITTIDetectionDataset(str(tmp_path), mapping, decentralize=decentralize)
    assert len(ds) == N_SCENES and ds.data_ids == ids
    for i in range(N_SCENES):
        d = os.path.join(str(tmp_path), "downsampled", ids[i])
        _check_sample(ds[i], np.load(os.path.join(d, "pc.npy")), np.load(os.path.join(d, "segm.npy")), decentralize)


def test_semantickitti_reader_and_sequence_filter(tmp_path):
    mapping, ids = write_labelled_root(str(tmp_path), "semantickitti", 7, N_POINTS, N_OBJECTS, seed=12)
    assert mapping is None and len(ids) == 7
    assert [int(name[:2]) for name in ids] == [SYNTHETIC_SEQUENCES[i % 3] for i in range(7)]
    everything = datasets.SemanticKITTIDataset(str(tmp_path))
    assert everything.data_ids == sorted(ids)
    evaluated = datasets.SemanticKITTIDataset(str(tmp_path), sequence_list=list(range(11)), decentralize=True)
    assert evaluated.data_ids == sorted(name for name in ids if int(name[:2]) <= 10) and 0 < len(evaluated) < 7
    one = datasets.SemanticKITTIDataset(str(tmp_path), sequence_list=[8])
    assert one.data_ids == sorted(name for name in ids if name.startswith("08")) and len(one) == 2
    for i in range(len(evaluated)):
        d = os.path.join(str(tmp_path), "downsampled", evaluated.data_ids[i])
        _check_sample(evaluated[i], np.load(os.path.join(d, "pc.npy")), np.load(os.path.join(d, "segm.npy")), True)


def test_augmented_single_frame_sample(tmp_path):
    mapping, _ = write_labelled_root(str(tmp_path), "kittidet", 1, N_POINTS, N_OBJECTS, seed=13)
    args = {"scale_low": 0.95, "scale_high": 1.05, "degree_range": [0, 180, 0], "shift_range": [1, 0.1, 1]}
    pcs, segms, flows, valids = datasets.KITTIDetectionDataset(str(tmp_path), mapping, decentralize=True, aug_transform=True,
                                                               aug_transform_args=args)[0]
    assert pcs.shape == (4, N_POINTS, 3) and segms.shape == (4, N_POINTS) and flows.shape == (4, N_POINTS, 3)
    assert valids.shape == (4, N_POINTS) and np.array_equal(segms[:2], segms[2:]) and not flows.any()


def test_kittisf_layout_of_the_writer(tmp_path):
    mapping, ids = write_labelled_root(str(tmp_path), "kittisf", 2, N_POINTS, N_OBJECTS, seed=14, split="train")
    ds = datasets.KITTISceneFlowDataset(str(tmp_path), mapping, downsampled=True, view_sels=[[0, 1], [1, 0]])
    assert len(ds) == 4 and ds.data_ids == ids
    pcs, segms, flows, valids = ds[0]
    back = ds[1]
    assert pcs.shape == (2, N_POINTS, 3) and segms.dtype == np.int32 and segms.max() == N_OBJECTS - 1
    assert np.array_equal(pcs[0], back[0][1]) and np.array_equal(flows[1], back[2][0])
    with pytest.raises(KeyError):
        write_labelled_root(str(tmp_path), "waymo", 1, N_POINTS, N_OBJECTS)


@pytest.fixture(scope="module")
def pinned():
    with open(os.path.join(HERE, "golden", "seg_datasets.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("as_hard", (False, True))
@pytest.mark.parametrize("name", ("KITTISceneFlowDataset", "OGCDynamicRoomDataset", "SapienDataset", "KITTIDetectionDataset",
                                  "SemanticKITTIDataset"))
def test_save_predsegm_writes_the_reference_files(tmp_path, pinned, name, as_hard):
    spec = pinned["classes"][name]
    ds = object.__new__(getattr(datasets, name))        # `_save_predsegm` reads nothing but the ids
    ds.data_ids = spec["data_ids"]
    g = torch.Generator().manual_seed(3)
    want = {}
    for c in spec["calls"]:
        mask = torch.softmax(torch.rand(c["B"], pinned["n"], pinned["k"], generator=g), dim=2)
        hard = mask.numpy().argmax(2)
        given = (torch.from_numpy(hard).to(torch.int32) if c["offset"] % 2 else hard) if as_hard else mask
        ds._save_predsegm(given, save_root=str(tmp_path), batch_size=c["batch_size"], n_frame=c["n_frame"], offset=c["offset"])
        for i in range(c["B"]):
            want[c["offset"] * c["batch_size"] + i] = hard[i]
    files = sorted(os.path.relpath(os.path.join(d, f), str(tmp_path)) for d, _, fs in os.walk(str(tmp_path)) for f in fs)
    assert files == spec["files"]
    # sample s of the loader is file s in (scene, frame) order: the sorted list of the fixture for these ids and names
    assert len(want) == len(files)
    for s, rel in enumerate(files):
        stored = np.load(os.path.join(str(tmp_path), rel))
        assert str(stored.dtype) == spec["dtype"] == "int64" and np.array_equal(stored, want[s])


def test_save_predsegm_refuses_other_shapes(tmp_path):
    ds = object.__new__(datasets.KITTIDetectionDataset)
    ds.data_ids = ["a"]
    with pytest.raises(ValueError):
        ds._save_predsegm(np.zeros(8), save_root=str(tmp_path), batch_size=1)


def test_driver_settings_follow_the_reference(tmp_path):
    """Checkpoint path, frames per scene, view selections and ignore threshold of ogc_amd.test_seg (test_seg.py:80-116)."""
    from ogc_amd import test_seg
    assert test_seg.weight_path({"save_path": "ckpt/seg/x"}, 0) == os.path.join("ckpt/seg/x", "best.pth.tar")
    assert test_seg.weight_path({"save_path": "ckpt/seg/x"}, 2) == os.path.join("ckpt/seg/x_R2", "best.pth.tar")
    for layout, n_frame in (("kittisf", 2), ("kittidet", 1), ("semantickitti", 1)):
        root = str(tmp_path / layout)
        mapping, ids = write_labelled_root(root, layout, 4, 64, 3, seed=5)
        cfg = {"dataset": layout, "data": {"decentralize": True}}
        ds, frames, thresh, seen_root = test_seg.build_test_set(cfg, "val", root, mapping)
        assert (frames, thresh, seen_root) == (n_frame, 50, root) and ds.decentralize
        assert len(ds) == (sum(int(i[:2]) <= 10 for i in ids) if layout == "semantickitti" else 4 * n_frame)
        if layout == "kittisf":
            assert ds.view_sels == [[0, 1], [1, 0]] and ds.downsampled
    assert test_seg.INDOOR_VIEW_SELS == [[0, 1], [1, 2], [2, 3], [3, 2]]
    with pytest.raises(KeyError):
        test_seg.build_test_set({"dataset": "waymo"}, "val", str(tmp_path))

"""ogc_amd.datasets.WaymoSingleFrameDataset against THE REFERENCE'S OWN datasets/dataset_waymo_singleframe.py on the seeded
synthetic root of utils/synthetic.py::write_waymo_singleframe_roots (tests/golden/waymo_singleframe.npz, written by
tests/golden/make_waymo_singleframe_golden.py; the cases are in tests/waymo_sf_cases.py): the sample ids, and every array of the
first and the last sample of every case, EXACTLY — all four combinations of onehot_label and aug_transform (numpy's global
generator seeded before the sample is read), downsampled=False, select_frame, sampled_interval, no filtering — and the files
`_save_predsegm` writes.  CPU only."""
import os

import numpy as np
import pytest
import torch

import waymo_sf_cases as wc

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "waymo_singleframe.npz"))


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("waymo_sf"))
    return tmp, wc.write_root(tmp)


@pytest.mark.parametrize("tag,split,kwargs", wc.CASES, ids=[c[0] for c in wc.CASES])
def test_samples_equal_the_reference_readers(golden, root, tag, split, kwargs):
    from ogc_amd.datasets import WaymoSingleFrameDataset
    tmp, made = root
    ds = WaymoSingleFrameDataset(**wc.reader_kwargs(tmp, made, split, kwargs))
    assert len(ds) == int(golden[tag + "/len"][0])
    assert ["%s:%d" % i for i in ds.data_ids] == list(golden[tag + "/ids"])
    assert ds.n_skipped == 1 if "select_frame" not in kwargs else not hasattr(ds, "n_skipped")
    for sid in (0, len(ds) - 1):
        np.random.seed(wc.SEED + sid)
        sample = ds[sid]
        assert len(sample) == 3
        for name, value in zip(("pcs", "segms", "valids"), sample):
            want = golden["%s/%d/%s" % (tag, sid, name)]
            if not kwargs.get("downsampled", True):
                assert isinstance(value, list) and len(value) == 1
                value = value[0]
            assert value.dtype == want.dtype and value.shape == want.shape, (tag, sid, name, value.dtype, value.shape)
            assert np.array_equal(value, want), (tag, sid, name)


def test_shapes_dtypes_and_the_ignore_mask(root):
    """The contract the drivers rely on, spelled out: (1, N, 3) / (1, N) / (1, N) without augmentation, two entries with it; i32
    labels and valids, f32 one-hot labels and valids; one-hot rows of ignored points are zero; both ignore rules act."""
    from ogc_amd.datasets import WaymoSingleFrameDataset
    tmp, made = root
    n = wc.N_POINTS
    by_tag = {c[0]: c for c in wc.CASES}
    get = lambda tag: WaymoSingleFrameDataset(**wc.reader_kwargs(tmp, made, by_tag[tag][1], by_tag[tag][2]))[0]  # noqa: E731
    pcs, segms, valids = get("plain")
    assert pcs.shape == (1, n, 3) and segms.shape == valids.shape == (1, n)
    assert pcs.dtype == np.float32 and segms.dtype == valids.dtype == np.int32
    assert 0 < (valids == 0).sum() < n and not segms[valids == 0].any()
    d = os.path.join(tmp, "data", made["train"]["names"][0])
    raw, semantic = np.load(os.path.join(d, "segm_0000.npy")), np.load(os.path.join(d, "semantic_segm_0000.npy"))
    by_class = np.isin(semantic, [2, 3])
    ids, sizes = np.unique(raw, return_counts=True)
    by_size = np.isin(raw, ids[sizes < wc.THRESH])
    assert by_class.any() and by_size.any() and (by_size & ~by_class).any() and (semantic == 3).any() and (semantic == 2).any()
    assert np.array_equal(valids[0] == 0, by_class | by_size)
    pcs, onehot, fvalids = get("onehot")
    assert onehot.shape == (1, n, 12) and onehot.dtype == fvalids.dtype == np.float32
    assert np.array_equal(onehot.sum(2), fvalids) and np.array_equal(onehot.argmax(2) * (fvalids > 0), segms)
    np.random.seed(0)
    pcs, segms2, valids2 = get("aug")
    assert pcs.shape == (2, n, 3) and segms2.shape == valids2.shape == (2, n)
    assert np.array_equal(segms2[0], segms2[1]) and np.array_equal(segms2[0], segms[0]) and not np.array_equal(pcs[0], pcs[1])


def test_save_predsegm(golden, root, tmp_path):
    from ogc_amd.datasets import WaymoSingleFrameDataset
    tmp, made = root
    tag, split, kwargs = wc.CASES[0]
    ds = WaymoSingleFrameDataset(**wc.reader_kwargs(tmp, made, split, kwargs))
    masks = wc.save_masks()
    out = str(tmp_path / "saved")
    for offset in range(masks.shape[0] // wc.SAVE_BATCH):
        part = masks[offset * wc.SAVE_BATCH:(offset + 1) * wc.SAVE_BATCH]
        # soft masks as a tensor in the first batch, hard labels as an array after it: both forms the drivers pass
        ds._save_predsegm(torch.from_numpy(part) if offset == 0 else part.argmax(2), out, wc.SAVE_BATCH, n_frame=1, offset=offset)
    want = sorted(k for k in golden.files if k.startswith("save/"))
    got = sorted("save/%s/%s" % (seq, f[:-4]) for seq in os.listdir(out) for f in os.listdir(os.path.join(out, seq)))
    assert got == want and len(got) == 6 and all(k.rsplit("/", 1)[1].startswith("segm_") for k in got)
    for key in want:
        _, seq, name = key.split("/")
        value = np.load(os.path.join(out, seq, name + ".npy"))
        assert value.dtype == golden[key].dtype and np.array_equal(value, golden[key]), key

"""KITTIDetectionDataset with `load_prediction` / `load_confidence` against the REFERENCE's own class
(tests/golden/selftrain_reader.npz, written by tests/golden/make_selftrain_golden.py: 4 frames of 96 points, predicted labels
with gaps in their ids and an object below the threshold, confidences in (0, 1), max_n_object 8, augmentation off).  The test
writes the fixture's root again and asks for the same arrays: integers exactly equal, float32 arrays equal in every bit.  Cases:
ground truth, predictions, predictions with confidences; each with ignore_npoint_thresh 0 and 12, with and without
onehot_label."""
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _recipe():
    spec = importlib.util.spec_from_file_location("make_selftrain_golden", os.path.join(HERE, "golden", "make_selftrain_golden.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


R = _recipe()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "selftrain_reader.npz"))


@pytest.fixture()
def root(golden, tmp_path):
    return str(tmp_path), R.write_root(str(tmp_path), golden)


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


@pytest.mark.parametrize("case", list(R.CASES))
def test_reader_returns_the_reference_readers_samples(golden, root, case):
    from ogc_amd.datasets import KITTIDetectionDataset
    ds = KITTIDetectionDataset(**R.reader_kwargs(*root, case))
    assert len(ds) == R.N_FRAME
    onehot = R.CASES[case][3]
    for sid in range(R.N_FRAME):
        sample = ds[sid]
        assert len(sample) == 4
        for name, value in zip(R.NAMES, sample):
            want = golden["%s/%d/%s" % (case, sid, name)]
            assert same(value, want), (case, sid, name)
        assert sample[1].dtype == (np.float32 if onehot else np.int32)


def test_the_fixture_exercises_what_it_is_for(golden):
    """Gaps in the predicted ids, an object below the threshold, confidences that reach the targets, a dropped object's column
    taken out together with its confidence."""
    for i in range(R.N_FRAME):
        labels, sizes = np.unique(golden["pred%d" % i], return_counts=True)
        assert list(labels) != list(range(len(labels))) and len(golden["conf%d" % i]) == len(labels)
        assert ((golden["conf%d" % i] > 0) & (golden["conf%d" % i] < 1)).all()
    labels, sizes = np.unique(golden["pred1"], return_counts=True)
    assert sizes.min() == R.SMALL_OBJECT_POINTS < 12
    conf = golden["conf1"].astype(np.float32)
    full, cut = golden["conf_t0_onehot/1/segms"][0], golden["conf_t12_onehot/1/segms"][0]
    # column j holds conf[j] at the points of the j-th label and 0 elsewhere
    for j in range(len(labels)):
        assert set(np.unique(full[:, j])) == {np.float32(0), conf[j]}
    assert not full[:, len(labels):].any()
    kept = [j for j in range(len(labels)) if sizes[j] >= 12]
    assert len(kept) == len(labels) - 1
    for col, j in enumerate(kept):
        assert set(np.unique(cut[:, col])) == {np.float32(0), conf[j]}
    assert golden["conf_t12_onehot/1/valids"][0].sum() == R.N_POINT - R.SMALL_OBJECT_POINTS
    assert not np.array_equal(golden["pred_t0_onehot/1/segms"], full)      # without confidences: ones


def test_default_arguments_read_the_ground_truth_as_before(golden, root):
    from ogc_amd.datasets import KITTIDetectionDataset
    from ogc_amd.utils.data_util import batch_segm_to_mask, compress_label_id
    data_root, mapping = root
    for onehot in (False, True):
        ds = KITTIDetectionDataset(data_root=data_root, mapping_path=mapping, decentralize=True, onehot_label=onehot,
                                   max_n_object=R.MAX_N_OBJECT, ignore_npoint_thresh=12)
        assert ds.predsegm_path is None and ds.load_confidence is False
        for sid in range(R.N_FRAME):
            pc, segm = golden["pc%d" % sid], compress_label_id(golden["segm%d" % sid].copy())
            pcs, segms, flows, valids = ds[sid]
            pc = pc - pc.mean(0)
            assert same(pcs, np.stack([pc, pc], 0).astype(np.float32)) and same(flows, np.zeros((2, R.N_POINT, 3), np.float32))
            if onehot:
                want, want_valid = batch_segm_to_mask(np.stack([segm, segm], 0), R.MAX_N_OBJECT, 12)
                assert same(segms, want.astype(np.float32)) and same(valids, want_valid.astype(np.float32))
            else:
                assert same(segms, np.stack([segm, segm], 0).astype(np.int32)) and same(valids, np.ones((2, R.N_POINT), np.float32))
            tag = "gt_t12_%s" % ("onehot" if onehot else "labels")
            assert same(segms, golden["%s/%d/segms" % (tag, sid)]) and same(valids, golden["%s/%d/valids" % (tag, sid)])


def test_load_confidence_without_the_file_raises(golden, root):
    from ogc_amd.datasets import KITTIDetectionDataset
    data_root, mapping = root
    os.remove(os.path.join(data_root, "segm_preds", R.PRED_NAME, R.IDS[2], "conf.npy"))
    ds = KITTIDetectionDataset(**R.reader_kwargs(data_root, mapping, "conf_t0_onehot"))
    ds[1]
    with pytest.raises(FileNotFoundError):
        ds[2]
    KITTIDetectionDataset(**R.reader_kwargs(data_root, mapping, "pred_t0_onehot"))[2]   # ones: the file is not asked for


def test_save_predsegm_writes_confidences_the_reader_returns(golden, root, tmp_path):
    from ogc_amd.datasets import KITTIDetectionDataset
    data_root, mapping = root
    ds = KITTIDetectionDataset(**R.reader_kwargs(data_root, mapping, "conf_t0_onehot"))
    save_root = os.path.join(data_root, "segm_preds", "P1")
    hard = np.stack([golden["pred%d" % i] for i in range(R.N_FRAME)], 0)
    conf = [golden["conf%d" % i] for i in range(R.N_FRAME)]
    # two batches of two, as a loader with batch_size 2 hands them over
    for offset in (0, 1):
        ds._save_predsegm(hard[2 * offset:2 * offset + 2], save_root, batch_size=2, offset=offset, conf=conf[2 * offset:2 * offset + 2])
    for i, idx in enumerate(R.IDS):
        assert sorted(os.listdir(os.path.join(save_root, idx))) == ["conf.npy", "segm.npy"]
        saved = np.load(os.path.join(save_root, idx, "conf.npy"))
        assert saved.dtype == np.float32 and same(saved, conf[i].astype(np.float32))
        assert same(np.load(os.path.join(save_root, idx, "segm.npy")), golden["pred%d" % i])
    again = KITTIDetectionDataset(**dict(R.reader_kwargs(data_root, mapping, "conf_t0_onehot"), load_prediction="P1"))
    for sid in range(R.N_FRAME):
        for got, want in zip(again[sid], ds[sid]):
            assert same(got, want)
    # without conf: segm.npy alone, as before
    ds._save_predsegm(hard[:2], os.path.join(data_root, "segm_preds", "P2"), batch_size=2, offset=0)
    assert os.listdir(os.path.join(data_root, "segm_preds", "P2", R.IDS[0])) == ["segm.npy"]


def test_export_refuses_masks_and_labels_that_do_not_belong_together(monkeypatch, tmp_path):
    """export_pseudo_labels pairs the masks of a batch with the hard labels test_seg.evaluate hands its saver; an evaluate that
    called the network twice, or not at all, before the saver must not get anything written."""
    import torch
    from ogc_amd import export_pseudo_labels, test_seg

    def evaluate_calling_the_network(times):
        def evaluate(segnet, loader, n_frame, ignore_npoint_thresh, saver=None, device="cuda"):
            for _ in range(times):
                segnet(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3))
            saver(torch.zeros(1, 4, dtype=torch.int32), 0)
        return evaluate

    for times in (0, 2):
        monkeypatch.setattr(test_seg, "evaluate", evaluate_calling_the_network(times))
        with pytest.raises(RuntimeError, match="%d network calls" % times):
            export_pseudo_labels.export(lambda a, b: torch.zeros(1, 4, 2), None, None, 0, str(tmp_path), 1)
    assert os.listdir(str(tmp_path)) == []

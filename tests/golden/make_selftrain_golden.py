"""Generates tests/golden/selftrain_reader.npz by running the REFERENCE's own KITTIDetectionDataset
(datasets/dataset_kittidet.py, imported from the reference checkout that make_golden.py names, which exists only in the build
container) on the CPU, with `load_prediction` and `load_confidence`:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_selftrain_golden.py

The root: 4 frames of 96 points under downsampled/<id>/{pc,segm}.npy, and for each a predicted segmentation under
segm_preds/P0/<id>/{segm,conf}.npy whose label ids have gaps, one object of fewer than 12 points, and one confidence in (0, 1)
per distinct label (the last frame's stored as float64: the reader casts).  max_n_object is 8, augmentation is off.  The fixture
holds these inputs and, for every case of CASES, the four arrays of every sample.  tests/test_selftrain_reader_cpu.py writes
the same root again with `write_root` and asks this package's reader for the same bits.  Only data is written."""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))

N_FRAME, N_POINT, MAX_N_OBJECT, PRED_NAME = 4, 96, 8, "P0"
IDS = ["%06d" % (7 * i + 3) for i in range(N_FRAME)]
PRED_LABELS = np.array([0, 2, 3, 7, 9, 12])          # gaps; at most six of the eight columns are used
SMALL_OBJECT_POINTS = 5                              # of label 9 in every frame: below the threshold of 12
# tag -> (load_prediction, load_confidence, ignore_npoint_thresh, onehot_label)
CASES = {"%s_t%d_%s" % (("gt", "pred", "conf")[mode], thresh, "onehot" if onehot else "labels"):
         ((None, PRED_NAME, PRED_NAME)[mode], mode == 2, thresh, onehot)
         for mode in (0, 1, 2) for thresh in (0, 12) for onehot in (True, False)}
NAMES = ("pcs", "segms", "flows", "valids")


def draw_inputs(seed=8100):
    rng = np.random.default_rng(seed)
    arrays = {}
    for i in range(N_FRAME):
        arrays["pc%d" % i] = (rng.standard_normal((N_POINT, 3)) * np.array([20.0, 1.0, 20.0]) + np.array([0.0, 0.0, 30.0])).astype(np.float32)
        arrays["segm%d" % i] = rng.integers(0, 5, N_POINT).astype(np.int64) * 3      # ground truth: ids 0, 3, ..., 12
        labels = PRED_LABELS[:4 + i % 3]                                             # 4, 5 or 6 predicted objects
        pred = labels[rng.integers(0, len(labels), N_POINT)]
        if 9 in labels:
            pred[pred == 9] = 0
            pred[rng.permutation(N_POINT)[:SMALL_OBJECT_POINTS]] = 9
        arrays["pred%d" % i] = pred.astype(np.int64)
        conf = rng.uniform(0.05, 0.95, len(np.unique(pred))).astype(np.float32)
        arrays["conf%d" % i] = conf.astype(np.float64) if i == N_FRAME - 1 else conf
    return arrays


def write_root(root, arrays):
    """The root of the fixture's inputs -> the path of its split file."""
    for i, idx in enumerate(IDS):
        d = os.path.join(root, "downsampled", idx)
        os.makedirs(d)
        np.save(os.path.join(d, "pc.npy"), arrays["pc%d" % i])
        np.save(os.path.join(d, "segm.npy"), arrays["segm%d" % i])
        d = os.path.join(root, "segm_preds", PRED_NAME, idx)
        os.makedirs(d)
        np.save(os.path.join(d, "segm.npy"), arrays["pred%d" % i])
        np.save(os.path.join(d, "conf.npy"), arrays["conf%d" % i])
    mapping = os.path.join(root, "train.txt")
    with open(mapping, "w") as f:
        f.write("\n".join(IDS) + "\n")
    return mapping


def reader_kwargs(root, mapping, case):
    load_prediction, load_confidence, thresh, onehot = CASES[case]
    kw = dict(data_root=root, mapping_path=mapping, decentralize=True, aug_transform=False, aug_transform_args=None,
              onehot_label=onehot, max_n_object=MAX_N_OBJECT, ignore_npoint_thresh=thresh)
    if load_prediction is not None:
        kw.update(load_prediction=load_prediction, load_confidence=load_confidence)
    return kw


def main():
    import importlib.util
    import tempfile

    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    sys.path.insert(0, os.path.dirname(HERE))
    import make_golden
    make_golden.install_shims()
    spec = importlib.util.spec_from_file_location("ref_dataset_kittidet", os.path.join(make_golden.REF, "datasets", "dataset_kittidet.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    arrays = draw_inputs()
    for i in range(N_FRAME):
        sizes = np.unique(arrays["pred%d" % i], return_counts=True)
        assert 0 < sizes[1].min() and (i % 3 == 0 or sizes[1][list(sizes[0]).index(9)] == SMALL_OBJECT_POINTS), sizes
        assert list(sizes[0]) != list(range(len(sizes[0]))) and len(sizes[0]) <= MAX_N_OBJECT
    out = dict(arrays)
    with tempfile.TemporaryDirectory() as tmp:
        mapping = write_root(tmp, arrays)
        for case in CASES:
            ds = ref.KITTIDetectionDataset(**reader_kwargs(tmp, mapping, case))
            assert len(ds) == N_FRAME
            for sid in range(N_FRAME):
                for name, value in zip(NAMES, ds[sid]):
                    out["%s/%d/%s" % (case, sid, name)] = value
            print("%-18s segms %s %s" % (case, out[case + "/0/segms"].shape, out[case + "/0/segms"].dtype))
    make_golden.save("selftrain_reader", **out)


if __name__ == "__main__":
    main()

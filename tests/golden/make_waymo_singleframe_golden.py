"""Writes tests/golden/waymo_singleframe.npz: samples of THE REFERENCE'S OWN datasets/dataset_waymo_singleframe.py
WaymoOpenDataset (imported from /root/reference at generation time only) on the seeded synthetic root of
ogc_amd/utils/synthetic.py::write_waymo_singleframe_roots, for ogc_amd.datasets.WaymoSingleFrameDataset.  CPU only; only data is
written.  tests/test_waymo_singleframe.py writes the same root again (same arguments) and compares exactly.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_waymo_singleframe_golden.py

Per case of CASES (tests/waymo_sf_cases.py): `<tag>/len`, `<tag>/ids` (the sample ids as "sequence:t") and, for the first and the
last sample, `<tag>/<sid>/pcs | segms | valids`.  The augmented cases seed numpy's global generator with SEED + sid right before
the sample is read, as the test does.  `save/<sequence>/segm_%04d` holds what `_save_predsegm` wrote for the masks of
waymo_sf_cases.save_masks()."""
import os
import sys
import tempfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import waymo_sf_cases as wc  # noqa: E402
from make_golden import install_shims, save  # noqa: E402


def main():
    import importlib.util
    install_shims()
    spec = importlib.util.spec_from_file_location("ref_dataset_waymo_singleframe",
                                                  "/root/reference/datasets/dataset_waymo_singleframe.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    arrays = {}
    with tempfile.TemporaryDirectory() as tmp:
        made = wc.write_root(tmp)
        for tag, split, kwargs in wc.CASES:
            ds = mod.WaymoOpenDataset(**wc.reader_kwargs(tmp, made, split, kwargs))
            arrays[tag + "/len"] = np.array([len(ds)])
            arrays[tag + "/ids"] = np.array(["%s:%d" % tuple(i) for i in ds.data_ids])
            for sid in (0, len(ds) - 1):
                np.random.seed(wc.SEED + sid)
                for name, value in zip(("pcs", "segms", "valids"), ds[sid]):
                    arrays["%s/%d/%s" % (tag, sid, name)] = value[0] if isinstance(value, list) else value
                assert isinstance(ds[sid][0], list) == (not kwargs.get("downsampled", True))
            print("%-22s %d samples, segms %s %s" % (tag, len(ds), arrays[tag + "/0/segms"].shape, arrays[tag + "/0/segms"].dtype))
        # the ignore mask of the root is not empty, and neither rule alone explains it
        valid = arrays["plain/0/valids"]
        assert 0 < int((valid == 0).sum()) < valid.size
        tag, split, kwargs = wc.CASES[0]
        ds = mod.WaymoOpenDataset(**wc.reader_kwargs(tmp, made, split, kwargs))
        out = os.path.join(tmp, "saved")
        masks = wc.save_masks()
        for offset in range(masks.shape[0] // wc.SAVE_BATCH):
            ds._save_predsegm(torch.from_numpy(masks[offset * wc.SAVE_BATCH:(offset + 1) * wc.SAVE_BATCH]), out, wc.SAVE_BATCH,
                              n_frame=1, offset=offset)
        for seq in sorted(os.listdir(out)):
            for f in sorted(os.listdir(os.path.join(out, seq))):
                arrays["save/%s/%s" % (seq, f[:-4])] = np.load(os.path.join(out, seq, f))
    save("waymo_singleframe", **arrays)


if __name__ == "__main__":
    main()

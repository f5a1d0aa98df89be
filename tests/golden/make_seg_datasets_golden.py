"""Writes tests/golden/seg_datasets.json: the files THE REFERENCE'S OWN data-set classes (imported from /root/reference at
generation time only) write in `_save_predsegm`, for the five classes of ogc_amd/datasets.py that carry that method.  CPU only.

    python tests/golden/make_seg_datasets_golden.py

Per class: the data ids given to it, the calls made (batch shape, batch_size, n_frame, offset), the relative paths of the files
found afterwards, sorted, and their dtype.  `_save_predsegm` reads nothing but `self.data_ids`, so the instances are made without
their constructors (no data set is on this machine); pyquaternion, which the SAPIEN module imports and this image lacks, and
the reference's native extension are replaced by empty modules for the import.  Nothing from the reference is copied: only names and dtypes are written.
"""
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
OUT = os.path.join(HERE, "seg_datasets.json")

# class -> (module, data ids, n_frame)
CLASSES = {
    "KITTISceneFlowDataset": ("datasets.dataset_kittisf", ["000000", "000003", "000007", "000012"], 2),
    "OGCDynamicRoomDataset": ("datasets.dataset_ogcdr", ["room_a/00000001", "room_a/00000005", "room_b/00000002", "room_b/00000009"], 4),
    "SapienDataset": ("datasets.dataset_sapien", [3, 17, 120, 4051], 4),
    "KITTIDetectionDataset": ("datasets.dataset_kittidet", ["000001", "000002", "000010", "000011", "007480"], 1),
    "SemanticKITTIDataset": ("datasets.dataset_semantickitti", ["00_000000", "00_000005", "08_000001", "08_000004", "10_000002"], 1),
}
N, K = 16, 5


def calls_of(n_ids, n_frame):
    """Two batches that cover every (scene, frame): batch_size = 2 * n_frame, a last batch that may be short."""
    batch_size = 2 * n_frame
    total = n_ids * n_frame
    return [{"B": min(batch_size, total - o * batch_size), "batch_size": batch_size, "n_frame": n_frame, "offset": o}
            for o in range((total + batch_size - 1) // batch_size)]


def main():
    assert os.path.isdir(REF), "the reference tree is only present in the build container"
    sys.path.insert(0, REF)
    # the modules pull in the native operators and pyquaternion at import; `_save_predsegm` uses neither
    sys.modules.setdefault("pointnet2_cuda", types.ModuleType("pointnet2_cuda"))
    sys.modules.setdefault("pyquaternion", types.ModuleType("pyquaternion"))
    sys.modules["pyquaternion"].Quaternion = object
    import importlib.util

    import torch
    out = {"n": N, "k": K, "classes": {}}
    g = torch.Generator().manual_seed(0)
    for name, (module, ids, n_frame) in CLASSES.items():
        # by its path: another top-level package named `datasets` may be installed
        spec = importlib.util.spec_from_file_location("ref_" + module.replace(".", "_"), os.path.join(REF, *module.split(".")) + ".py")
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        cls = getattr(mod, name)
        ds = object.__new__(cls)
        ds.data_ids = ids
        calls = calls_of(len(ids), n_frame)
        with tempfile.TemporaryDirectory() as tmp:
            for c in calls:
                mask = torch.softmax(torch.rand(c["B"], N, K, generator=g), dim=2)
                ds._save_predsegm(mask, save_root=tmp, batch_size=c["batch_size"], n_frame=c["n_frame"], offset=c["offset"])
            files = sorted(os.path.relpath(os.path.join(d, f), tmp) for d, _, fs in os.walk(tmp) for f in fs)
            dtypes = sorted({str(np.load(os.path.join(tmp, f)).dtype) for f in files})
            shapes = sorted({np.load(os.path.join(tmp, f)).shape for f in files})
        assert dtypes == ["int64"] and shapes == [(N,)], (dtypes, shapes)
        out["classes"][name] = {"data_ids": ids, "calls": calls, "files": files, "dtype": dtypes[0]}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote %s" % OUT)


if __name__ == "__main__":
    main()

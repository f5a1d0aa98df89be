"""KITTI Scene Flow preparation, stage 2 (reference: data_prepare/kittisf/downsample_kittisf.py): processed/<id>/{pc1,pc2,segm}.npy
-> <save_root>/data/<id>/{pc,segm,flow}{1,2}.npy, what KITTISceneFlowDataset(downsampled=True) reads.

    python -m ogc_amd.data_prepare.downsample_kittisf <data_root> --save_root <root> [--predflow_path NAME] [--n_sample_point 8192]

The scenes are those processed/ holds (the reference reads a list of 200).  Per scene and per view — KITTISceneFlowDataset over
the full-resolution frames with view_sels [[0, 1], [1, 0]] — furthest point sampling on the device (ogc_furthest_point_sampling)
picks n_sample_point points of the view's first frame; points, labels and flows are gathered by its indices.  With
--predflow_path the flows are the predictions under <data_root>/flow_preds/NAME and go to <save_root>/flow_preds/NAME/<id>/
flow{1,2}.npy instead.  The ids written are listed in <save_root>/<split>.txt.  A scene with fewer than n_sample_point points is
skipped, named on stderr and counted: the reference's FPS would repeat indices there.
"""
import argparse
import os
import sys
import tempfile

import numpy as np
import torch

from ..datasets import KITTISceneFlowDataset
from ..utils.data_util import fps_downsample

VIEW_SELS = [[0, 1], [1, 0]]


def scene_ids(processed_root):
    return sorted(d for d in os.listdir(processed_root) if os.path.isfile(os.path.join(processed_root, d, "pc1.npy")))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("data_root", type=str, help="Root path for the dataset")
    ap.add_argument("--save_root", type=str, required=True, help="Path to save the downsampled dataset")
    ap.add_argument("--predflow_path", type=str, default=None, help="Path to load pre-saved flow predictions")
    ap.add_argument("--n_sample_point", type=int, default=8192)
    ap.add_argument("--split", type=str, default="all", help="name of the split file written under save_root")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("downsample_kittisf needs a HIP device; ogc_amd has no CPU path")
    save_dir = os.path.join(args.save_root, "data")
    os.makedirs(save_dir, exist_ok=True)
    flow_dir = None
    if args.predflow_path is not None:
        flow_dir = os.path.join(args.save_root, "flow_preds", args.predflow_path)
        os.makedirs(flow_dir, exist_ok=True)
    ids = scene_ids(os.path.join(args.data_root, "processed"))
    with tempfile.TemporaryDirectory() as tmp:
        mapping = os.path.join(tmp, "scenes.txt")
        with open(mapping, "w") as f:
            f.write("\n".join(ids) + "\n")
        dataset = KITTISceneFlowDataset(data_root=args.data_root, mapping_path=mapping, downsampled=False, view_sels=VIEW_SELS,
                                        predflow_path=args.predflow_path)
    written = []
    for idx, data_id in enumerate(ids):
        samples = [dataset[idx * len(VIEW_SELS) + v] for v in range(len(VIEW_SELS))]
        n_point = min(s[0][0].shape[0] for s in samples)
        if n_point < args.n_sample_point:
            print("downsample_kittisf: scene %s skipped, it has %d points, fewer than %d" % (data_id, n_point, args.n_sample_point),
                  file=sys.stderr)
            continue
        save_path = os.path.join(save_dir, data_id)
        os.makedirs(save_path, exist_ok=True)
        for v, (pcs, segms, flows, _) in enumerate(samples):
            fps_idx = fps_downsample(pcs[0], n_sample_point=args.n_sample_point)
            np.save(os.path.join(save_path, "pc%d.npy" % (v + 1)), pcs[0][fps_idx])
            np.save(os.path.join(save_path, "segm%d.npy" % (v + 1)), segms[0][fps_idx])
            if flow_dir is not None:
                os.makedirs(os.path.join(flow_dir, data_id), exist_ok=True)
                np.save(os.path.join(flow_dir, data_id, "flow%d.npy" % (v + 1)), flows[0][fps_idx])
            else:
                np.save(os.path.join(save_path, "flow%d.npy" % (v + 1)), flows[0][fps_idx])
        written.append(data_id)
    split_file = os.path.join(args.save_root, args.split + ".txt")
    with open(split_file, "w") as f:
        f.write("\n".join(written) + "\n")
    skipped = len(ids) - len(written)
    print("downsample_kittisf: %d scenes written to %s, %d skipped; split file %s" % (len(written), save_dir, skipped, split_file))
    return {"scenes": len(written), "skipped": skipped, "split_file": split_file}


if __name__ == "__main__":
    main()

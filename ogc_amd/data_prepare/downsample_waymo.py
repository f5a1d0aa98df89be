"""Waymo preparation, stage 2 (reference: data_prepare/waymo/downsample_waymo.py): the full-resolution root process_waymo writes
-> <save_root>/data/<sequence>/{pc,segm,semantic_segm}_%04d.npy and flow_%04d_%04d.npy with n_sample_point points per frame, what
WaymoOpenDataset / WaymoSingleFrameDataset(downsampled=True) read.

    python -m ogc_amd.data_prepare.downsample_waymo --data_root R --save_root S --split_file F [--predflow_path NAME]
                                                    [--n_sample_point 8192] [--synthetic N]

Over the frame pairs (t, t - 1) of WaymoOpenDataset(downsampled=False): furthest point sampling on the device
(ogc_furthest_point_sampling) picks n_sample_point points of frame t; points, both label arrays and the backward flow are gathered
by its indices.  Frame t - 1 is sampled and written only for the pair (1, 0) — the reference's `view_id2 == 0` rule — so every
frame is sampled once.  With --predflow_path the flows are the predictions under <data_root>/flow_preds/NAME and go to
<save_root>/flow_preds/NAME/<sequence>/.  The split file is copied to <save_root>/<split>.txt.
An empty frame is written as it is, as in the reference.  A frame with 0 < N < n_sample_point points is written WHOLE and
unsampled, named on stderr, counted and listed in <save_root>/short_frames.json: the reference's CUDA FPS repeats indices there
in an order its code does not pin, and such frames are the ones filter_empty keeps out of the frame lists.
`--synthetic N` first writes N synthetic sequences of four frames into --data_root and the split file
(ogc_amd/utils/synthetic.py::write_waymo_moving_root).
"""
import argparse
import json
import os
import shutil
import sys

import numpy as np
import torch

from ..datasets import WaymoOpenDataset
from ..utils.data_util import fps_downsample

LABELS = ("segm", "semantic_segm")


def sample_frame(arrays, n_sample_point):
    """arrays: the per-point arrays of one frame, the points first -> (the arrays gathered by the FPS indices of the points,
    whether the frame was short).  Empty and short frames come back as they are."""
    n_point = arrays[0].shape[0]
    if n_point < n_sample_point:
        return arrays, n_point > 0
    fps_idx = fps_downsample(arrays[0], n_sample_point=n_sample_point)
    return [a[fps_idx] for a in arrays], False


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--data_root", type=str, required=True, help="Root path for the dataset")
    ap.add_argument("--save_root", type=str, required=True, help="Path to save the downsampled dataset")
    ap.add_argument("--split_file", type=str, required=True, help="Text file with the sequences to process, one name per line")
    ap.add_argument("--predflow_path", type=str, default=None, help="Path to load pre-saved flow predictions")
    ap.add_argument("--n_sample_point", type=int, default=8192)
    ap.add_argument("--synthetic", type=int, default=0, help="write this many synthetic sequences into data_root first")
    ap.add_argument("--synthetic_points", type=int, default=0, help="points per synthetic frame (default: 2.5 x n_sample_point)")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("downsample_waymo needs a HIP device; ogc_amd has no CPU path")
    split, ext = os.path.splitext(os.path.basename(args.split_file))
    if args.synthetic > 0:
        from ..utils.synthetic import write_waymo_moving_root
        if os.path.dirname(os.path.abspath(args.split_file)) != os.path.abspath(args.data_root) or ext != ".txt":
            raise ValueError("--synthetic writes the split file as <data_root>/<name>.txt: name it so")
        write_waymo_moving_root(args.data_root, args.synthetic, 4, args.synthetic_points or args.n_sample_point * 5 // 2,
                                args.n_sample_point, split=split)
    save_dir = os.path.join(args.save_root, "data")
    os.makedirs(save_dir, exist_ok=True)
    flow_root = save_flow_root = None
    if args.predflow_path is not None:
        flow_root = os.path.join(args.data_root, "flow_preds", args.predflow_path)
        save_flow_root = os.path.join(args.save_root, "flow_preds", args.predflow_path)
        os.makedirs(save_flow_root, exist_ok=True)
    dataset = WaymoOpenDataset(data_root=args.data_root, mapping_path=args.split_file)      # only for the sample ids
    n_frames, short = 0, []

    def load(sequence_path, view_id):
        return [np.load(os.path.join(sequence_path, "%s_%04d.npy" % (what, view_id))) for what in ("pc",) + LABELS]

    def save(save_path, view_id, arrays):
        for what, value in zip(("pc",) + LABELS, arrays):
            np.save(os.path.join(save_path, "%s_%04d.npy" % (what, view_id)), value)

    for sequence_name, view_id1, view_id2 in dataset.data_ids:
        sequence_path = os.path.join(args.data_root, "data", sequence_name)
        flow_name = "flow_%04d_%04d.npy" % (view_id1, view_id2)
        flow = np.load(os.path.join(flow_root, sequence_name, flow_name) if flow_root else os.path.join(sequence_path, flow_name))
        save_path = os.path.join(save_dir, sequence_name)
        os.makedirs(save_path, exist_ok=True)
        frames = [(view_id1, load(sequence_path, view_id1) + [flow])]
        if view_id2 == 0:         # a later frame has been sampled as `view_id1` of the pair before
            frames.append((view_id2, load(sequence_path, view_id2)))
        for view_id, arrays in frames:
            n_point = arrays[0].shape[0]
            arrays, is_short = sample_frame(arrays, args.n_sample_point)
            if is_short:
                print("downsample_waymo: frame %s %d written whole, it has %d points, fewer than %d"
                      % (sequence_name, view_id, n_point, args.n_sample_point), file=sys.stderr)
                short.append([sequence_name, view_id, n_point])
            save(save_path, view_id, arrays[:3])
            n_frames += 1
            if view_id == view_id1:
                flow_dir = os.path.join(save_flow_root, sequence_name) if save_flow_root else save_path
                os.makedirs(flow_dir, exist_ok=True)
                np.save(os.path.join(flow_dir, flow_name), arrays[3])
    split_copy = os.path.join(args.save_root, split + ".txt")
    if os.path.abspath(split_copy) != os.path.abspath(args.split_file):
        shutil.copyfile(args.split_file, split_copy)
    with open(os.path.join(args.save_root, "short_frames.json"), "w") as f:
        json.dump(short, f)
    print("downsample_waymo: %d frames of %d pairs written to %s, %d short; split file %s"
          % (n_frames, len(dataset), save_dir, len(short), split_copy))
    return {"frames": n_frames, "pairs": len(dataset), "short": short, "split_file": split_copy}


if __name__ == "__main__":
    main()

"""Waymo preparation, the frame list of the supervised baseline (reference: data_prepare/waymo/filter_empty.py): the frames of a
split, every `sampled_interval`-th one, that hold at least n_sample_point points -> <split>_sup.json, what
WaymoSingleFrameDataset(select_frame=...) reads and select_mov turns into frame pairs.

    python -m ogc_amd.data_prepare.filter_empty --data_root <full root> --split_file F --out <split>_sup.json
                                                [--n_sample_point 8192] [--sampled_interval 5]

The ids are those of WaymoSingleFrameDataset over the full-resolution root.  A frame's number of points is read from the header of
its pc_%04d.npy; no array is loaded (the reference loads every frame through its reader for this one number).  Frames below the
count are printed as the reference prints them: sequence, frame, number of points.  Needs no device.
"""
import argparse
import json
import os

import numpy as np

from ..datasets import WaymoSingleFrameDataset


def frame_points(data_root, sequence_name, view_id):
    """The number of points of a frame from the .npy header alone."""
    return int(np.load(os.path.join(data_root, "data", sequence_name, "pc_%04d.npy" % view_id), mmap_mode="r").shape[0])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--data_root", type=str, required=True, help="Root path for the full-resolution dataset")
    ap.add_argument("--split_file", type=str, required=True, help="Text file with the sequences of the split, one name per line")
    ap.add_argument("--out", type=str, required=True, help="The json file to write, <split>_sup.json")
    ap.add_argument("--n_sample_point", type=int, default=8192)
    ap.add_argument("--sampled_interval", type=int, default=5)
    args = ap.parse_args(argv)
    dataset = WaymoSingleFrameDataset(data_root=args.data_root, mapping_path=args.split_file, downsampled=False,
                                      sampled_interval=args.sampled_interval)
    keep_samples, ignore_samples = [], []
    for sequence_name, view_id in dataset.data_ids:
        n_point = frame_points(args.data_root, sequence_name, view_id)
        if n_point < args.n_sample_point:
            print(sequence_name, view_id, n_point)
            ignore_samples.append((sequence_name, view_id))
        else:
            keep_samples.append((sequence_name, view_id))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(keep_samples, f)
    print("filter_empty: %d frames kept, %d below %d points; list %s" % (len(keep_samples), len(ignore_samples), args.n_sample_point, args.out))
    return {"kept": keep_samples, "ignored": ignore_samples, "out": args.out}


if __name__ == "__main__":
    main()

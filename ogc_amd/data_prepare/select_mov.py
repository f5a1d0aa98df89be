"""Waymo preparation, the frame-pair list of the unsupervised training (reference: data_prepare/waymo/select_mov.py): the frames
of <split>_sup.json as pairs (t, t - 1) -> <split>_sup_paired.json, and those pairs in which enough of the scene moves
-> <split>_unsup.json, what WaymoOpenDataset(downsampled=True, select_frame=...) reads.

    python -m ogc_amd.data_prepare.select_mov --data_root <downsampled root> --pose_root <full root> --split_file F
                                              --sup_frames <split>_sup.json --out_dir D [--predflow_path NAME]
                                              [--ignore_class_ids 2 3] [--ignore_npoint_thresh 50] [--moving_thresh 0.2]
                                              [--ratio_thresh 0.2] [--batch 64]

Per batch of pairs the first frame's files and the two pose_%04d.npy are read on the host, the relative motion rot2^T rot1,
rot2^T (t1 - t2) is computed in float64 and the flow cast to float32 as the reader casts it; then ONE upload, ONE launch
(ogc_moving_stats) and one copy of three integers per pair back.  A pair is selected iff the reader's filtered labels
of its first frame hold more than one value (n_distinct != 1), a point above y = 0.3 exists and np.float32(n_mov) / n_fg >
ratio_thresh: the reference's expression, evaluated on the host from the integers.  The selected pairs are written in data-set
order, and the two counts are printed as the reference prints them.
One deviation: a pair whose two frames differ in their number of points cannot be stacked by the reader with downsampled=True
(the reference's run would stop there).  Such a pair is dropped, named on stderr and counted.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

from ..datasets import WaymoOpenDataset
from .scan_ops import moving_counts

GROUND_Y = 0.3            # select_mov.py:91


def convert_id_to_pair(data_ids):
    """Single-frame ids (sequence, t) -> pair ids (sequence, t, t - 1) of the frames with t > 0 (select_mov.py:13-20)."""
    paired_data_ids = []
    for data_id in data_ids:
        sequence_name, view_id = data_id
        if view_id > 0:
            paired_data_ids.append((sequence_name, view_id, view_id - 1))
    return paired_data_ids


def relative_motion(pose1, pose2):
    """select_mov.py:85-88 -> (12,) float64: the row-major rotation rot2^T rot1, then the translation rot2^T (t1 - t2)."""
    rot1, transl1 = pose1[0:3, 0:3], pose1[0:3, 3]
    rot2, transl2 = pose2[0:3, 0:3], pose2[0:3, 3]
    rot = rot2.T @ rot1
    transl = rot2.T @ (transl1 - transl2)
    return np.concatenate([np.asarray(rot, dtype=np.float64).reshape(9), np.asarray(transl, dtype=np.float64)])


def is_selected(n_distinct, n_fg, n_mov, ratio_thresh):
    return bool(n_distinct != 1 and n_fg > 0 and np.float32(n_mov) / n_fg > ratio_thresh)


def batch_counts(dataset, pose_root, pairs, moving_thresh, device="cuda"):
    """The (n_distinct, n_fg, n_mov) rows of `pairs` (ids of `dataset`): host reads, one upload, one launch, one copy back."""
    pcs, flows, segms, semantics, motions, offsets = [], [], [], [], [], [0]
    for sequence_name, view_id1, view_id2 in pairs:
        d = os.path.join(dataset.data_root, sequence_name)
        pcs.append(np.load(os.path.join(d, "pc_%04d.npy" % view_id1)).astype(np.float32, copy=False))
        segms.append(np.load(os.path.join(d, "segm_%04d.npy" % view_id1)).astype(np.int32, copy=False))
        semantics.append(np.load(os.path.join(d, "semantic_segm_%04d.npy" % view_id1)).astype(np.int32, copy=False))
        load_flow = dataset._load_predflow if dataset.predflow_path is not None else dataset._load_flow
        flows.append(load_flow(sequence_name, view_id1, view_id2)[0].astype(np.float32, copy=False))
        pose_dir = os.path.join(pose_root, "data", sequence_name)
        motions.append(relative_motion(np.load(os.path.join(pose_dir, "pose_%04d.npy" % view_id1)),
                                       np.load(os.path.join(pose_dir, "pose_%04d.npy" % view_id2))))
        n = pcs[-1].shape[0]
        if not (flows[-1].shape == (n, 3) and segms[-1].shape == (n,) and semantics[-1].shape == (n,)):
            raise ValueError("frame %s %d: pc, flow and labels differ in their number of points" % (sequence_name, view_id1))
        offsets.append(offsets[-1] + n)

    def up(arrays, dtype, tail):
        return torch.from_numpy(np.ascontiguousarray(np.concatenate(arrays, 0).reshape((-1,) + tail), dtype=dtype)).to(device)
    try:
        return moving_counts(up(pcs, np.float32, (3,)), up(flows, np.float32, (3,)), up(segms, np.int32, ()), up(semantics, np.int32, ()),
                             torch.tensor(offsets, dtype=torch.int32, device=device), up(motions, np.float64, (12,)),
                             ignore_class_ids=dataset.ignore_class_ids, ignore_npoint_thresh=dataset.ignore_npoint_thresh,
                             ground_y=GROUND_Y, moving_thresh=moving_thresh)
    except ValueError as e:
        raise ValueError("%s (the batch starts at pair %s)" % (e, (pairs[0],))) from None


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--data_root", type=str, required=True, help="Root path of the downsampled dataset")
    ap.add_argument("--pose_root", type=str, required=True, help="Root path of the full-resolution dataset, which holds the poses")
    ap.add_argument("--split_file", type=str, required=True, help="Text file with the sequences of the split, one name per line")
    ap.add_argument("--sup_frames", type=str, required=True, help="<split>_sup.json, the frame list filter_empty wrote")
    ap.add_argument("--out_dir", type=str, required=True, help="Where <split>_sup_paired.json and <split>_unsup.json go")
    ap.add_argument("--predflow_path", type=str, default=None, help="Name of the predicted flows to judge the motion by")
    ap.add_argument("--ignore_class_ids", type=int, nargs="*", default=[2, 3], help="Pedestrian and Cyclist, as the reference")
    ap.add_argument("--ignore_npoint_thresh", type=int, default=50)
    ap.add_argument("--moving_thresh", type=float, default=0.2)
    ap.add_argument("--ratio_thresh", type=float, default=0.2)
    ap.add_argument("--batch", type=int, default=64, help="frame pairs per launch")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("select_mov needs a HIP device; ogc_amd has no CPU path")
    if args.batch < 1:
        raise ValueError("--batch must be at least 1")
    split = os.path.splitext(os.path.basename(args.split_file))[0]
    with open(args.sup_frames, "r") as f:
        data_ids = [(str(seq), int(t)) for seq, t in json.load(f)]
    os.makedirs(args.out_dir, exist_ok=True)
    paired = os.path.join(args.out_dir, "%s_sup_paired.json" % split)
    with open(paired, "w") as f:
        json.dump(convert_id_to_pair(data_ids), f)
    dataset = WaymoOpenDataset(data_root=args.data_root, mapping_path=args.split_file, downsampled=True, select_frame=paired,
                               predflow_path=args.predflow_path, ignore_class_ids=args.ignore_class_ids,
                               ignore_npoint_thresh=args.ignore_npoint_thresh)
    usable, dropped = [], []
    for sequence_name, view_id1, view_id2 in dataset.data_ids:
        n1, n2 = (int(np.load(os.path.join(dataset.data_root, sequence_name, "pc_%04d.npy" % v), mmap_mode="r").shape[0])
                  for v in (view_id1, view_id2))
        if n1 != n2:
            print("select_mov: pair %s %d %d dropped, its frames have %d and %d points" % (sequence_name, view_id1, view_id2, n1, n2),
                  file=sys.stderr)
            dropped.append((sequence_name, view_id1, view_id2))
        else:
            usable.append((sequence_name, view_id1, view_id2))
    moving_samples = []
    for start in range(0, len(usable), args.batch):
        pairs = usable[start:start + args.batch]
        counts = batch_counts(dataset, args.pose_root, pairs, args.moving_thresh)
        moving_samples += [pair for pair, row in zip(pairs, counts) if is_selected(int(row[0]), int(row[1]), int(row[2]), args.ratio_thresh)]
    print(len(dataset), len(moving_samples))
    save_file = os.path.join(args.out_dir, "%s_unsup.json" % split)
    with open(save_file, "w") as f:
        json.dump(moving_samples, f)
    if dropped:
        print("select_mov: %d pairs dropped, their frames differ in their number of points" % len(dropped), file=sys.stderr)
    return {"pairs": len(dataset), "moving": moving_samples, "dropped": dropped, "paired_file": paired, "unsup_file": save_file}


if __name__ == "__main__":
    main()

"""SemanticKITTI preparation (reference: data_prepare/semantickitti/process_semantickitti.py): raw sequences ->
downsampled/%02d_%06d/{pc,segm}.npy, what SemanticKITTIDataset reads.

    python -m ogc_amd.data_prepare.process_semantickitti <data_root> [--n_sample_point 8192] [--synthetic N]

Per frame one upload of the scan and its label words, then on the device: the camera crop without R0 at the fixed 1242 x 375
(ogc_scan_crop_camera), FPS on the cropped cloud, the labels gathered by keep_idx and then by the FPS indices; one download of
n_sample_point rows.  The class filter on the low 16 bits and the np.unique relabelling run on the host: they touch
n_sample_point integers.  Sequences 00 .. 10 are taken where they exist, the frames are the files labels/ holds.  A frame whose
crop leaves fewer than n_sample_point points is skipped, named on stderr and counted.
`--synthetic N` first writes one synthetic raw sequence of N frames into <data_root>
(ogc_amd/utils/synthetic.py::write_semantickitti_raw_root).
"""
import argparse
import os
import sys

import numpy as np
import torch

from . import kitti_io
from .process_kittidet import CLIP_DISTANCE, DEPTH_THRESH, sample_frame
from .scan_ops import crop_camera

IMG_WIDTH, IMG_HEIGHT = 1242, 375
SELECTED_CLASS_IDS = [10, 18, 252, 258]     # car, truck, moving-car, moving-truck
SEQUENCE_IDS = tuple(range(11))


def relabel(label):
    """The label words of the sampled points -> segm: instances of the selected classes keep their word, everything else is 0,
    then ranks (process_semantickitti.py:85-89)."""
    segm = np.zeros_like(label)
    keep = np.isin(label & 0xFFFF, SELECTED_CLASS_IDS)
    segm[keep] = label[keep]
    return np.unique(segm, return_inverse=True)[1].reshape(-1)


def prepare_frame(scan, label, calib, n_sample_point):
    """scan (N, 4) float32, label (N,) int32 numpy -> (pc (n_sample_point, 3) float32, segm (n_sample_point,) int64) numpy, or
    None when the crop leaves too few points."""
    pc, keep_idx = crop_camera(torch.from_numpy(scan).cuda(), calib, IMG_WIDTH, IMG_HEIGHT, CLIP_DISTANCE, DEPTH_THRESH)
    if pc.shape[0] < n_sample_point:
        return None
    fps_idx = sample_frame(pc, n_sample_point)
    label = torch.from_numpy(label).cuda()[keep_idx.long()][fps_idx]
    return pc[fps_idx].cpu().numpy(), relabel(label.cpu().numpy())


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("data_root", type=str, help="Root path for the dataset")
    ap.add_argument("--n_sample_point", type=int, default=8192)
    ap.add_argument("--synthetic", type=int, default=0, help="write a synthetic raw sequence of this many frames into data_root first")
    ap.add_argument("--synthetic_points", type=int, default=30000)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("process_semantickitti needs a HIP device; ogc_amd has no CPU path")
    if args.synthetic > 0:
        from ..utils.synthetic import write_semantickitti_raw_root
        write_semantickitti_raw_root(args.data_root, args.synthetic, args.synthetic_points)
    src = os.path.join(args.data_root, "sequences")
    save_dir = os.path.join(args.data_root, "downsampled")
    os.makedirs(save_dir, exist_ok=True)
    written = skipped = 0
    for seq_id in SEQUENCE_IDS:
        seq_dir = os.path.join(src, "%02d" % seq_id)
        if not os.path.isdir(seq_dir):
            continue
        calib = kitti_io.read_semantickitti_calib(os.path.join(seq_dir, "calib.txt"))
        print("Processing sequence %02d" % seq_id)
        for sid in range(len(os.listdir(os.path.join(seq_dir, "labels")))):
            scan = np.fromfile(os.path.join(seq_dir, "velodyne", "%06d.bin" % sid), dtype=np.float32).reshape(-1, 4)
            label = np.fromfile(os.path.join(seq_dir, "labels", "%06d.label" % sid), dtype=np.int32).reshape(-1)
            result = prepare_frame(scan, label, calib, args.n_sample_point)
            if result is None:
                print("process_semantickitti: frame %02d_%06d skipped, its crop leaves fewer than %d points"
                      % (seq_id, sid, args.n_sample_point), file=sys.stderr)
                skipped += 1
                continue
            save_path = os.path.join(save_dir, "%02d_%06d" % (seq_id, sid))
            os.makedirs(save_path, exist_ok=True)
            np.save(os.path.join(save_path, "pc.npy"), result[0])
            np.save(os.path.join(save_path, "segm.npy"), result[1])
            written += 1
    print("process_semantickitti: %d frames written to %s, %d skipped" % (written, save_dir, skipped))
    return {"frames": written, "skipped": skipped}


if __name__ == "__main__":
    main()

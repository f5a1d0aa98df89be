"""KITTI-Det preparation (reference: data_prepare/kittidet/process_kittidet.py): raw frames -> downsampled/%06d/{pc,segm}.npy,
what KITTIDetectionDataset reads.

    python -m ogc_amd.data_prepare.process_kittidet <data_root> [--n_sample_point 8192] [--synthetic N]

Per frame one upload of the scan, then on the device: the camera crop (ogc_scan_crop_camera), FPS (ogc_furthest_point_sampling)
on the cropped cloud, the labels of the sampled points from the `Car` boxes (ogc_box_segm); one download of n_sample_point rows.
The frames are the scans velodyne/ holds (the reference hard-codes 7481).  A frame whose crop leaves fewer than n_sample_point
points is skipped, named on stderr and counted: the reference's FPS would repeat indices there.
`--synthetic N` first writes N synthetic raw frames into <data_root> (ogc_amd/utils/synthetic.py::write_kittidet_raw_root).
"""
import argparse
import os
import sys

import numpy as np
import torch

from ..pointnet2.pointnet2 import furthest_point_sample
from . import kitti_io
from .scan_ops import box_segm, crop_camera

CLIP_DISTANCE, DEPTH_THRESH = 2.0, 35.0


def sample_frame(pc, n_sample_point):
    """FPS indices (n_sample_point,) int64 into a cropped cloud pc (M, 3) on the device."""
    return furthest_point_sample(pc[None].contiguous(), n_sample_point)[0].long()


def prepare_frame(scan, calib, width, height, objects, n_sample_point):
    """scan (N, 4) float32 numpy -> (pc (n_sample_point, 3) float32, segm (n_sample_point,) int32) numpy, or None when the crop
    leaves too few points."""
    pc, _ = crop_camera(torch.from_numpy(scan).cuda(), calib, width, height, CLIP_DISTANCE, DEPTH_THRESH)
    if pc.shape[0] < n_sample_point:
        return None
    pc = pc[sample_frame(pc, n_sample_point)]
    boxes, ids = kitti_io.kittidet_boxes(objects)
    segm, _ = box_segm(pc, torch.from_numpy(boxes).cuda(), torch.from_numpy(ids).cuda(), sign=kitti_io.KITTIDET_SIGN)
    return pc.cpu().numpy(), segm.cpu().numpy()


def frame_ids(lidar_root):
    return sorted(int(os.path.splitext(f)[0]) for f in os.listdir(lidar_root) if f.endswith(".bin"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("data_root", type=str, help="Root path for the dataset")
    ap.add_argument("--n_sample_point", type=int, default=8192)
    ap.add_argument("--synthetic", type=int, default=0, help="write this many synthetic raw frames into data_root first")
    ap.add_argument("--synthetic_points", type=int, default=30000)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("process_kittidet needs a HIP device; ogc_amd has no CPU path")
    if args.synthetic > 0:
        from ..utils.synthetic import write_kittidet_raw_root
        write_kittidet_raw_root(args.data_root, args.synthetic, args.synthetic_points)
    src = os.path.join(args.data_root, "training")
    save_dir = os.path.join(args.data_root, "downsampled")
    os.makedirs(save_dir, exist_ok=True)
    ids = frame_ids(os.path.join(src, "velodyne"))
    skipped = 0
    for sid in ids:
        scan = np.fromfile(os.path.join(src, "velodyne", "%06d.bin" % sid), dtype=np.float32).reshape(-1, 4)
        calib = kitti_io.read_kittidet_calib(os.path.join(src, "calib", "%06d.txt" % sid))
        width, height = kitti_io.image_size(os.path.join(src, "image_2", "%06d.png" % sid))
        objects = kitti_io.read_label(os.path.join(src, "label_2", "%06d.txt" % sid))
        result = prepare_frame(scan, calib, width, height, objects, args.n_sample_point)
        if result is None:
            print("process_kittidet: frame %06d skipped, its crop leaves fewer than %d points" % (sid, args.n_sample_point),
                  file=sys.stderr)
            skipped += 1
            continue
        save_path = os.path.join(save_dir, "%06d" % sid)
        os.makedirs(save_path, exist_ok=True)
        np.save(os.path.join(save_path, "pc.npy"), result[0])
        np.save(os.path.join(save_path, "segm.npy"), result[1])
    print("process_kittidet: %d frames written to %s, %d skipped" % (len(ids) - skipped, save_dir, skipped))
    return {"frames": len(ids) - skipped, "skipped": skipped}


if __name__ == "__main__":
    main()

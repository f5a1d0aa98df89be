"""Waymo preparation (reference: data_prepare/waymo/process_waymo.py, WaymoDataset.process_sequence): info files, raw scans and
velocities -> <save_root>/data/<sequence>/{pc,segm,semantic_segm,pose}_%04d.npy and flow_%04d_%04d.npy, what WaymoOpenDataset
and WaymoSingleFrameDataset read.

    python -m ogc_amd.data_prepare.process_waymo --data_root R --save_root S --split_file F [--cfg_file config/waymo_prepare.yaml]
                                                 [--n_sample_point 8192] [--synthetic N]

Per frame one upload of the (N, 6) scan, then on the device: the front crop (ogc_scan_crop_front), the velocities gathered by
keep_idx and turned into the backward scene flow in fp64 with the UN-permuted poses (process_flow, the reference's sign), the
labels of the cropped points from the boxes (ogc_box_segm), and last the axis permutation (x, y, z) -> (y, z, x) of points,
flows and poses; one download of the cropped frame.  The boxes are filtered on the host as the reference filters them — `unknown`
dropped, then with FILTER_EMPTY_BOXES the boxes without points and the classes outside Vehicle / Pedestrian / Cyclist — and
tracking ids become integers in the order they first appear in the sequence.  Files, names and dtypes are the reference's: pc
float32, flow and pose float64, labels int32.  --n_sample_point is accepted for symmetry with the camera drivers; this stage
keeps the cropped frame whole (the sampling is downsample_waymo's).
`--synthetic N` first writes N synthetic raw sequences of three frames into --data_root and the split file
(ogc_amd/utils/synthetic.py::write_waymo_raw_root).
"""
import argparse
import os
import pickle

import numpy as np
import torch
import yaml

from . import kitti_io
from .scan_ops import box_segm, crop_front

CLASS_NAMES = ["Vehicle", "Pedestrian", "Cyclist"]
PERM = np.array([[0, 1, 0], [0, 0, 1], [1, 0, 0]], dtype=np.float32)      # (x, y, z) -> (y, z, x)
AXIS_ORDER = [1, 2, 0]                                                    # PERM applied to rows of points: columns y, z, x
DEFAULT_CFG = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "config", "waymo_prepare.yaml")


def process_flow(velocity, pc2, pose1, pose2):
    """process_waymo.py:29-45 on the device in float64: velocity (N, 3) m/s and pc2 (N, 3) of the current frame, pose1 the
    previous and pose2 the current sensor-to-world pose (4, 4) float64 -> pc2 - (pc2 - 0.1 velocity seen from the previous frame)."""
    flow = velocity * 0.1                                     # fp32, as the reference's first line
    pose1 = torch.as_tensor(pose1, dtype=torch.float64, device=pc2.device)
    pose2 = torch.as_tensor(pose2, dtype=torch.float64, device=pc2.device)
    rot1, transl1 = pose1[0:3, 0:3], pose1[0:3, 3]
    rot2, transl2 = pose2[0:3, 0:3], pose2[0:3, 3]
    inv_rot2 = torch.linalg.inv(rot2)
    pc2 = pc2.double()
    return pc2 - ((pc2 - flow.double()) @ inv_rot2 + transl2 - transl1) @ rot1


def filter_annos(annos, filter_empty):
    """(gt_boxes (K, 7), class names, tracking ids) of a frame after the reference's filters (process_waymo.py:156-166)."""
    keep = [i for i, x in enumerate(annos["name"]) if x != "unknown"]
    boxes, names, trackings = annos["gt_boxes_lidar"][keep], annos["name"][keep], annos["obj_ids"][keep]
    if filter_empty:
        mask = annos["num_points_in_gt"][keep] > 0
        boxes, names, trackings = boxes[mask], names[mask], trackings[mask]
        selected = np.array([i for i, x in enumerate(names) if x in CLASS_NAMES], dtype=np.int64)
        boxes, names, trackings = boxes[selected], names[selected], trackings[selected]
    return boxes, names, trackings


def permute_pose(pose):
    out = np.array(pose, copy=True)
    out[0:3, 0:3], out[0:3, 3] = PERM @ pose[0:3, 0:3] @ PERM.T, PERM @ pose[0:3, 3]
    return out


def process_sequence(infos, data_path, flow_path, save_path, cfg):
    """One sequence: `infos` the list of frame infos of its .pkl.  Returns the number of frames written."""
    os.makedirs(save_path, exist_ok=True)
    tracking_to_idx, prev_pose = {}, None
    for t, info in enumerate(infos):
        sequence_name, sample_idx = info["point_cloud"]["lidar_sequence"], info["point_cloud"]["sample_idx"]
        scan = torch.from_numpy(np.load(os.path.join(data_path, sequence_name, "%04d.npy" % sample_idx)).astype(np.float32, copy=False)).cuda()
        pc, keep_idx = crop_front(scan.contiguous())
        pose = np.asarray(info["pose"], dtype=np.float64)
        flow = None
        if t > 0:
            velocity = torch.from_numpy(np.load(os.path.join(flow_path, sequence_name, "%04d.npy" % sample_idx))[:, :3]).cuda()
            flow = -process_flow(velocity[keep_idx.long()], pc, prev_pose, pose)
        prev_pose = pose.copy()

        gt_boxes, names, trackings = filter_annos(info["annos"], cfg.get("FILTER_EMPTY_BOXES", False))
        for tracking in trackings:
            if tracking not in tracking_to_idx:
                tracking_to_idx[tracking] = len(tracking_to_idx) + 1
        object_ids = np.array([tracking_to_idx[tracking] for tracking in trackings], dtype=np.int32)
        class_ids = np.array([CLASS_NAMES.index(name) + 1 for name in names], dtype=np.int32)
        boxes, ids = kitti_io.waymo_boxes(gt_boxes, object_ids, class_ids)
        segm, semantic_segm = box_segm(pc, torch.from_numpy(boxes).cuda(), torch.from_numpy(ids).cuda())

        pc = pc[:, AXIS_ORDER]
        np.save(os.path.join(save_path, "pose_%04d.npy" % sample_idx), permute_pose(pose))
        np.save(os.path.join(save_path, "pc_%04d.npy" % sample_idx), pc.cpu().numpy())
        np.save(os.path.join(save_path, "segm_%04d.npy" % sample_idx), segm.cpu().numpy())
        np.save(os.path.join(save_path, "semantic_segm_%04d.npy" % sample_idx), semantic_segm.cpu().numpy())
        if flow is not None:
            flow = flow[:, AXIS_ORDER]
            np.save(os.path.join(save_path, "flow_%04d_%04d.npy" % (sample_idx, sample_idx - 1)), flow.cpu().numpy())
    return len(infos)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--data_root", type=str, required=True, help="Root path for the dataset")
    ap.add_argument("--save_root", type=str, required=True, help="Save path for the processed dataset")
    ap.add_argument("--split_file", type=str, required=True, help="Text file with the sequences to process, one name per line")
    ap.add_argument("--cfg_file", type=str, default=DEFAULT_CFG)
    ap.add_argument("--n_sample_point", type=int, default=8192)
    ap.add_argument("--synthetic", type=int, default=0, help="write this many synthetic raw sequences into data_root first")
    ap.add_argument("--synthetic_points", type=int, default=30000)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("process_waymo needs a HIP device; ogc_amd has no CPU path")
    with open(args.cfg_file) as f:
        cfg = yaml.safe_load(f)
    if args.synthetic > 0:
        from ..utils.synthetic import write_waymo_raw_root
        split, ext = os.path.splitext(os.path.basename(args.split_file))
        if os.path.dirname(os.path.abspath(args.split_file)) != os.path.abspath(args.data_root) or ext != ".txt":
            raise ValueError("--synthetic writes the split file as <data_root>/<name>.txt: name it so")
        write_waymo_raw_root(args.data_root, args.synthetic, 3, args.synthetic_points, data_tag=cfg["PROCESSED_DATA_TAG"],
                             flow_tag=cfg["SCENE_FLOW_TAG"], split=split)
    data_path = os.path.join(args.data_root, cfg["PROCESSED_DATA_TAG"])
    flow_path = os.path.join(args.data_root, cfg["SCENE_FLOW_TAG"])
    with open(args.split_file) as f:
        sequences = [os.path.splitext(line.strip())[0] for line in f if line.strip()]
    save_root = os.path.join(args.save_root, "data")
    print("Processing Waymo dataset... Save into %s" % save_root)
    os.makedirs(save_root, exist_ok=True)
    n_frames = n_skipped = 0
    for k, sequence_name in enumerate(sequences):
        info_path = os.path.join(data_path, sequence_name, sequence_name + ".pkl")
        if not os.path.exists(info_path):
            n_skipped += 1
            continue
        with open(info_path, "rb") as f:
            infos = pickle.load(f)
        print("---%d/%d %s" % (k, len(sequences), sequence_name))
        n_frames += process_sequence(infos, data_path, flow_path, os.path.join(save_root, sequence_name), cfg)
    print("Processing finished. %d frames written. Total skipped (unavailable) sequences %d" % (n_frames, n_skipped))
    return {"frames": n_frames, "skipped_sequences": n_skipped}


if __name__ == "__main__":
    main()

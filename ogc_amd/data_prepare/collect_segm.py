"""OGC-DR preparation, the single-view set (reference: data_prepare/ogcdrsv/collect_segm.py): the single-view clouds
<dest_root>/pcd/<id>/pc_%02d.pcd and the complete clouds of <src_root>/data/<id>/ -> <dest_root>/data/<id>/{pc,segm,pose}_%02d.npy.

    python -m ogc_amd.data_prepare.collect_segm --src_root <OGC-DR root> --dest_root <OGC-DRSV root> [--n_sample_point 2048]

Per scene the four .pcd files are read on the host (mesh_io.read_pcd: ascii or binary, float32 x y z), sampled down to
n_sample_point points by furthest point sampling on the device, and every point takes the label of its nearest neighbour in the
complete cloud of its frame — `segm_src[cdist(pc, pc_src).argmin(1)]` in the reference, mesh_ops.nearest_label here:
one call for the frames of a scene whose complete clouds have the same size, which is all four of them in a root that
sample_pointcloud wrote.  segm keeps the dtype of the complete cloud's labels; pose is copied.  At the end the three split files
are copied from <src_root>/data.  A .pcd with fewer points than n_sample_point is an error that names it.
"""
import argparse
import os
import shutil

import numpy as np
import torch

from ..pointnet2.pointnet2 import furthest_point_sample
from .mesh_io import read_pcd
from .mesh_ops import nearest_label

N_FRAME = 4
SPLITS = ("train", "val", "test")


def collect_scene(data_path, src_path, n_sample_point, device="cuda"):
    """-> [(pc (n_sample_point, 3) float32, segm (n_sample_point,) of the source's dtype)] per frame, numpy."""
    pcs, sources, labels = [], [], []
    for frame_id in range(N_FRAME):
        pcd_file = os.path.join(data_path, "pc_%02d.pcd" % frame_id)
        pc = read_pcd(pcd_file)
        if pc.shape[0] < n_sample_point:
            raise ValueError("%s holds %d points, fewer than the %d to sample" % (pcd_file, pc.shape[0], n_sample_point))
        pc = torch.from_numpy(pc).to(device)
        fps_idx = furthest_point_sample(pc.unsqueeze(0).contiguous(), n_sample_point)[0].long()
        pcs.append(pc[fps_idx])
        sources.append(np.load(os.path.join(src_path, "pc_%02d.npy" % frame_id)).astype(np.float32, copy=False))
        labels.append(np.load(os.path.join(src_path, "segm_%02d.npy" % frame_id)))
        if sources[-1].ndim != 2 or sources[-1].shape[1] != 3 or labels[-1].shape != (sources[-1].shape[0],) or sources[-1].shape[0] < 1:
            raise ValueError("%s: pc_%02d.npy and segm_%02d.npy must be (N, 3) and (N,) with N >= 1" % (src_path, frame_id, frame_id))
    out = [None] * N_FRAME
    for size in sorted({s.shape[0] for s in sources}):      # one call for the frames that share a source size
        frames = [t for t in range(N_FRAME) if sources[t].shape[0] == size]
        segm, _ = nearest_label(torch.stack([pcs[t] for t in frames]).contiguous(),
                                torch.from_numpy(np.stack([sources[t] for t in frames])).to(device),
                                torch.from_numpy(np.stack([labels[t].astype(np.int32) for t in frames])).to(device))
        segm = segm.cpu().numpy()
        for row, t in enumerate(frames):
            out[t] = (pcs[t].cpu().numpy(), segm[row].astype(labels[t].dtype))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--src_root", type=str, required=True, help="Root path for the OGC-DR dataset")
    ap.add_argument("--dest_root", type=str, required=True, help="Root path for the OGC-DRSV dataset")
    ap.add_argument("--n_sample_point", type=int, default=2048)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("collect_segm needs a HIP device; ogc_amd has no CPU path")
    if args.n_sample_point < 1:
        raise ValueError("--n_sample_point must be at least 1")
    src_root, data_root = os.path.join(args.src_root, "data"), os.path.join(args.dest_root, "pcd")
    save_root = os.path.join(args.dest_root, "data")
    os.makedirs(save_root, exist_ok=True)
    data_ids = sorted(os.listdir(data_root))
    for data_id in data_ids:
        src_path, save_path = os.path.join(src_root, data_id), os.path.join(save_root, data_id)
        os.makedirs(save_path, exist_ok=True)
        for frame_id, (pc, segm) in enumerate(collect_scene(os.path.join(data_root, data_id), src_path, args.n_sample_point)):
            np.save(os.path.join(save_path, "pc_%02d.npy" % frame_id), pc)
            np.save(os.path.join(save_path, "segm_%02d.npy" % frame_id), segm)
            shutil.copyfile(os.path.join(src_path, "pose_%02d.npy" % frame_id), os.path.join(save_path, "pose_%02d.npy" % frame_id))
    for split in SPLITS:
        shutil.copyfile(os.path.join(src_root, split + ".lst"), os.path.join(save_root, split + ".lst"))
    print("collect_segm: %d scenes of %d frames written to %s" % (len(data_ids), N_FRAME, save_root))
    return {"scenes": data_ids, "save_root": save_root}


if __name__ == "__main__":
    main()

"""KITTI Scene Flow preparation, stage 1 (reference: data_prepare/kittisf/process_kittisf.py): the download's disparity,
optical-flow and instance maps -> processed/%06d/{pc1,pc2,segm}.npy, what KITTISceneFlowDataset(downsampled=False) and
downsample_kittisf read.

    python -m ogc_amd.data_prepare.process_kittisf <data_root> [--synthetic N]

Per frame the four 16-bit PNGs (training/disp_occ_0, disp_occ_1, flow_occ, instance; %06d_10.png) are decoded on the host
(png16.read_png), uploaded, and one call of scan_ops.kittisf_unproject (ogc_kittisf_unproject) gives the two clouds in
correspondence and the labels of the `Car` and `Truck` instances; one download of the kept rows.  P_rect_02 comes from
training/calib_cam_to_cam/%06d.txt.  The frames are those disp_occ_0 holds (the reference hard-codes 200).
`--synthetic N` first writes N synthetic raw frames into <data_root> (ogc_amd/utils/synthetic.py::write_kittisf_raw_root).
"""
import argparse
import os

import numpy as np
import torch

from ..pointnet2_cuda import U16
from . import kitti_io
from .png16 import read_png
from .scan_ops import KITTISF_SELECT_SEMANTICS, kittisf_unproject

DEPTH_THRESH = 35.0
MAPS = (("disp_occ_0", 2), ("disp_occ_1", 2), ("flow_occ", 3), ("instance", 2))    # directory, dimensions of the decoded array


def upload(array):
    """A uint16 numpy array as a device tensor of the library's 16-bit dtype (the same bits)."""
    return torch.from_numpy(array.view(np.int16)).cuda().view(U16)


def read_frame(src, sid):
    """The four maps of frame `sid` as uint16 numpy arrays, and P_rect_02 (3, 4) float32."""
    maps = []
    for sub, ndim in MAPS:
        path = os.path.join(src, sub, "%06d_10.png" % sid)
        array = read_png(path)
        if array.dtype != np.uint16 or array.ndim != ndim:
            raise ValueError("%s: expected a 16-bit %s image, got %s %s" % (path, "RGB" if ndim == 3 else "grey", array.dtype, array.shape))
        maps.append(array)
    return maps, kitti_io.read_kittisf_calib(os.path.join(src, "calib_cam_to_cam", "%06d.txt" % sid))


def prepare_frame(maps, P_rect):
    """(disp1, disp2, flow, inst) uint16 numpy, P_rect -> (pc1 (M, 3) float32, pc2 (M, 3) float32, segm (M,) int64) numpy; int64
    is what the reference's `astype(int)` leaves in segm.npy."""
    pc1, pc2, segm, _ = kittisf_unproject(*(upload(m) for m in maps), P_rect, KITTISF_SELECT_SEMANTICS, DEPTH_THRESH)
    return pc1.cpu().numpy(), pc2.cpu().numpy(), segm.cpu().numpy().astype(np.int64)


def frame_ids(disp_root):
    return sorted(int(f[:-len("_10.png")]) for f in os.listdir(disp_root) if f.endswith("_10.png"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("data_root", type=str, help="Root path for the dataset")
    ap.add_argument("--synthetic", type=int, default=0, help="write this many synthetic raw frames into data_root first")
    ap.add_argument("--synthetic_height", type=int, default=48)
    ap.add_argument("--synthetic_width", type=int, default=160)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("process_kittisf needs a HIP device; ogc_amd has no CPU path")
    if args.synthetic > 0:
        from ..utils.synthetic import write_kittisf_raw_root
        write_kittisf_raw_root(args.data_root, args.synthetic, args.synthetic_height, args.synthetic_width)
    src = os.path.join(args.data_root, "training")
    save_dir = os.path.join(args.data_root, "processed")
    os.makedirs(save_dir, exist_ok=True)
    ids = frame_ids(os.path.join(src, "disp_occ_0"))
    points = 0
    for sid in ids:
        maps, P_rect = read_frame(src, sid)
        pc1, pc2, segm = prepare_frame(maps, P_rect)
        save_path = os.path.join(save_dir, "%06d" % sid)
        os.makedirs(save_path, exist_ok=True)
        np.save(os.path.join(save_path, "pc1.npy"), pc1)
        np.save(os.path.join(save_path, "pc2.npy"), pc2)
        np.save(os.path.join(save_path, "segm.npy"), segm)
        points += pc1.shape[0]
    print("process_kittisf: %d frames written to %s, %d points in all" % (len(ids), save_dir, points))
    return {"frames": len(ids), "points": points}


if __name__ == "__main__":
    main()

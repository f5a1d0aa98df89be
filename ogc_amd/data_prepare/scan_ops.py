"""The device operators of data preparation (csrc/scan_prepare.hip).  Inputs are CUDA tensors, results stay on the
device; the only host read is the number of kept points of a crop.  There is no CPU path."""
import numpy as np
import torch

from .. import pointnet2_cuda as _native
from ..pointnet2_cuda import BOX_SEGM_BOX_DOUBLES, BOX_SEGM_CHUNK, SCAN_CROP_CAMERA_DOUBLES, SCAN_CROP_TILE  # noqa: F401


def _check_scan(scan, min_columns):
    if not isinstance(scan, torch.Tensor):
        raise TypeError("scan must be a torch.Tensor")
    if scan.dtype != torch.float32:
        raise TypeError("scan must be float32, got %s" % scan.dtype)
    if scan.device.type != "cuda":
        raise RuntimeError("scan must be a CUDA tensor (HIP device); ogc_amd has no CPU path")
    if scan.dim() != 2 or scan.shape[1] < min_columns:
        raise ValueError("scan must be (N, >= %d), got %s" % (min_columns, tuple(scan.shape)))
    if not scan.is_contiguous():
        raise RuntimeError("scan must be contiguous")


def camera_block(calib, width, height):
    """The fp64 parameter block of ogc_scan_crop_camera (include/ogc_ops.h) from a calibration dict {"V2C" (3, 4), "P" (3, 4),
    optionally "R0" (3, 3)} (kitti_io.read_kittidet_calib / read_semantickitti_calib): numpy (36,) float64."""
    block = np.zeros(SCAN_CROP_CAMERA_DOUBLES, dtype=np.float64)
    block[0:12] = np.asarray(calib["V2C"], dtype=np.float64).reshape(12)
    r0 = calib.get("R0")
    if r0 is not None:
        block[12:21] = np.asarray(r0, dtype=np.float64).reshape(9)
        block[35] = 1.0
    block[21:33] = np.asarray(calib["P"], dtype=np.float64).reshape(12)
    block[33], block[34] = float(width), float(height)
    return block


def _alloc(scan):
    n = scan.shape[0]
    out_pc = torch.empty(n, 3, dtype=torch.float32, device=scan.device)
    keep_idx = torch.empty(n, dtype=torch.int32, device=scan.device)
    count = torch.empty(1, dtype=torch.int32, device=scan.device)
    return n, out_pc, keep_idx, count


def crop_camera(scan, calib, width, height, clip_distance=2.0, depth_thresh=35.0):
    """The front-view cloud of a KITTI scan (process_kittidet.py:99-114; without calib["R0"] process_semantickitti.py:61-78):
    scan (N, >= 3) fp32 CUDA tensor -> (pc (M, 3) fp32 in the flipped camera frame, keep_idx (M,) int32 rows of the scan), both
    on the device, in scan order."""
    _check_scan(scan, 3)
    n, out_pc, keep_idx, count = _alloc(scan)
    cam = torch.from_numpy(camera_block(calib, width, height)).to(scan.device)
    _native.scan_crop_camera_wrapper(n, scan.shape[1], scan, cam, clip_distance, depth_thresh, out_pc, keep_idx, count)
    m = int(count.item())
    return out_pc[:m], keep_idx[:m]


def crop_front(scan):
    """The front-view cloud of a Waymo scan (process_waymo.py:132-141): scan (N, >= 6) fp32 CUDA tensor [x, y, z, intensity,
    elongation, NLZ flag] -> (pc (M, 3) fp32, keep_idx (M,) int32), on the device, in scan order."""
    _check_scan(scan, 6)
    n, out_pc, keep_idx, count = _alloc(scan)
    _native.scan_crop_front_wrapper(n, scan.shape[1], scan, out_pc, keep_idx, count)
    m = int(count.item())
    return out_pc[:m], keep_idx[:m]


def box_segm(pc, boxes, ids, sign=(1, 1, 1)):
    """Labels from oriented boxes, the last box wins: pc (N, 3) fp32, boxes (K, 18) fp64 rows [rot | centre | lo | hi], ids (K, 2)
    int32 [object id, class id], CUDA tensors; sign three values in {1, -1} applied to the point first
    -> (segm (N,), semantic_segm (N,)) int32 on the device."""
    for t, name, dtype in ((pc, "pc", torch.float32), (boxes, "boxes", torch.float64), (ids, "ids", torch.int32)):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor" % name)
        if t.dtype != dtype:
            raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
        if t.device.type != "cuda":
            raise RuntimeError("%s must be a CUDA tensor (HIP device); ogc_amd has no CPU path" % name)
    if pc.dim() != 2 or pc.shape[1] != 3:
        raise ValueError("pc must be (N, 3), got %s" % (tuple(pc.shape),))
    if boxes.dim() != 2 or boxes.shape[1] != BOX_SEGM_BOX_DOUBLES:
        raise ValueError("boxes must be (K, %d), got %s" % (BOX_SEGM_BOX_DOUBLES, tuple(boxes.shape)))
    if ids.dim() != 2 or ids.shape[1] != 2 or ids.shape[0] != boxes.shape[0]:
        raise ValueError("ids must be (K, 2) with K = %d, got %s" % (boxes.shape[0], tuple(ids.shape)))
    sign = tuple(int(s) for s in sign)
    if len(sign) != 3 or any(s not in (1, -1) for s in sign):
        raise ValueError("sign must be three values in {1, -1}, got %r" % (sign,))
    n = pc.shape[0]
    segm = torch.empty(n, dtype=torch.int32, device=pc.device)
    semantic_segm = torch.empty(n, dtype=torch.int32, device=pc.device)
    _native.box_segm_wrapper(n, boxes.shape[0], pc.contiguous(), sign, boxes.contiguous(), ids.contiguous(), segm, semantic_segm)
    return segm, semantic_segm

"""The device operators of data preparation (csrc/scan_prepare.hip; csrc/kittisf_prepare.hip, DESIGN §4k;
csrc/moving_stats.hip).  Inputs are CUDA tensors, results stay on the device; the only host reads are the number of
kept points of a crop and moving_counts' copy of its integers.  There is no CPU path."""
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


KITTISF_SELECT_SEMANTICS = (26, 28)     # `Car` and `Truck`, the categories process_kittisf.py keeps


def _check_maps(maps):
    """maps: (tensor, name, shape) of the 16-bit maps of one frame.  Types first, so that a wrong dtype is a TypeError whichever
    map has it and wherever the tensors live."""
    for t, name, _ in maps:
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor" % name)
        if t.dtype != _native.U16:
            raise TypeError("%s must be %s, got %s" % (name, _native.U16, t.dtype))
    for t, name, shape in maps:
        if t.device.type != "cuda":
            raise RuntimeError("%s must be a CUDA tensor (HIP device); ogc_amd has no CPU path" % name)
        if tuple(t.shape) != shape:
            raise ValueError("%s must be %s, got %s" % (name, shape, tuple(t.shape)))
        if not t.is_contiguous():
            raise RuntimeError("%s must be contiguous" % name)


def kittisf_unproject(disp1, disp2, flow, inst, P_rect, select_semantics=KITTISF_SELECT_SEMANTICS, depth_thresh=35.0):
    """The two clouds of a KITTI Scene Flow frame (process_kittisf.py:43-87): disp1, disp2, inst (H, W) and flow (H, W, 3), the
    16-bit samples of the four PNGs as CUDA tensors (torch.uint16; int16 views of the same bits where torch has none), P_rect the
    (3, 4) float32 numpy array of P_rect_02 -> (pc1 (M, 3) fp32, pc2 (M, 3) fp32, segm (M,) int32, keep_idx (M,) int32 = row *
    W + column), on the device, in pixel order.  segm numbers the instance ids present among the kept pixels whose semantic
    (id >> 8) is in select_semantics 1, 2, ... in ascending order; everything else is 0 (kittisf_util.py:72-81)."""
    if not isinstance(disp1, torch.Tensor):
        raise TypeError("disp1 must be a torch.Tensor")
    if disp1.dim() != 2:
        raise ValueError("disp1 must be (H, W), got %s" % (tuple(disp1.shape),))
    height, width = disp1.shape
    _check_maps(((disp1, "disp1", (height, width)), (disp2, "disp2", (height, width)), (flow, "flow", (height, width, 3)),
                 (inst, "inst", (height, width))))
    P = np.asarray(P_rect)
    if P.dtype != np.float32 or P.shape != (3, 4):
        raise ValueError("P_rect must be a (3, 4) float32 array, got %s %s" % (P.dtype, P.shape))
    if not (P[0, 1] == 0 and P[1, 0] == 0 and P[2, 0] == 0 and P[2, 1] == 0 and P[0, 0] == P[1, 1]):   # kittisf_util.py:7-11
        raise ValueError("P_rect must have P[0,1] = P[1,0] = P[2,0] = P[2,1] = 0 and P[0,0] = P[1,1]")
    select = [int(s) for s in select_semantics]
    if len(select) > 256:
        raise ValueError("select_semantics holds %d values, at most 256" % len(select))
    focal = P[0, 0]
    fb = np.float32(focal * 0.54)               # FOCAL_LENGTH_PIXEL * BASELINE as the reference writes it (kittisf_util.py:60-61)
    n = height * width
    dev = disp1.device
    pc1 = torch.empty(n, 3, dtype=torch.float32, device=dev)
    pc2 = torch.empty(n, 3, dtype=torch.float32, device=dev)
    segm = torch.empty(n, dtype=torch.int32, device=dev)
    keep_idx = torch.empty(n, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    sel = torch.tensor(select + [0] * (1 if not select else 0), dtype=torch.int32, device=dev)
    _native.kittisf_unproject_wrapper(height, width, disp1, disp2, flow, inst, fb, focal, P[0, 2], P[0, 3], P[1, 2], P[1, 3], P[2, 3],
                                      depth_thresh, sel, len(select), pc1, pc2, segm, keep_idx, count)
    m = int(count.item())
    return pc1[:m], pc2[:m], segm[:m], keep_idx[:m]


MOVING_STATS_LABEL_CAP = _native.MOVING_STATS_LABEL_CAP


def moving_stats(pc, flow, segm, semantic_segm, offsets, motion, ignore_class_ids=(), ignore_npoint_thresh=0, ground_y=0.3,
                 moving_thresh=0.2):
    """What the selection of moving Waymo samples needs of a ragged batch of B frame pairs (select_mov.py:74-96 with the reader's
    filter_segm, dataset_waymo.py:110-128), in one launch: the first frames' raw arrays concatenated along points — pc, flow
    (total, 3) fp32, segm, semantic_segm (total,) int32 —, offsets (B + 1,) int32 delimiting the samples and motion (B, 12) fp64 (the
    row-major rotation, then the translation of the relative sensor motion), CUDA tensors; ignore_class_ids a sequence of ints
    -> stats (B, 4) int32 on the device: the number of distinct filtered labels, the points with y >= ground_y, those of them whose
    flow differs from the rigid flow by more than moving_thresh, and a status (include/ogc_ops.h: ogc_moving_stats)."""
    tensors = ((pc, "pc", torch.float32), (flow, "flow", torch.float32), (segm, "segm", torch.int32),
               (semantic_segm, "semantic_segm", torch.int32), (offsets, "offsets", torch.int32), (motion, "motion", torch.float64))
    for t, name, dtype in tensors:
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor" % name)
        if t.dtype != dtype:
            raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    for t, name, _ in tensors:
        if t.device.type != "cuda":
            raise RuntimeError("%s must be a CUDA tensor (HIP device); ogc_amd has no CPU path" % name)
    if pc.dim() != 2 or pc.shape[1] != 3:
        raise ValueError("pc must be (total, 3), got %s" % (tuple(pc.shape),))
    total = pc.shape[0]
    if tuple(flow.shape) != (total, 3):
        raise ValueError("flow must be (%d, 3), got %s" % (total, tuple(flow.shape)))
    for t, name in ((segm, "segm"), (semantic_segm, "semantic_segm")):
        if tuple(t.shape) != (total,):
            raise ValueError("%s must be (%d,), got %s" % (name, total, tuple(t.shape)))
    if offsets.dim() != 1 or offsets.shape[0] < 1:
        raise ValueError("offsets must be (B + 1,), got %s" % (tuple(offsets.shape),))
    batch = offsets.shape[0] - 1
    if tuple(motion.shape) != (batch, 12):
        raise ValueError("motion must be (%d, 12), got %s" % (batch, tuple(motion.shape)))
    for t, name, _ in tensors:
        if not t.is_contiguous():
            raise RuntimeError("%s must be contiguous" % name)
    if total > 0x7fffffff:
        raise ValueError("%d points are beyond 32-bit offsets" % total)
    ignore = [int(c) for c in ignore_class_ids]
    if int(ignore_npoint_thresh) != ignore_npoint_thresh or ignore_npoint_thresh < 0:
        raise ValueError("ignore_npoint_thresh must be an integer >= 0, got %r" % (ignore_npoint_thresh,))
    if not (np.isfinite(ground_y) and np.isfinite(moving_thresh) and moving_thresh >= 0):
        raise ValueError("ground_y must be finite and moving_thresh finite and >= 0, got %r, %r" % (ground_y, moving_thresh))
    ign = torch.tensor(ignore, dtype=torch.int32, device=pc.device)
    stats = torch.empty(batch, 4, dtype=torch.int32, device=pc.device)
    _native.moving_stats_wrapper(batch, total, offsets, pc, flow, segm, semantic_segm, motion, ign, len(ignore), int(ignore_npoint_thresh),
                                 ground_y, moving_thresh, stats)
    return stats


MOVING_STATUS = {1: "a label outside [0, %d)" % MOVING_STATS_LABEL_CAP, 2: "offsets that descend or leave the arrays"}


def moving_counts(*args, **kwargs):
    """moving_stats and the single device -> host copy: numpy (B, 3) int32 = {n_distinct, n_fg, n_mov} per sample.  A sample with
    a status set is a ValueError that names it."""
    stats = moving_stats(*args, **kwargs).cpu().numpy()
    bad = np.nonzero(stats[:, 3])[0]
    if bad.size:
        raise ValueError("moving_stats: " + "; ".join("sample %d has %s" % (b, MOVING_STATUS.get(int(stats[b, 3]), "status %d" % stats[b, 3]))
                                                      for b in bad))
    return stats[:, :3]

"""Writes tests/golden/scan_prepare.npz: inputs and expected results for the crop and box-labelling kernels
(ogc_amd/csrc/scan_prepare.hip, ogc_amd/data_prepare/scan_ops.py).  CPU only.

    python tests/golden/make_scan_prepare_golden.py --reference <root of the reference tree>

Camera crop.  `crop_camera_mirror` is the float64 statement of process_kittidet.py:99-114 / process_semantickitti.py:61-78
written for this repository, element by element in the order include/ogc_ops.h documents (the reference goes through np.dot,
whose summation order belongs to the BLAS it meets).  What makes EQUAL count, keep_idx and out_pc a fair demand is asserted on the
drawn inputs: among the points that pass the clip test no u, W - u, v, H - v within 1e-6 px of zero; the same chain evaluated
in np.longdouble gives the same decisions and the same fp32 value of every rect coordinate; and the np.dot chain of the
reference's calibration class gives the same results as the mirror on this machine.  A point that fails is redrawn alone and
counted.

Box labelling.  The expected labels are what the reference's own `process_waymo.box_to_segm` (numpy and scipy only) returns for
float64 boxes; `box_segm_mirror` on the rows of `kitti_io.waymo_boxes` must equal it everywhere, float32 boxes must give the same
labels, and no |q_i - bound| may lie below 1e-7 m.

Front crop: `crop_front_mirror` IS the reference's expression in numpy float32; the GPU test draws its own frames.
The smallest margin of each kind goes into the metadata.
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
THRESHOLDS = {"pixel": 1e-6, "face": 1e-7}
TILE = 1024     # OGC_SCAN_CROP_TILE
CHUNK = 128     # OGC_BOX_SEGM_CHUNK

# a KITTI-like calibration: the velodyne frame (x forward, y left, z up) turned into the camera's (x right, y down, z forward) with
# a tilt of about a degree, a rectifying rotation of a few milliradians and a 721-px pinhole with a baseline term
CALIB = {
    "P": np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]]),
    "V2C": np.array([[0.0075337, -0.9999714, -0.0006166, -0.00406977], [0.0148025, 0.0007281, -0.9998902, -0.0763162],
                     [0.9998621, 0.0075238, 0.0148075, -0.2717806]]),
    "R0": np.array([[0.9999239, 0.00983776, -0.00744505], [-0.0098698, 0.9999421, -0.00427846], [0.00740253, 0.00435161, 0.9999631]]),
}
WIDTH, HEIGHT, CLIP, DEPTH = 1242, 375, 2.0, 35.0


# ---- mirrors ---------------------------------------------------------------------------------------------------------------
def camera_chain(scan, calib, dtype=np.float64):
    """(rect (N, 3), u, v) of the projection, element by element, sums left to right, in `dtype`."""
    x, y, z = (scan[:, i].astype(dtype) for i in range(3))
    V, P = np.asarray(calib["V2C"]).astype(dtype), np.asarray(calib["P"]).astype(dtype)
    with np.errstate(all="ignore"):
        r = [((V[i, 0] * x + V[i, 1] * y) + V[i, 2] * z) + V[i, 3] for i in range(3)]
        if calib.get("R0") is not None:
            R = np.asarray(calib["R0"]).astype(dtype)
            r = [(R[i, 0] * r[0] + R[i, 1] * r[1]) + R[i, 2] * r[2] for i in range(3)]
        img = [((P[i, 0] * r[0] + P[i, 1] * r[1]) + P[i, 2] * r[2]) + P[i, 3] for i in range(3)]
        u, v = img[0] / img[2], img[1] / img[2]
    return np.stack(r, 1), u, v


def crop_camera_mirror(scan, calib, width, height, clip_distance=2.0, depth_thresh=35.0, dtype=np.float64, parts=False):
    """scan (N, >= 3) float32 -> (out_pc (M, 3) float32, keep_idx (M,) int32): the camera crop in scan order."""
    scan = np.asarray(scan)
    rect, u, v = camera_chain(scan, calib, dtype)
    with np.errstate(all="ignore"):
        fov = (u < width) & (u >= 0) & (v < height) & (v >= 0)
        clip = scan[:, 0] > np.float32(clip_distance)
        out = (rect * np.array([-1.0, -1.0, 1.0], dtype=dtype)).astype(np.float32)
        near = out[:, 2] < np.float32(depth_thresh)
    keep = fov & clip & near
    if parts:
        return out, keep, clip, u, v
    return out[keep], np.nonzero(keep)[0].astype(np.int32)


def crop_camera_numpy(scan, calib, width, height, clip_distance=2.0, depth_thresh=35.0):
    """The same crop through np.dot on homogeneous points, as the reference's calibration class goes."""
    pc_velo = np.asarray(scan)[:, :3]
    hom = np.hstack((pc_velo, np.ones((pc_velo.shape[0], 1))))
    with np.errstate(all="ignore"):
        rect = np.dot(hom, np.transpose(calib["V2C"]))
        if calib.get("R0") is not None:
            rect = np.transpose(np.dot(calib["R0"], np.transpose(rect)))
        img = np.dot(np.hstack((rect, np.ones((rect.shape[0], 1)))), np.transpose(calib["P"]))
        img[:, 0] /= img[:, 2]
        img[:, 1] /= img[:, 2]
        fov = (img[:, 0] < width) & (img[:, 0] >= 0) & (img[:, 1] < height) & (img[:, 1] >= 0)
        fov = fov & (pc_velo[:, 0] > clip_distance)
        pc = rect[fov]
        idx = np.nonzero(fov)[0]
        pc[:, :2] *= -1.
        pc = pc.astype(np.float32)
        near = pc[:, 2] < depth_thresh
    return pc[near], idx[near].astype(np.int32)


def crop_front_mirror(scan):
    """process_waymo.py:132-141 in numpy float32: scan (N, 6) -> (pc (M, 3), keep_idx (M,) int32)."""
    scan = np.asarray(scan)
    pc, flag = scan[:, :3], scan[:, 5]
    with np.errstate(all="ignore"):
        keep = ((flag == -1) * (pc[:, 0] > abs(pc[:, 1])) * ((np.square(pc[:, 0]) + np.square(pc[:, 1]) + np.square(pc[:, 2])) < 60 * 60)
                * (abs(pc[:, 1]) < 50) * (pc[:, 0] < 35))
    return pc[keep], np.nonzero(keep)[0].astype(np.int32)


def box_segm_mirror(pc, boxes, ids, sign=(1, 1, 1), margins=None):
    """pc (N, 3) float32, boxes (K, 18) float64 rows [rot | centre | lo | hi], ids (K, 2) -> (segm, semantic_segm) int32; the
    boxes overwrite one another in order.  `margins`, a list, receives the smallest |q_i - bound| of every box."""
    p = np.asarray(pc, dtype=np.float32) * np.asarray(sign, dtype=np.float32)
    p = p.astype(np.float64)
    segm, semantic = np.zeros(p.shape[0], dtype=np.int32), np.zeros(p.shape[0], dtype=np.int32)
    for k in range(boxes.shape[0]):
        rot, c, lo, hi = boxes[k, 0:9].reshape(3, 3), boxes[k, 9:12], boxes[k, 12:15], boxes[k, 15:18]
        d = p - c
        q = np.stack([(rot[i, 0] * d[:, 0] + rot[i, 1] * d[:, 1]) + rot[i, 2] * d[:, 2] for i in range(3)], 1)
        inside = ((lo < q) & (q < hi)).all(1)
        if margins is not None and p.shape[0]:
            margins.append(float(min(np.abs(q - lo).min(), np.abs(q - hi).min())))
        segm[inside] = ids[k, 0]
        semantic[inside] = ids[k, 1]
    return segm, semantic


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def draw_scan(n, rs):
    """A velodyne-like scan (n, 4): most points in front within 45 m, some behind, some beyond the depth threshold."""
    scan = np.stack([-10.0 + 55.0 * rs.rand(n), (rs.rand(n) - 0.5) * 60.0, -3.0 + 5.0 * rs.rand(n), rs.rand(n)], 1)
    near = rs.rand(n) < 0.7                      # most of the points inside a +-40 degree wedge, so that many survive
    scan[near, 1] = scan[near, 0] * (rs.rand(int(near.sum())) - 0.5) * 1.6
    scan[near, 2] = -1.7 + 2.5 * rs.rand(int(near.sum()))
    return scan.astype(np.float32)


def camera_point_ok(scan, calib, record=None):
    """Per point: the fairness conditions of the module docstring."""
    out, keep, clip, u, v = crop_camera_mirror(scan, calib, WIDTH, HEIGHT, CLIP, DEPTH, parts=True)
    out_l, keep_l, _, _, _ = crop_camera_mirror(scan, calib, WIDTH, HEIGHT, CLIP, DEPTH, dtype=np.longdouble, parts=True)
    with np.errstate(all="ignore"):
        pixel = np.minimum(np.minimum(np.abs(u), np.abs(WIDTH - u)), np.minimum(np.abs(v), np.abs(HEIGHT - v)))
    pixel = np.where(clip & np.isfinite(pixel), pixel, np.inf)
    same = (keep == keep_l) & (out.view(np.int32) == out_l.view(np.int32)).all(1)
    if record is not None:
        record.append(float(pixel.min()))
    return same & (pixel >= THRESHOLDS["pixel"])


def camera_case(n, seed):
    rs = np.random.RandomState(seed)
    scan = draw_scan(n, rs)
    redrawn = 0
    for calib in (CALIB, {k: v for k, v in CALIB.items() if k != "R0"}):
        for _ in range(100):
            bad = np.nonzero(~camera_point_ok(scan, calib))[0]
            if bad.size == 0:
                break
            scan[bad] = draw_scan(bad.size, rs)
            redrawn += int(bad.size)
        else:
            raise RuntimeError("the camera case does not settle")
    # the special rows come last so that they never shift: NaN, inf, the origin (all rejected, as numpy rejects them)
    scan[-3:] = np.array([[np.nan, 1.0, 1.0, 0.0], [np.inf, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]], dtype=np.float32)
    return scan, redrawn


def draw_boxes(k, rs):
    """Waymo-like boxes (k, 7) float64 [x, y, z, l, w, h, heading], crowded enough to overlap."""
    return np.stack([2.0 + 30.0 * rs.rand(k), (rs.rand(k) - 0.5) * 30.0, (rs.rand(k) - 0.5) * 1.5, 1.5 + 4.0 * rs.rand(k),
                     0.8 + 1.8 * rs.rand(k), 1.0 + 1.5 * rs.rand(k), (rs.rand(k) - 0.5) * 2 * np.pi], 1)


def draw_box_points(n, gt, rs):
    """Half of the points inside or just around a box, the rest anywhere."""
    k = gt.shape[0]
    which = rs.randint(k, size=n)
    local = (rs.rand(n, 3) - 0.5) * 1.15 * gt[which][:, [3, 5, 4]]        # x: l, y: h, z: w as the reference pairs them
    c, s = np.cos(gt[which, 6]), np.sin(gt[which, 6])
    world = np.stack([c * local[:, 0] - s * local[:, 1], s * local[:, 0] + c * local[:, 1], local[:, 2]], 1) + gt[which, 0:3]
    free = np.stack([35.0 * rs.rand(n), (rs.rand(n) - 0.5) * 34.0, (rs.rand(n) - 0.5) * 3.0], 1)
    return np.where((rs.rand(n) < 0.5)[:, None], world, free).astype(np.float32)


def box_case(n, k, seed, reference_fn, waymo_boxes):
    rs = np.random.RandomState(seed)
    gt = draw_boxes(k, rs)
    object_ids = (rs.permutation(k) + 1).astype(np.int32)
    class_ids = (1 + rs.randint(3, size=k)).astype(np.int32)
    pc = draw_box_points(n, gt, rs)
    rows, ids = waymo_boxes(gt, object_ids, class_ids)
    redrawn = 0
    for _ in range(100):
        q_margin = np.full(n, np.inf)
        p = pc.astype(np.float64)
        for b in range(k):
            rot, c, lo, hi = rows[b, 0:9].reshape(3, 3), rows[b, 9:12], rows[b, 12:15], rows[b, 15:18]
            q = (p - c) @ rot.T
            q_margin = np.minimum(q_margin, np.minimum(np.abs(q - lo), np.abs(q - hi)).min(1))
        bad = np.nonzero(q_margin < THRESHOLDS["face"])[0]
        if bad.size == 0:
            break
        pc[bad] = draw_box_points(bad.size, gt, rs)
        redrawn += int(bad.size)
    else:
        raise RuntimeError("the box case does not settle")
    want = reference_fn(pc, gt, object_ids, class_ids)
    margins = []
    got = box_segm_mirror(pc, rows, ids, margins=margins)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), "the mirror differs from the reference's function"
    want32 = reference_fn(pc, gt.astype(np.float32), object_ids, class_ids)
    assert np.array_equal(want32[0], want[0]) and np.array_equal(want32[1], want[1]), "float32 boxes decide differently"
    per_point = np.zeros(n, dtype=np.int32)
    for b in range(k):
        per_point += box_segm_mirror(pc, rows[b:b + 1], np.ones((1, 2), np.int32))[0]
    return {"pc": pc, "gt": gt, "object_ids": object_ids, "class_ids": class_ids, "segm": want[0].astype(np.int32),
            "semantic_segm": want[1].astype(np.int32)}, min(margins), redrawn, int((per_point >= 2).sum()), int((per_point >= 3).sum())


def build(reference_root):
    sys.path.insert(0, ROOT)
    from ogc_amd.data_prepare.kitti_io import waymo_boxes
    sys.path.insert(0, os.path.join(reference_root, "data_prepare", "waymo"))
    import process_waymo as ref
    out, meta = {}, {"thresholds": THRESHOLDS, "width": WIDTH, "height": HEIGHT, "clip_distance": CLIP, "depth_thresh": DEPTH,
                     "cases": {}}
    for key, value in CALIB.items():
        out["calib_" + key] = value

    n = 2 * TILE + 301
    scan, redrawn = camera_case(n, seed=11)
    out["cam_scan"] = scan
    pixel = []
    for name, calib in (("cam_r0", CALIB), ("cam_noR0", {k: v for k, v in CALIB.items() if k != "R0"})):
        ok = camera_point_ok(scan[:-3], calib, record=pixel)
        assert ok.all()
        pc, idx = crop_camera_mirror(scan, calib, WIDTH, HEIGHT, CLIP, DEPTH)
        pc_np, idx_np = crop_camera_numpy(scan, calib, WIDTH, HEIGHT, CLIP, DEPTH)
        assert np.array_equal(idx, idx_np) and np.array_equal(pc.view(np.int32), pc_np.view(np.int32)), "np.dot chain differs"
        assert idx.size > TILE // 2 and idx.size < n - TILE // 2 and idx[-1] < n - 3
        out[name + "_pc"], out[name + "_keep_idx"] = pc, idx
        meta["cases"][name] = {"n": n, "kept": int(idx.size), "R0": "R0" in calib}
        print("%-9s n %d kept %d" % (name, n, idx.size))
    meta["camera_points_redrawn"] = redrawn
    meta["smallest_pixel_margin"] = min(pixel)
    print("camera: %d points redrawn, smallest pixel margin %.3g" % (redrawn, min(pixel)))

    face, box_redrawn = [], 0
    for name, n, k, seed in (("box_a", 3000, 40, 21), ("box_b", 1500, CHUNK + 5, 22)):
        case, margin, redrawn, in2, in3 = box_case(n, k, seed, ref.box_to_segm, waymo_boxes)
        assert in3 >= 5, "too few points inside three boxes"
        for key, value in case.items():
            out["%s_%s" % (name, key)] = value
        meta["cases"][name] = {"n": n, "k": k, "labelled": int((case["segm"] > 0).sum()), "in_two_boxes": in2, "in_three_boxes": in3}
        face.append(margin)
        box_redrawn += redrawn
        print("%-9s n %d k %d labelled %d, in >= 2 boxes %d, in >= 3 boxes %d, smallest face margin %.3g, redrawn %d"
              % (name, n, k, (case["segm"] > 0).sum(), in2, in3, margin, redrawn))
    meta["box_points_redrawn"] = box_redrawn
    meta["smallest_face_margin"] = min(face)
    out["meta"] = np.asarray(json.dumps(meta))
    return out, meta


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference tree (its data_prepare/waymo/process_waymo.py is imported)")
    args = ap.parse_args()
    out, meta = build(args.reference)
    path = os.path.join(HERE, "scan_prepare.npz")
    np.savez_compressed(path, **out)
    print({k: v for k, v in meta.items() if k != "cases"})
    print("%s: %d bytes" % (path, os.path.getsize(path)))

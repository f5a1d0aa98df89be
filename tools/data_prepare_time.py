"""Time of the two data-preparation kernels at the sizes they run at — one Waymo frame (180 000 x 6 points, 120 boxes on the
cropped frame) and one KITTI frame (120 000 x 4 points, 12 `Car` boxes on 8192 sampled points):

  device   HIP-event time of the launches alone on preallocated outputs: ogc_scan_crop_front / ogc_scan_crop_camera (two
           kernels each) and ogc_box_segm, plus the wall time of the public operator (allocation, launch, the read of `count`)
  host     the numpy mirror of the same stage (tests/golden/make_scan_prepare_golden.py: the reference's arithmetic), wall time,
           for orientation: what the reference's scripts spend there per frame

after warm-up and after a check that both give the same results.  Needs the GPU.

    python tools/data_prepare_time.py [--calls 200] [--warmup 20] [--host-calls 5] [--out profiles/data_prepare_time.txt]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_scan_prepare_golden as mirror  # noqa: E402
from ogc_amd import pointnet2_cuda as nat  # noqa: E402
from ogc_amd.data_prepare import kitti_io, scan_ops  # noqa: E402


def summary(ms):
    ms = sorted(ms)
    return "median %.4f ms, min %.4f, p90 %.4f over %d calls" % (statistics.median(ms), ms[0], ms[int(0.9 * len(ms))], len(ms))


def events(fn, calls, warmup):
    out = []
    for i in range(warmup + calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= warmup:
            out.append(e0.elapsed_time(e1))
    return out


def wall(fn, calls, warmup, device=True):
    out = []
    for i in range(warmup + calls):
        if device:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if device:
            torch.cuda.synchronize()
        if i >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return out


def waymo_frame(n, rs):
    scan = np.stack([-75.0 + 150.0 * rs.rand(n), (rs.rand(n) - 0.5) * 150.0, -2.0 + 6.0 * rs.rand(n), rs.rand(n), rs.rand(n),
                     np.where(rs.rand(n) < 0.1, 0.0, -1.0)], 1)
    front = rs.rand(n) < 0.6                                   # the share of a real frame that survives is roughly a third
    scan[front, 0] = 35.0 * rs.rand(int(front.sum()))
    scan[front, 1] = scan[front, 0] * (rs.rand(int(front.sum())) - 0.5) * 2.4
    return scan.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "data_prepare_time.py measures on the GPU"
    lines = ["device: %s" % torch.cuda.get_device_name(0)]
    rs = np.random.RandomState(0)

    def crop_buffers(n):
        return (torch.empty(n, 3, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda"),
                torch.empty(1, dtype=torch.int32, device="cuda"))

    def box_stage(tag, pc_np, rows, ids, sign):
        pc, rows_d, ids_d = torch.from_numpy(pc_np).cuda(), torch.from_numpy(rows).cuda(), torch.from_numpy(ids).cuda()
        want = mirror.box_segm_mirror(pc_np, rows, ids, sign=sign)
        got = scan_ops.box_segm(pc, rows_d, ids_d, sign=sign)
        differ = int((got[0].cpu().numpy() != want[0]).sum())
        assert differ <= 2, differ                             # random points: one within rounding of a face plane may flip
        segm, semantic = torch.empty_like(got[0]), torch.empty_like(got[1])
        n, k = pc_np.shape[0], rows.shape[0]
        dev = events(lambda: nat.box_segm_wrapper(n, k, pc, sign, rows_d, ids_d, segm, semantic), args.calls, args.warmup)
        host = wall(lambda: mirror.box_segm_mirror(pc_np, rows, ids, sign=sign), args.host_calls, 1, device=False)
        return ["%s box labelling: %d points x %d boxes, %d labelled, %d of them differ from the mirror" % (tag, n, k, int((want[0] > 0).sum()), differ),
                "  ogc_box_segm launch alone, HIP events: %s" % summary(dev),
                "  numpy mirror on the host, wall: %s" % summary(host)]

    # ---- Waymo-sized frame
    n = 180000
    scan_np = waymo_frame(n, rs)
    scan = torch.from_numpy(scan_np).cuda()
    want = mirror.crop_front_mirror(scan_np)
    got = scan_ops.crop_front(scan)
    assert np.array_equal(got[1].cpu().numpy(), want[1]) and np.array_equal(got[0].cpu().numpy(), want[0])
    out_pc, keep_idx, count = crop_buffers(n)
    dev = events(lambda: nat.scan_crop_front_wrapper(n, 6, scan, out_pc, keep_idx, count), args.calls, args.warmup)
    op = wall(lambda: scan_ops.crop_front(scan), args.calls, args.warmup)
    host = wall(lambda: mirror.crop_front_mirror(scan_np), args.host_calls, 1, device=False)
    lines += ["Waymo front crop: %d x 6 points, %d kept; input %.2f MB" % (n, want[1].shape[0], scan_np.nbytes / 1e6),
              "  ogc_scan_crop_front, two launches alone, HIP events: %s" % summary(dev),
              "  scan_ops.crop_front (allocation, launches, read of count), wall: %s" % summary(op),
              "  numpy mirror on the host, wall: %s" % summary(host)]
    cropped = np.ascontiguousarray(want[0])
    gt = np.stack([35.0 * rs.rand(120), (rs.rand(120) - 0.5) * 40.0, 4.0 * rs.rand(120), 1.0 + 5.0 * rs.rand(120), 0.8 + 2.0 * rs.rand(120),
                   1.0 + 2.0 * rs.rand(120), (rs.rand(120) - 0.5) * 2 * np.pi], 1)
    rows, ids = kitti_io.waymo_boxes(gt, np.arange(1, 121), 1 + np.arange(120) % 3)
    lines += box_stage("Waymo", cropped, rows, ids, (1, 1, 1))

    # ---- KITTI-sized frame
    n = 120000
    scan_np = mirror.draw_scan(n, rs)
    scan = torch.from_numpy(scan_np).cuda()
    calib = mirror.CALIB
    want = mirror.crop_camera_mirror(scan_np, calib, mirror.WIDTH, mirror.HEIGHT)
    got = scan_ops.crop_camera(scan, calib, mirror.WIDTH, mirror.HEIGHT)
    differ = abs(got[1].shape[0] - want[1].shape[0])
    assert differ <= 2, differ                                 # random points: one within rounding of an image edge may flip
    cam = torch.from_numpy(scan_ops.camera_block(calib, mirror.WIDTH, mirror.HEIGHT)).cuda()
    out_pc, keep_idx, count = crop_buffers(n)
    dev = events(lambda: nat.scan_crop_camera_wrapper(n, 4, scan, cam, 2.0, 35.0, out_pc, keep_idx, count), args.calls, args.warmup)
    op = wall(lambda: scan_ops.crop_camera(scan, calib, mirror.WIDTH, mirror.HEIGHT), args.calls, args.warmup)
    host = wall(lambda: mirror.crop_camera_numpy(scan_np, calib, mirror.WIDTH, mirror.HEIGHT), args.host_calls, 1, device=False)
    lines += ["KITTI camera crop: %d x 4 points, %d kept (mirror: %d); input %.2f MB" % (n, got[1].shape[0], want[1].shape[0], scan_np.nbytes / 1e6),
              "  ogc_scan_crop_camera, two launches alone, HIP events: %s" % summary(dev),
              "  scan_ops.crop_camera (parameter upload, allocation, launches, read of count), wall: %s" % summary(op),
              "  numpy (np.dot chain of the reference) on the host, wall: %s" % summary(host)]
    sampled = np.ascontiguousarray(want[0][rs.permutation(want[0].shape[0])[:8192]])
    objects = [kitti_io.Object3d("Car 0.00 0 -1.57 100.00 120.00 300.00 220.00 %.2f %.2f %.2f %.2f 1.65 %.2f %.2f"
                                 % (1.4 + 0.4 * rs.rand(), 1.5 + 0.4 * rs.rand(), 3.2 + 1.2 * rs.rand(), (rs.rand() - 0.5) * 30.0,
                                    5.0 + 28.0 * rs.rand(), (rs.rand() - 0.5) * 6.0)) for _ in range(12)]
    rows, ids = kitti_io.kittidet_boxes(objects)
    lines += box_stage("KITTI", sampled, rows, ids, kitti_io.KITTIDET_SIGN)

    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

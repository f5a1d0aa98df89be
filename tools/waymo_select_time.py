"""Time of the selection of moving Waymo samples (ogc_amd/data_prepare/select_mov.py) at the shape it runs at — a batch
of 64 frame pairs x 8192 points (make_waymo_select_golden.draw_sample):

  kernel   HIP-event time of ogc_moving_stats alone, on tensors that are on the device already
  step     wall time of the whole device step of a batch: concatenation on the host, upload, launch, the copy of the integers back
  host     wall time of the numpy mirror (tests/golden/make_waymo_select_golden.py::moving_mirror) over the same batch — the
           reference's path without its reader's second frame —, the baseline
  files    wall time of reading the batch's files (four arrays and two poses per pair) from a temporary directory, i.e. from the
           page cache: a LOWER bound of what a run pays for its reads

after warm-up and after a check that device and mirror give the same integers.  Needs the GPU.

    python tools/waymo_select_time.py [--calls 200] [--warmup 20] [--host-calls 5] [--out profiles/waymo_select_time.txt]"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_waymo_select_golden as mirror  # noqa: E402
from ogc_amd import pointnet2_cuda as nat  # noqa: E402
from ogc_amd.data_prepare import scan_ops  # noqa: E402

BATCH, N_POINT = 64, 8192
IGNORE, THRESH = (2, 3), 50


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


def device_step(samples):
    """What select_mov.batch_counts does after its reads: concatenate, upload, launch, copy back."""
    offsets = np.cumsum([0] + [s[0].shape[0] for s in samples]).astype(np.int32)
    up = [torch.from_numpy(np.concatenate([s[k] for s in samples], 0)).cuda() for k in range(4)]
    motion = torch.from_numpy(np.stack([s[4] for s in samples], 0)).cuda()
    return scan_ops.moving_counts(*up, torch.from_numpy(offsets).cuda(), motion, ignore_class_ids=IGNORE, ignore_npoint_thresh=THRESH)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "waymo_select_time.py measures on the GPU"
    lines = ["device: %s" % torch.cuda.get_device_name(0)]
    samples = [mirror.draw_sample(N_POINT, np.random.RandomState(500 + b), ("moving", "static")[b % 2], n_label=40) for b in range(BATCH)]

    def host():
        return np.array([mirror.moving_mirror(*s, IGNORE, THRESH) for s in samples], dtype=np.int32)
    want = host()
    assert np.array_equal(device_step(samples), want)
    offsets = torch.from_numpy(np.cumsum([0] + [N_POINT] * BATCH).astype(np.int32)).cuda()
    dev = [torch.from_numpy(np.concatenate([s[k] for s in samples], 0)).cuda() for k in range(4)]
    motion = torch.from_numpy(np.stack([s[4] for s in samples], 0)).cuda()
    ign = torch.tensor(IGNORE, dtype=torch.int32, device="cuda")
    stats = torch.empty(BATCH, 4, dtype=torch.int32, device="cuda")
    total = BATCH * N_POINT
    kernel = events(lambda: nat.moving_stats_wrapper(BATCH, total, offsets, dev[0], dev[1], dev[2], dev[3], motion, ign, len(IGNORE), THRESH,
                                                     0.3, 0.2, stats), args.calls, args.warmup)
    step = wall(lambda: device_step(samples), args.calls, args.warmup)
    cpu = wall(host, args.host_calls, 1, device=False)
    with tempfile.TemporaryDirectory() as tmp:
        for b, s in enumerate(samples):
            for k, what in enumerate(("pc", "flow", "segm", "semantic_segm")):
                np.save(os.path.join(tmp, "%s_%04d.npy" % (what, b)), s[k].astype(np.float64) if what == "flow" else s[k])
            np.save(os.path.join(tmp, "pose_%04d.npy" % b), np.eye(4))

        def read():
            for b in range(BATCH):
                for what in ("pc", "flow", "segm", "semantic_segm", "pose", "pose"):
                    np.load(os.path.join(tmp, "%s_%04d.npy" % (what, b)))
        files = wall(read, args.host_calls, 1, device=False)
    read_bytes = total * (12 + 12 + 4 + 4)
    lines += ["Waymo moving-sample selection: %d pairs x %d points; device == mirror in every integer (%d pairs with n_mov > 0)"
              % (BATCH, N_POINT, int((want[:, 2] > 0).sum())),
              "  bytes the kernel reads: %.2f MB (32 B per point)" % (read_bytes / 1e6),
              "  ogc_moving_stats, one launch alone, HIP events: %s" % summary(kernel),
              "  device step of a batch (host concatenation, upload, launch, copy back), wall: %s" % summary(step),
              "  numpy mirror on the host for the same batch, wall: %s" % summary(cpu),
              "  reading the batch's files (pc, float64 flow, two label arrays, two poses per pair) from the page cache, wall: %s" % summary(files)]
    med = {k: statistics.median(v) for k, v in (("kernel", kernel), ("step", step), ("cpu", cpu), ("files", files))}
    bound = "file reads" if med["files"] > max(med["step"], 0.0) else "the device step"
    lines.append("  the stage with the device step: reads %.2f ms + step %.2f ms per batch; with the host mirror: reads %.2f ms + mirror %.2f ms;"
                 " the larger part of the stage as built is %s, and a cold disk only adds to the reads" % (med["files"], med["step"], med["files"], med["cpu"], bound))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

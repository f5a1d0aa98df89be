"""Time of the KITTI Scene Flow preparation stage at the size it runs at — one 375 x 1242 frame (make_kittisf_maps: about
44 % of the pixels kept):

  device   HIP-event time of the three launches of ogc_kittisf_unproject alone, on preallocated outputs, and the wall time of
           the public operator scan_ops.kittisf_unproject (parameter upload, allocation, launches, the read of `count`)
  host     wall time of png16.read_png per kind of file (16-bit grey, 16-bit RGB; inflate, ogc_png_unfilter, byte swap), and of
           the numpy mirror of the device stage (tests/golden/make_kittisf_prepare_golden.py), for orientation: the reference
           walks the image in a Python double loop instead

after warm-up and after a check that device and mirror give the same bits.  Needs the GPU.

    python tools/kittisf_prepare_time.py [--calls 200] [--warmup 20] [--host-calls 10] [--out profiles/kittisf_prepare_time.txt]"""
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
import make_kittisf_prepare_golden as mirror  # noqa: E402
from ogc_amd import pointnet2_cuda as nat  # noqa: E402
from ogc_amd.data_prepare import png16, scan_ops  # noqa: E402
from ogc_amd.data_prepare.process_kittisf import upload  # noqa: E402
from ogc_amd.utils.synthetic import make_kittisf_maps  # noqa: E402

HEIGHT, WIDTH = 375, 1242


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-calls", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "kittisf_prepare_time.py measures on the GPU"
    lines = ["device: %s" % torch.cuda.get_device_name(0)]
    maps_np = make_kittisf_maps(HEIGHT, WIDTH, np.random.RandomState(0))
    P = mirror.p_rect()
    maps = [upload(m) for m in maps_np]
    want = mirror.unproject_mirror(*maps_np, P)
    got = scan_ops.kittisf_unproject(*maps, P)
    assert np.array_equal(got[3].cpu().numpy(), want[3]) and np.array_equal(got[2].cpu().numpy(), want[2])
    assert np.array_equal(got[0].cpu().numpy().view(np.int32), want[0].view(np.int32))
    assert np.array_equal(got[1].cpu().numpy().view(np.int32), want[1].view(np.int32))
    n, m = HEIGHT * WIDTH, want[3].shape[0]
    out = (torch.empty(n, 3, device="cuda"), torch.empty(n, 3, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda"),
           torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda"))
    sel = torch.tensor(scan_ops.KITTISF_SELECT_SEMANTICS, dtype=torch.int32, device="cuda")
    scalars = [float(v) for v in (np.float32(P[0, 0] * 0.54), P[0, 0], P[0, 2], P[0, 3], P[1, 2], P[1, 3], P[2, 3], 35.0)]
    dev = events(lambda: nat.kittisf_unproject_wrapper(HEIGHT, WIDTH, *maps, *scalars, sel, 2, *out), args.calls, args.warmup)
    op = wall(lambda: scan_ops.kittisf_unproject(*maps, P), args.calls, args.warmup)
    host = wall(lambda: mirror.unproject_mirror(*maps_np, P), args.host_calls, 1, device=False)
    moved = 2 * n * 12 + n * 2 + m * 32
    lines += ["KITTI-SF unprojection: %d x %d = %d pixels, %d kept, %d labels; device == mirror in every bit" % (HEIGHT, WIDTH, n, m, int(want[2].max())),
              "  bytes by the kernels' own reads and writes: %.2f MB (12 B per pixel twice, the ids once per kept pixel and pass, 32 B per kept point)" % (moved / 1e6),
              "  ogc_kittisf_unproject, three launches alone, HIP events: %s" % summary(dev),
              "  scan_ops.kittisf_unproject (parameter upload, allocation, launches, read of count), wall: %s" % summary(op),
              "  numpy mirror on the host, wall: %s" % summary(host)]
    with tempfile.TemporaryDirectory() as tmp:
        for tag, array in (("16-bit grey (disparity)", maps_np[0]), ("16-bit grey (instance)", maps_np[3]), ("16-bit RGB (flow)", maps_np[2])):
            path = os.path.join(tmp, "map.png")
            png16.write_png(path, array)
            assert np.array_equal(png16.read_png(path), array)
            ms = wall(lambda: png16.read_png(path), args.host_calls, 1, device=False)
            lines.append("  png16.read_png, %s, %.2f MB file, mixed filters, wall: %s" % (tag, os.path.getsize(path) / 1e6, summary(ms)))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

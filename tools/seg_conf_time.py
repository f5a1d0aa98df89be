"""Time of the confidences of one batch of predicted segmentations at the two shapes they are written at — B = 64 frames x
n = 8192 points x k = 18 slots (a test_seg batch of downsampled KITTI-Det frames) and B = 1 x n = 100000 x k = 18 (one raw
scan) — on masks that are the softmax of seeded normal logits:

  new path        ogc_amd.metrics.seg_conf.pseudo_label_confidences — ogc_slot_confidence + one (B, k + 1) device->host copy
  framework path  the composition it replaces, on the same device tensor: arg-max, one-hot, masked sums in float64, the sizes,
                  the division, and one copy of the (B, k) confidences and sizes

Wall time per batch with a device synchronisation before and after each call, the two paths alternating call by call in one
process, after warm-up and after a check that both give the same labels' confidences (to one float32 ulp); and the HIP-event
time of the ogc_slot_confidence launch alone on preallocated outputs.  Needs the GPU.

    python tools/seg_conf_time.py [--calls 300] [--warmup 30] [--out profiles/seg_conf_time.txt]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ogc_amd.metrics.seg_conf import pseudo_label_confidences, slot_confidence_batch  # noqa: E402
from ogc_amd.pointnet2_cuda import slot_confidence_wrapper  # noqa: E402

SHAPES = ((64, 8192, 18), (1, 100000, 18))


def summary(ms):
    ms = sorted(ms)
    return "median %.4f ms, min %.4f, p90 %.4f over %d calls" % (statistics.median(ms), ms[0], ms[int(0.9 * len(ms))], len(ms))


def framework_path(mask):
    """-> list of B float32 arrays, as pseudo_label_confidences."""
    k = mask.shape[2]
    own = torch.nn.functional.one_hot(mask.argmax(dim=2), k)                     # (B, n, k) i64
    sizes = own.sum(dim=1)                                                        # (B, k)
    sums = (mask.double() * own).sum(dim=1)                                       # (B, k) f64
    conf = (sums / sizes.clamp(min=1)).float()
    table = torch.cat([conf, sizes.float()], dim=1).cpu().numpy()                 # the only copy to the host
    return [table[b, :k][table[b, k:] > 0] for b in range(table.shape[0])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "seg_conf_time.py measures on the GPU"
    lines = ["device: %s" % torch.cuda.get_device_name(0)]
    for B, n, k in SHAPES:
        g = torch.Generator().manual_seed(B)
        mask = torch.softmax(torch.randn(B, n, k, generator=g), dim=2).cuda()

        def new_path():
            return pseudo_label_confidences(mask)

        def parent_path():
            return framework_path(mask)

        got, want = new_path(), parent_path()
        for a, b in zip(got, want):
            assert a.shape == b.shape and (np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32)) <= 1).all(), (a, b)
        for _ in range(args.warmup):
            new_path()
            parent_path()
        wall = {"new": [], "parent": []}
        for _ in range(args.calls):
            for name, fn in (("new", new_path), ("parent", parent_path)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                wall[name].append((time.perf_counter() - t0) * 1e3)

        res = slot_confidence_batch(mask)
        out = [torch.empty_like(t) for t in res]
        kernel = []
        for i in range(args.warmup + args.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            slot_confidence_wrapper(B, n, k, mask, *out)
            e1.record()
            e1.synchronize()
            if i >= args.warmup:
                kernel.append(e0.elapsed_time(e1))
        assert all(torch.equal(a, b) for a, b in zip(out, res))
        lines += ["shape: B=%d n=%d k=%d; input bytes %.2f MB" % (B, n, k, mask.numel() * 4 / 1e6),
                  "  pseudo_label_confidences (new path), wall per batch: %s" % summary(wall["new"]),
                  "  arg-max, one-hot, masked fp64 sums, division, copy (framework path), wall per batch: %s" % summary(wall["parent"]),
                  "  framework / new (medians): %.2f" % (statistics.median(wall["parent"]) / statistics.median(wall["new"])),
                  "  ogc_slot_confidence launch alone, HIP events: %s" % summary(kernel)]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

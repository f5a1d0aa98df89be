"""Time of the scene-flow evaluation of one batch at the two shapes it runs at — B = 48 pairs x N = 2048 points (an OGC-DR batch
of test_flow) and B = 1 x N = 100000 (one full-resolution KITTI-SF scan) — with predictions drawn to straddle the thresholds:

  new path      ogc_amd.metrics.flow_eval.eval_flow_device — ogc_flow_eval + one (B, 4) device->host copy
  parent path   ogc_amd.metrics.flow_metric.flow_metrics(...).tolist() on the same device tensors, unchanged

Wall time per batch with a device synchronisation before and after each call, the two paths alternating call by call in one
process, after warm-up and after a check that both give the same results; and the HIP-event time of the ogc_flow_eval launch
alone on preallocated outputs.  Needs the GPU.

    python tools/flow_eval_time.py [--calls 300] [--warmup 30] [--out profiles/flow_eval_time.txt]"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ogc_amd.metrics.flow_eval import eval_flow_device, flow_eval_batch  # noqa: E402
from ogc_amd.metrics.flow_metric import flow_metrics  # noqa: E402
from ogc_amd.pointnet2_cuda import flow_eval_wrapper  # noqa: E402

SHAPES = ((48, 2048, 0.01), (1, 100000, 0.05))


def summary(ms):
    ms = sorted(ms)
    return "median %.4f ms, min %.4f, p90 %.4f over %d calls" % (statistics.median(ms), ms[0], ms[int(0.9 * len(ms))], len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "flow_eval_time.py measures on the GPU"
    lines = ["device: %s" % torch.cuda.get_device_name(0)]
    for B, N, thresh in SHAPES:
        g = torch.Generator().manual_seed(B)
        gt = 5 * thresh * torch.randn(B, N, 3, generator=g)
        direction = torch.randn(B, N, 3, generator=g)
        pred = gt + direction / direction.norm(dim=2, keepdim=True) * thresh * 10.0 ** (3 * torch.rand(B, N, 1, generator=g) - 1.5)
        gt, pred = gt.cuda(), pred.cuda()

        def new_path():
            return eval_flow_device(gt, pred, epe_norm_thresh=thresh)[0]

        def parent_path():
            return flow_metrics(gt, pred, thresh).tolist()

        got, want = new_path(), parent_path()
        assert abs(got[0] - want[0]) <= 1e-6 * want[0], (got, want)
        assert all(abs(a - b) * B * N < 1.5 for a, b in zip(got[1:], want[1:])), (got, want)   # at most one point decided otherwise
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

        res = flow_eval_batch(gt, pred, thresh)
        epe_sum, counts = torch.empty_like(res.epe_sum), torch.empty_like(res.counts)
        kernel = []
        for i in range(args.warmup + args.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            flow_eval_wrapper(B, N, gt, pred, thresh, 1e-10, epe_sum, counts)
            e1.record()
            e1.synchronize()
            if i >= args.warmup:
                kernel.append(e0.elapsed_time(e1))
        assert torch.equal(epe_sum, res.epe_sum) and torch.equal(counts, res.counts)
        lines += ["shape: B=%d N=%d epe_norm_thresh=%g; input bytes %.2f MB" % (B, N, thresh, 2 * gt.numel() * 4 / 1e6),
                  "  eval_flow_device (new path), wall per batch: %s" % summary(wall["new"]),
                  "  flow_metrics(...).tolist() (parent path), wall per batch: %s" % summary(wall["parent"]),
                  "  parent / new (medians): %.2f" % (statistics.median(wall["parent"]) / statistics.median(wall["new"])),
                  "  ogc_flow_eval launch alone, HIP events: %s" % summary(kernel)]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

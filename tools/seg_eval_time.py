"""Time of the segmentation evaluation of one batch at the evaluation shape of test_seg (B = 64 clouds x n = 8192 points,
k = `n_slot` of config/kittisf_unsup_synthetic.yaml, twelve labelled objects, masks = soft-max of random logits, the outdoor
ignore threshold of 50 points):

  new path      ogc_amd.metrics.seg_eval.accumulate_seg_eval — ogc_seg_eval + ogc_lsap_maximize + one device->host copy
  parent path   ogc_amd.metrics.seg_metric.accumulate_eval_results + ClusteringMetrics on the same device tensors, both unchanged

Wall time per batch with a device synchronisation before and after each call, the two paths alternating call by call in one
process, after warm-up and after a check that both give the same results; and the HIP-event time of the ogc_seg_eval launch
alone on preallocated outputs.  Needs the GPU.

    python tools/seg_eval_time.py [--calls 200] [--warmup 20] [--out profiles/seg_eval_time.txt]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ogc_amd.metrics.seg_eval import accumulate_seg_eval, seg_eval_batch  # noqa: E402
from ogc_amd.metrics.seg_metric import ClusteringMetrics, accumulate_eval_results  # noqa: E402
from ogc_amd.pointnet2_cuda import seg_eval_wrapper  # noqa: E402

B, N, N_OBJECTS, THRESH = 64, 8192, 12, 50


def summary(ms):
    ms = sorted(ms)
    return "median %.4f ms, min %.4f, p90 %.4f over %d calls" % (statistics.median(ms), ms[0], ms[int(0.9 * len(ms))], len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "seg_eval_time.py measures on the GPU"
    with open(os.path.join(ROOT, "config", "kittisf_unsup_synthetic.yaml")) as f:
        k = yaml.safe_load(f)["segnet"]["n_slot"]
    g = torch.Generator().manual_seed(0)
    segm = torch.randint(0, N_OBJECTS, (B, N), generator=g).cuda()                       # int64, as the loaders' labels after .long()
    segm32 = segm.to(torch.int32)
    mask = torch.softmax(4 * torch.rand(B, N, k, generator=g), dim=2).cuda()
    clustering = ClusteringMetrics()

    def new_path():
        return accumulate_seg_eval(segm32, mask, THRESH)

    def parent_path():
        table = accumulate_eval_results(segm, mask, THRESH)
        per = clustering(mask, segm, THRESH)
        return table + (np.asarray(per["iou"]), np.asarray(per["ri"]))

    got, want = new_path(), parent_path()
    assert got[3] == want[3] and np.array_equal(got[1], want[1])
    np.testing.assert_allclose(got[0], want[0], rtol=2.0 ** -52, atol=0)
    np.testing.assert_allclose(got[2], want[2], rtol=(2 * N + 2) * 2.0 ** -53, atol=0)
    assert np.abs(got[4] - want[4]).max() <= 64 * 2.0 ** -24 and np.abs(got[5] - want[5]).max() <= 1e-15

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

    # the launch alone, on outputs allocated once
    res = seg_eval_batch(segm32, mask, THRESH)
    out = [torch.empty_like(t) for t in (res.hard, res.counts, res.pred_iou, res.confidence, res.valid.int(), res.n_gt, res.score,
                                         res.rows, res.ri, res.status)]
    kernel = []
    for i in range(args.warmup + args.calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        seg_eval_wrapper(B, N, k, segm32, mask, THRESH, *out)
        e1.record()
        e1.synchronize()
        if i >= args.warmup:
            kernel.append(e0.elapsed_time(e1))
    assert torch.equal(out[0], res.hard) and torch.equal(out[2], res.pred_iou) and torch.equal(out[3], res.confidence)

    new_med, parent_med = statistics.median(wall["new"]), statistics.median(wall["parent"])
    lines = ["device: %s" % torch.cuda.get_device_name(0),
             "shape: B=%d n=%d k=%d, %d labelled objects, ignore_npoint_thresh=%d; mask bytes %.1f MB"
             % (B, N, k, N_OBJECTS, THRESH, mask.numel() * 4 / 1e6),
             "accumulate_seg_eval (new path), wall per batch: %s" % summary(wall["new"]),
             "accumulate_eval_results + ClusteringMetrics (parent path), wall per batch: %s" % summary(wall["parent"]),
             "parent / new (medians): %.2f" % (parent_med / new_med),
             "ogc_seg_eval launch alone, HIP events: %s" % summary(kernel)]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

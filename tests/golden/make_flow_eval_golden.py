"""Writes tests/golden/flow_eval.npz: ground-truth flows, predictions and what THE REFERENCE'S OWN metrics/flow_metric.py
(imported from /root/reference at generation time only, as make_seg_eval_golden.py does) makes of them on the CPU, for
ogc_flow_eval (ogc_amd/csrc/flow_eval.hip) and ogc_amd/metrics/flow_eval.py.  Nothing from the reference is copied: only inputs
and outputs are written.

    python tests/golden/make_flow_eval_golden.py

Per case `<name>_gt` and `<name>_pred` (B, N, 3) float32, `<name>_thresh` (), `<name>_ref` (4,) float64 — eval_flow on the batch:
EPE, AccS, AccR, Outlier — and `<name>_ref_per_sample` (B, 4) — eval_flow sample by sample.

The recipe (`make_case`, which tests/test_flow_eval_gpu.py imports for its larger cases): GT flow = scale * randn with
scale = 5 * thresh; prediction = GT + a unit direction times thresh * 10**U(-1.5, 1.5), so that the error straddles thresh,
2 thresh and 6 thresh and the ratio straddles 0.05 and 0.1; gt[0, 0] = 0, one point with a zero GT flow.  `margin` is the
smallest relative distance, in float64, of any point's error or ratio from any of the five thresholds; a case is re-drawn
(seed + 1000) until it exceeds MARGIN = 1e-5, forty times the 2.4e-7 that four fp32 roundings can move a norm or a ratio:
the counts of a correct fp32 evaluation then equal the float64 counts exactly.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
OUT = os.path.join(HERE, "flow_eval.npz")
MARGIN = 1e-5
EPS = 1e-10
CASES = (("n1", 3, 1, 0.01, 0), ("n63", 2, 63, 0.01, 1), ("n64", 2, 64, 0.01, 2), ("n65", 5, 65, 0.05, 3),
         ("n257", 1, 257, 0.05, 4), ("n2048", 6, 2048, 0.01, 5))     # name, B, N, thresh, first seed


def draw(B, N, thresh, seed):
    rng = np.random.default_rng(seed)
    gt = (5.0 * thresh * rng.standard_normal((B, N, 3))).astype(np.float32)
    direction = rng.standard_normal((B, N, 3))
    direction /= np.linalg.norm(direction, axis=2, keepdims=True)
    magnitude = thresh * 10.0 ** rng.uniform(-1.5, 1.5, (B, N, 1))
    gt[0, 0] = 0.0
    return gt, (gt.astype(np.float64) + direction * magnitude).astype(np.float32)


def truth64(gt, pred, thresh, eps=EPS):
    """float64 evaluation of the fp32 inputs -> (epe (B, N), counts (B, 3) int64, margin)."""
    gt, pred = gt.astype(np.float64), pred.astype(np.float64)
    e = np.linalg.norm(pred - gt, axis=2)
    r = e / (np.linalg.norm(gt, axis=2) + eps)
    counts = np.stack([np.logical_or(e < thresh, r < 0.05).sum(1), np.logical_or(e < 2 * thresh, r < 0.1).sum(1),
                       np.logical_or(e > 6 * thresh, r > 0.1).sum(1)], 1)
    margin = min(min(np.abs(e / t - 1.0).min() for t in (thresh, 2 * thresh, 6 * thresh)),
                 min(np.abs(r / t - 1.0).min() for t in (0.05, 0.1)))
    return e, counts, float(margin)


def make_case(B, N, thresh, seed, tries=64):
    """-> (gt, pred, seed used): the first of seed, seed + 1000, ... whose margin exceeds MARGIN."""
    for k in range(tries):
        gt, pred = draw(B, N, thresh, seed + 1000 * k)
        if truth64(gt, pred, thresh)[2] > MARGIN:
            return gt, pred, seed + 1000 * k
    raise RuntimeError("no draw of (%d, %d, %g) from seed %d keeps the margin" % (B, N, thresh, seed))


def main():
    import torch
    sys.path.insert(0, REF)
    from metrics.flow_metric import eval_flow
    out = {}
    for name, B, N, thresh, seed in CASES:
        gt, pred, used = make_case(B, N, thresh, seed)
        _, counts, margin = truth64(gt, pred, thresh)
        assert margin > MARGIN
        tg, tp = torch.from_numpy(gt), torch.from_numpy(pred)
        ref = np.array(eval_flow(tg, tp, epe_norm_thresh=thresh), np.float64)
        per = np.array([eval_flow(tg[b:b + 1], tp[b:b + 1], epe_norm_thresh=thresh) for b in range(B)], np.float64)
        # the reference's fp32 evaluation counts what float64 counts
        assert np.array_equal(np.rint(per[:, 1:] * N).astype(np.int64), counts), name
        out.update({name + "_gt": gt, name + "_pred": pred, name + "_thresh": np.float64(thresh), name + "_ref": ref,
                    name + "_ref_per_sample": per})
        print("%-6s B=%d N=%d thresh=%g seed=%d margin=%.3g ref=%s" % (name, B, N, thresh, used, margin, ref))
    np.savez(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()

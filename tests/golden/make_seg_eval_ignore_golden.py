"""Writes tests/golden/seg_eval_ignore.npz: labels, soft masks, per-point ignore masks and what THE REFERENCE'S OWN
metrics/seg_metric.py (imported from /root/reference at generation time only, as make_seg_eval_golden.py does) makes of the
RELABELLED sample, for ogc_seg_eval_ignore (ogc_amd/csrc/seg_eval.hip), ogc_amd/metrics/seg_eval.py (ignore=) and
ogc_amd/metrics/seg_metric_ignmask.py.  CPU only.  Nothing from the reference is copied: only inputs and outputs are written.

    python tests/golden/make_seg_eval_ignore_golden.py

The reference ships no ignore-mask metric; DESIGN.md 4h defines one from the code it has: evaluating (segm, mask, ignore, thresh)
gives what eval_segm / accumulate_eval_results / ClusteringMetrics give with threshold T' = max(thresh, 2) on the sample in which
every ignored point carries a fresh label of its own above all real labels.  That is what this script runs, for thresh 0 (`t0`)
and one positive threshold (`tp`).  Per case `<name>_segm` (B, n) int32, `<name>_mask` (B, n, k) float32, `<name>_ignore` (B, n)
int32 and per tag `<name>_<t>_pred_iou / _pred_matched / _confidence / _n_valid / _n_gt / _miou / _ri` as in seg_eval.npz.
The labels stored under ignored points are 0, as the Waymo reader leaves them (nothing may read them).

Asserted, smallest margins recorded in `meta` (those of make_seg_eval_golden.py):
  * every pred_iou is at least 1e-9 from 0.5; the confidences of a case are pairwise at least 1e-5 apart; every ignore ratio is
    exactly 0.5 by construction or at least 1e-9 from it; at least one kept GT object per sample.
And the conditions under which T' = 2 stands for thresh = 0:
  * every real object holds at least 2 non-ignored points;
  * no label below the largest real label is absent.
Two cases cannot meet them at the shapes they are there to cover, and say so in `meta["exceptions"]`:
  * `n1` (one point, not ignored) has nothing ignored, so there is nothing to relabel and no singleton to drop: the reference
    runs on the sample itself with T' = thresh (for any case without an ignored point the two definitions coincide).
  * `n65` (65 points, label 63) cannot hold 64 labels of two points each.  Its absent labels are dropped by T' = 2, while the
    kernel's rule for thresh = 0 (that of ogc_seg_eval) keeps them as zero rows.  Zero rows add nothing to the matched sum of
    the assignment, only to the divisor, so its stored `t0_miou` is the reference's mean times (rows of the reference) /
    (largest label + 1); every other stored number of the case is the reference's own.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
OUT = os.path.join(HERE, "seg_eval_ignore.npz")
sys.path.insert(0, HERE)
from make_seg_eval_golden import random_case, soft_masks  # noqa: E402


def random_ignore(rng, segm, frac):
    """A fraction `frac` of the points, the first two points of every label of every sample left alone."""
    ignore = (rng.random(segm.shape) < frac).astype(np.int32)
    for b in range(segm.shape[0]):
        for g in np.unique(segm[b]):
            ignore[b, np.nonzero(segm[b] == g)[0][:2]] = 0
    return ignore


def with_ignore(rng, B, n, k, labels, sizes, frac, clear=()):
    segm, mask = random_case(rng, B, n, k, labels, sizes=sizes)
    for b in range(B):                      # every label present twice at least
        for j, g in enumerate(labels):
            segm[b, 2 * j:2 * j + 2] = g
    ignore = random_ignore(rng, segm, frac)
    for b in clear:
        ignore[b] = 0
    segm[ignore != 0] = 0
    return segm, mask, ignore


def special_case(rng):
    """n = 1025, k = 15, thresh 50; two samples.  Sample 0, slot by slot (slot 0 is empty):
    1: 30 ignored points + 10 of object 0: ratio 0.75, dropped IN FRONT OF the valid slots (the column shift);
    2: 20 ignored points + 20 of object 0: exactly half, stays valid;
    12: 25 ignored points and nothing else: nothing left of it;
    3: the 40 points of object 3 (only the threshold drops it) + 100 of object 1;
    5: object 4, 60 points of which 15 are ignored: above the threshold in total, below it (45) without them;
    the rest: large objects over two slots each, a tenth of object 5 ignored.  Sample 1 is random."""
    n, k = 1025, 15
    segm = np.zeros((2, n), np.int64)
    hard = np.zeros((2, n), np.int64)
    ignore = np.zeros((2, n), np.int32)
    ignore[0, :30], hard[0, :30] = 1, 1
    segm[0, 30:40], hard[0, 30:40] = 0, 1
    ignore[0, 40:60], hard[0, 40:60] = 1, 2
    segm[0, 60:80], hard[0, 60:80] = 0, 2
    ignore[0, 80:105], hard[0, 80:105] = 1, 12
    segm[0, 105:145], hard[0, 105:145] = 3, 3
    segm[0, 145:245], hard[0, 145:245] = 1, 3
    segm[0, 245:305], hard[0, 245:305] = 4, 5
    ignore[0, 290:305] = 1
    segm[0, 305:500], hard[0, 305:500] = 0, 4
    segm[0, 500:700], hard[0, 500:700] = 1, np.where(rng.random(200) < 0.8, 6, 7)
    segm[0, 700:900], hard[0, 700:900] = 2, np.where(rng.random(200) < 0.7, 8, 14)
    segm[0, 900:], hard[0, 900:] = 5, np.where(rng.random(n - 900) < 0.75, 9, 10)
    ignore[0, 900:] = rng.random(n - 900) < 0.1
    ignore[0, 900:902] = 0
    labels = [0, 1, 2, 3, 4, 5, 6]
    s1, m1 = random_case(rng, 1, n, k, labels, sizes=[300, 200, 30, 150, 100, 60, 185])
    for j, g in enumerate(labels):
        s1[0, 2 * j:2 * j + 2] = g
    segm[1] = s1[0]
    ignore[1] = random_ignore(rng, s1, 0.2)[0]
    mask = soft_masks(rng, hard, k)
    mask[1] = m1[0]
    segm[ignore != 0] = 0
    return segm.astype(np.int32), mask, ignore


def tables(segm, mask, ignore, thresh):
    """One sample in exact integers / float64, straight from the rules of DESIGN.md 4h: (ignore ratios not exactly half, number
    of exact halves, pred_iou of the valid predictions, kept objects, valid predictions, non-ignored sizes, rows)."""
    hard = mask.argmax(1)
    k = mask.shape[1]
    seen = ignore == 0
    tab = np.zeros((64, k), np.int64)
    np.add.at(tab, (segm[seen], hard[seen]), 1)
    ign = np.bincount(hard[~seen], minlength=k)
    gs = tab.sum(1)
    dropped = (gs < thresh) if thresh > 0 else np.zeros(64, bool)
    keep = (gs > 0) & ~dropped
    ps = tab.sum(0) + ign
    ia = ign + tab[dropped].sum(0)
    present = ps > 0
    ratio = ia[present] / ps[present]
    exact_half = 2 * ia[present] == ps[present]
    kept = ps - ia
    valid = present & (kept > 0) & ~(2 * ia > ps)
    iou = (tab[keep][:, valid] / (gs[keep][:, None] + kept[valid][None] - tab[keep][:, valid])).max(0) if keep.any() else np.zeros(0)
    top = int(np.nonzero(gs > 0)[0].max()) + 1 if (gs > 0).any() else 0
    return ratio[~exact_half], int(exact_half.sum()), iou, int(keep.sum()), int(valid.sum()), gs, int((~dropped[:top]).sum())


def relabel(segm, ignore):
    """Every ignored point becomes an object of one point with a label above the sample's real labels."""
    out = segm.astype(np.int64).copy()
    for b in range(segm.shape[0]):
        idx = np.nonzero(ignore[b])[0]
        seen = segm[b][ignore[b] == 0]
        out[b, idx] = (int(seen.max()) + 1 if seen.size else 0) + np.arange(len(idx))
    return out


def main():
    assert os.path.isdir(REF), "the reference tree is only present in the build container"
    os.environ.setdefault("MPLBACKEND", "Agg")
    sys.path.insert(0, REF)
    import torch
    from metrics.seg_metric import ClusteringMetrics, accumulate_eval_results, eval_segm

    builders = {
        "n1": lambda rng: (np.zeros((1, 1), np.int32), np.ones((1, 1, 1), np.float32), np.zeros((1, 1), np.int32), 1),
        "n63": lambda rng: with_ignore(rng, 1, 63, 2, [0, 1, 2], [30, 25, 8], 0.15) + (10,),
        "n65": lambda rng: with_ignore(rng, 2, 65, 64, [0, 5, 17, 63], [30, 20, 4, 11], 0.2) + (8,),
        "n1025": lambda rng: special_case(rng) + (50,),
        "n2048": lambda rng: with_ignore(rng, 3, 2048, 22, list(range(12)),
                                         [400, 300, 250, 40, 200, 30, 180, 160, 20, 150, 140, 178], 0.15, clear=(1,)) + (50,),
    }
    exceptions = {"n1": "nothing ignored: T' = thresh", "n65": "absent labels: t0_miou rescaled to the zero-row rule"}
    cm = ClusteringMetrics()

    def evaluate(name, segm, mask, ignore, thresh_pos):
        B, n, k = mask.shape
        assert segm.shape == ignore.shape == (B, n) and segm.dtype == ignore.dtype == np.int32 and mask.dtype == np.float32
        assert not segm[ignore != 0].any()
        res = {name + "_segm": segm, name + "_mask": mask, name + "_ignore": ignore}
        worst = {"pred_iou_from_half": np.inf, "confidence_gap": np.inf, "ignore_ratio_from_half": np.inf, "exact_half_ratios": 0}
        relab = relabel(segm, ignore)
        ts, tm = torch.from_numpy(relab), torch.from_numpy(mask)
        nothing_ignored = not ignore.any()
        assert nothing_ignored == (name == "n1")
        for tag, thresh in (("t0", 0), ("tp", thresh_pos)):
            t_ref = thresh if nothing_ignored else max(thresh, 2)
            n_valid, n_gt, scale = [], [], []
            for b in range(B):
                ratios, halves, iou, kept_objects, valid, gs, rows = tables(segm[b], mask[b], ignore[b], thresh)
                if kept_objects < 1:
                    return None, None
                present = gs > 0
                if thresh == 0 and not nothing_ignored:
                    if gs[present].min() < 2:
                        return None, None
                    top = int(np.nonzero(present)[0].max()) + 1
                    assert name == "n65" or present[:top].all(), "an absent label below the largest in case %s" % name
                scale.append(int(present.sum()) / rows if thresh == 0 else 1.0)
                pred_iou, _, _, n_gt_b = eval_segm(relab[b], mask[b], ignore_npoint_thresh=t_ref)
                assert len(pred_iou) == valid and n_gt_b == kept_objects
                assert np.allclose(pred_iou, iou, rtol=1e-12, atol=0)
                n_valid.append(len(pred_iou))
                n_gt.append(n_gt_b)
                worst["exact_half_ratios"] += halves
                if len(ratios):
                    worst["ignore_ratio_from_half"] = min(worst["ignore_ratio_from_half"], float(np.abs(ratios - 0.5).min()))
                if len(iou):
                    worst["pred_iou_from_half"] = min(worst["pred_iou_from_half"], float(np.abs(iou - 0.5).min()))
            pred_iou, pred_matched, confidence, n_gt_all = accumulate_eval_results(ts, tm, ignore_npoint_thresh=t_ref)
            assert len(pred_iou) == sum(n_valid) and int(n_gt_all) == sum(n_gt)
            if len(confidence) > 1:
                worst["confidence_gap"] = min(worst["confidence_gap"], float(np.diff(np.sort(confidence.astype(np.float64))).min()))
            clu = cm(tm, ts, t_ref)
            assert all(s == 1.0 for s in scale) or name == "n65"
            pre = "%s_%s_" % (name, tag)
            res[pre + "pred_iou"] = np.asarray(pred_iou, np.float64)
            res[pre + "pred_matched"] = np.asarray(pred_matched, np.float64)
            res[pre + "confidence"] = np.asarray(confidence, np.float64)
            res[pre + "n_valid"] = np.asarray(n_valid, np.int32)
            res[pre + "n_gt"] = np.asarray(n_gt, np.int32)
            res[pre + "miou"] = np.asarray(clu["iou"], np.float64) * np.asarray(scale, np.float64)
            res[pre + "ri"] = np.asarray(clu["ri"], np.float64)
        return res, worst

    out, meta = {}, {"cases": {}, "exceptions": exceptions,
                     "reference": "metrics/seg_metric.py on the relabelled sample (singletons, T' = max(thresh, 2))"}
    margins = {"pred_iou_from_half": np.inf, "confidence_gap": np.inf, "ignore_ratio_from_half": np.inf, "exact_half_ratios": 0}
    for index, (name, builder) in enumerate(builders.items()):
        # the inputs are random: a draw that lands within a margin or misses a condition is drawn again (the draw is recorded)
        for draw in range(200):
            segm, mask, ignore, thresh_pos = builder(np.random.default_rng([20261019, index, draw]))
            res, worst = evaluate(name, segm, mask, ignore, thresh_pos)
            if res is not None and worst["pred_iou_from_half"] >= 1e-9 and worst["confidence_gap"] >= 1e-5 \
                    and worst["ignore_ratio_from_half"] >= 1e-9:
                break
        else:
            raise AssertionError("no draw of case %s keeps the margins" % name)
        out.update(res)
        B, n, k = mask.shape
        meta["cases"][name] = {"B": B, "n": n, "k": k, "thresh": {"t0": 0, "tp": thresh_pos}, "draw": draw,
                               "ignored_points": int((ignore != 0).sum())}
        for key in margins:
            margins[key] = margins[key] + worst[key] if key == "exact_half_ratios" else min(margins[key], worst[key])
    assert margins["pred_iou_from_half"] >= 1e-9, margins
    assert margins["confidence_gap"] >= 1e-5, margins
    assert margins["ignore_ratio_from_half"] >= 1e-9, margins
    assert margins["exact_half_ratios"] >= 2, "the exactly-half slot of case n1025 is gone"
    assert not out["n2048_ignore"][1].any() and out["n2048_ignore"][0].any() and out["n2048_ignore"][2].any()
    # the constructed slots of n1025, sample 0, at the positive threshold
    sizes = tables(out["n1025_segm"][0], out["n1025_mask"][0], out["n1025_ignore"][0], 50)[5]
    assert sizes[3] == 40 and sizes[4] == 45
    meta["smallest_margins"] = margins
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
    print(json.dumps(margins))


if __name__ == "__main__":
    main()

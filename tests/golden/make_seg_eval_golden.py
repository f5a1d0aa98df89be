"""Writes tests/golden/seg_eval.npz: labels, soft masks and what THE REFERENCE'S OWN metrics/seg_metric.py (imported from
/root/reference at generation time only, as make_golden.py does) makes of them, for ogc_seg_eval (ogc_amd/csrc/seg_eval.hip) and
ogc_amd/metrics/seg_eval.py.  CPU only.  Nothing from the reference is copied: only inputs and outputs are written.

    python tests/golden/make_seg_eval_golden.py

Per case `<name>_segm` (B, n) int32 and `<name>_mask` (B, n, k) float32, and for thresh 0 (`t0`) and one positive threshold
(`tp`): `<name>_<t>_pred_iou / _pred_matched / _confidence` (concatenated over the samples, as accumulate_eval_results returns
them), `_n_valid` (B,) and `_n_gt` (B,) per sample (eval_segm sample by sample), `_miou` and `_ri` (B,) from ClusteringMetrics.

The generator asserts what makes equality of the discrete results fair, and records the smallest margins it met in `meta`:
  * every pred_iou is at least 1e-9 from 0.5 (Pred_Matched cannot flip);
  * the confidences of a case are pairwise at least 1e-5 apart (the reference averages in float32: AP's order cannot flip);
  * every ignore ratio is exactly 0.5 by construction (integers a, 2a) or at least 1e-9 from it;
  * at least one kept GT object per sample (the reference raises without one).
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
OUT = os.path.join(HERE, "seg_eval.npz")


def soft_masks(rng, hard, k, bonus=3.0):
    """Soft-max of uniform noise plus `bonus` at the wanted slot: arg-max = hard, values spread over (0, 1)."""
    logits = rng.random(hard.shape + (k,))
    np.put_along_axis(logits, hard[..., None], np.take_along_axis(logits, hard[..., None], -1) + bonus, -1)
    e = np.exp(logits - logits.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


def noisy_prediction(rng, segm, k, slot_of_label, flip=0.15):
    """The slot of each point's GT label, a fraction `flip` of the points moved to a random slot."""
    hard = slot_of_label[segm]
    move = rng.random(segm.shape) < flip
    return np.where(move, rng.integers(0, k, segm.shape), hard)


def random_case(rng, B, n, k, labels, sizes=None):
    labels = np.asarray(labels)
    segm = np.empty((B, n), np.int64)
    for b in range(B):
        p = rng.random(len(labels)) + 0.2 if sizes is None else np.asarray(sizes, float)
        segm[b] = labels[rng.choice(len(labels), size=n, p=p / p.sum())]
        segm[b, rng.integers(0, n)] = labels[0]
    slot_of_label = np.zeros(64, np.int64)
    slot_of_label[labels] = rng.permutation(max(k, len(labels)))[:len(labels)] % k
    hard = noisy_prediction(rng, segm, k, slot_of_label)
    return segm.astype(np.int32), soft_masks(rng, hard, k)


def special_case(rng):
    """n = 1025, k = 15, thresh 50; three samples.
    0: slot 0 empty; slot 1 = 30 points of the ignored object 5 (size 30) + 10 others: ratio 0.75, dropped BEFORE the valid slots
       (the reference's column shift); slot 2 = 20 of the 40 points of the ignored object 7 + 20 points of a kept object: ratio
       exactly 0.5, stays valid.
    1: ties in mask rows (two and three equal maxima, the first wins), slots 0 and 3 empty.
    2: a prediction entirely inside an ignored object (nothing left of it) behind valid ones, label 63 and gaps."""
    n, k = 1025, 15
    segm = np.zeros((3, n), np.int64)
    hard = np.zeros((3, n), np.int64)
    # sample 0
    segm[0, :30], hard[0, :30] = 5, 1
    segm[0, 30:70] = 7
    hard[0, 30:50], hard[0, 50:70] = 2, 3
    segm[0, 70:400], segm[0, 400:800], segm[0, 800:] = 0, 2, 9
    hard[0, 70:80] = 1
    hard[0, 80:100] = 2
    hard[0, 100:400] = 4
    hard[0, 400:800] = np.where(rng.random(400) < 0.8, 6, 3)
    hard[0, 800:] = np.where(rng.random(n - 800) < 0.7, 9, 14)
    # sample 1
    segm[1] = np.repeat([1, 4, 6, 11], [300, 300, 300, 125])
    hard[1] = noisy_prediction(rng, segm[1], k, np.arange(64) % k)
    hard[1] = np.where((hard[1] == 0) | (hard[1] == 3), 5, hard[1])
    # sample 2
    segm[2] = np.repeat([3, 20, 63, 40], [500, 25, 300, 200])
    hard[2] = noisy_prediction(rng, segm[2], k, np.array([(3 * g + 1) % k for g in range(64)]), flip=0.1)
    hard[2] = np.where(hard[2] == 12, 2, hard[2])
    hard[2, 500:525] = 12          # slot 12 lies entirely in the ignored object 20
    mask = soft_masks(rng, hard, k)
    for i in range(0, 200, 7):     # ties in sample 1: the maximum twice, and three times
        top = mask[1, i].max()
        second = (hard[1, i] + 1 + i % 5) % k
        mask[1, i, second] = top
        if i % 2:
            mask[1, i, (second + 3) % k] = top
    return segm.astype(np.int32), mask


def tables(segm, mask, thresh):
    """Margins of one sample in exact integers / float64: (ignore ratios, pred_iou of the valid predictions, kept objects)."""
    hard = mask.argmax(1)
    k = mask.shape[1]
    tab = np.zeros((64, k), np.int64)
    np.add.at(tab, (segm, hard), 1)
    gs, ps = tab.sum(1), tab.sum(0)
    ign = (gs > 0) & (gs < thresh)
    keep = (gs > 0) & ~ign
    ia = tab[ign].sum(0)
    present = ps > 0
    ratio = ia[present] / ps[present]
    exact_half = 2 * ia[present] == ps[present]
    kept = ps - ia
    valid = present & (kept > 0) & ~(2 * ia > ps)
    iou = (tab[keep][:, valid] / (gs[keep][:, None] + kept[valid][None] - tab[keep][:, valid])).max(0)
    return ratio[~exact_half], int(exact_half.sum()), iou, int(keep.sum()), int(valid.sum())


def main():
    assert os.path.isdir(REF), "the reference tree is only present in the build container"
    os.environ.setdefault("MPLBACKEND", "Agg")
    sys.path.insert(0, REF)
    import torch
    from metrics.seg_metric import ClusteringMetrics, accumulate_eval_results, eval_segm

    builders = {
        "n1": lambda rng: (np.zeros((1, 1), np.int32), np.ones((1, 1, 1), np.float32), 1),
        "n63": lambda rng: random_case(rng, 1, 63, 2, [0, 1, 2], sizes=[30, 25, 8]) + (12,),
        "batch5": lambda rng: random_case(rng, 5, 64, 15, [0, 2, 3, 7, 10, 21]) + (6,),
        "n65": lambda rng: random_case(rng, 2, 65, 64, [0, 5, 17, 63], sizes=[30, 20, 4, 11]) + (8,),
        "n1023": lambda rng: random_case(rng, 1, 1023, 33, [0, 1, 2, 3, 4, 8, 9, 10, 30, 62, 63],
                                         sizes=[200, 150, 20, 100, 30, 120, 90, 10, 140, 60, 100]) + (50,),
        "special": lambda rng: special_case(rng) + (50,),
        "n2048": lambda rng: random_case(rng, 1, 2048, 15, list(range(12)),
                                         sizes=[400, 300, 250, 40, 200, 30, 180, 160, 20, 150, 140, 178]) + (50,),
    }
    cm = ClusteringMetrics()

    def evaluate(name, segm, mask, thresh_pos):
        """The reference's results of one case and the smallest margins met in it."""
        B, n, k = mask.shape
        assert segm.shape == (B, n) and segm.dtype == np.int32 and mask.dtype == np.float32
        res = {name + "_segm": segm, name + "_mask": mask}
        worst = {"pred_iou_from_half": np.inf, "confidence_gap": np.inf, "ignore_ratio_from_half": np.inf, "exact_half_ratios": 0}
        ts, tm = torch.from_numpy(segm.astype(np.int64)), torch.from_numpy(mask)
        for tag, thresh in (("t0", 0), ("tp", thresh_pos)):
            n_valid, n_gt = [], []
            for b in range(B):
                ratios, halves, iou, kept_objects, valid = tables(segm[b], mask[b], thresh)
                if kept_objects < 1:
                    return None, None
                pred_iou, _, _, n_gt_b = eval_segm(segm[b], mask[b], ignore_npoint_thresh=thresh)
                assert len(pred_iou) == valid and n_gt_b == kept_objects
                assert np.allclose(pred_iou, iou, rtol=1e-12, atol=0)
                n_valid.append(len(pred_iou))
                n_gt.append(n_gt_b)
                worst["exact_half_ratios"] += halves
                if len(ratios):
                    worst["ignore_ratio_from_half"] = min(worst["ignore_ratio_from_half"], float(np.abs(ratios - 0.5).min()))
                if len(iou):
                    worst["pred_iou_from_half"] = min(worst["pred_iou_from_half"], float(np.abs(iou - 0.5).min()))
            pred_iou, pred_matched, confidence, n_gt_all = accumulate_eval_results(ts, tm, ignore_npoint_thresh=thresh)
            assert len(pred_iou) == sum(n_valid) and int(n_gt_all) == sum(n_gt)
            if len(confidence) > 1:
                worst["confidence_gap"] = min(worst["confidence_gap"], float(np.diff(np.sort(confidence.astype(np.float64))).min()))
            clu = cm(tm, ts, thresh)
            pre = "%s_%s_" % (name, tag)
            res[pre + "pred_iou"] = np.asarray(pred_iou, np.float64)
            res[pre + "pred_matched"] = np.asarray(pred_matched, np.float64)
            res[pre + "confidence"] = np.asarray(confidence, np.float64)
            res[pre + "n_valid"] = np.asarray(n_valid, np.int32)
            res[pre + "n_gt"] = np.asarray(n_gt, np.int32)
            res[pre + "miou"] = np.asarray(clu["iou"], np.float64)
            res[pre + "ri"] = np.asarray(clu["ri"], np.float64)
        return res, worst

    out, meta = {}, {"cases": {}, "reference": "metrics/seg_metric.py: accumulate_eval_results, eval_segm, ClusteringMetrics"}
    margins = {"pred_iou_from_half": np.inf, "confidence_gap": np.inf, "ignore_ratio_from_half": np.inf, "exact_half_ratios": 0}
    for index, (name, builder) in enumerate(builders.items()):
        # the inputs are random: a draw that lands within a margin is drawn again (the draw taken is recorded)
        for draw in range(200):
            segm, mask, thresh_pos = builder(np.random.default_rng([20260219, index, draw]))
            res, worst = evaluate(name, segm, mask, thresh_pos)
            if res is not None and worst["pred_iou_from_half"] >= 1e-9 and worst["confidence_gap"] >= 1e-5 \
                    and worst["ignore_ratio_from_half"] >= 1e-9:
                break
        else:
            raise AssertionError("no draw of case %s keeps the margins" % name)
        out.update(res)
        B, n, k = mask.shape
        meta["cases"][name] = {"B": B, "n": n, "k": k, "thresh": {"t0": 0, "tp": thresh_pos}, "draw": draw}
        for key in margins:
            margins[key] = margins[key] + worst[key] if key == "exact_half_ratios" else min(margins[key], worst[key])
    assert margins["pred_iou_from_half"] >= 1e-9, margins
    assert margins["confidence_gap"] >= 1e-5, margins
    assert margins["ignore_ratio_from_half"] >= 1e-9, margins
    assert margins["exact_half_ratios"] >= 1, "the exactly-half prediction of case special is gone"
    meta["smallest_margins"] = margins
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
    print(json.dumps(margins))


if __name__ == "__main__":
    main()

"""Instance-segmentation metrics with a per-point ignore mask: the module the reference's test_seg_waymo.py:11 imports
(`metrics.seg_metric_ignmask`) and its tree does not hold.  THE SEMANTICS ARE THIS PACKAGE'S DEFINITION, derived
from what the reference does with the points of GT objects below `ignore_npoint_thresh` (metrics/seg_metric.py:61-79 and
:204-214, :226-228, :238-239), because an ignored point is a point of such an object:

  evaluating (segm, mask, ignore, thresh) gives what the reference's eval_segm / ClusteringMetrics give with threshold
  max(thresh, 2) on the sample in which every ignored point carries a fresh label of its own, above all real labels.

Written here directly as rules on one table, tab[g][p] = non-ignored points with label g and arg-max slot p, and one vector,
ign[p] = ignored points of slot p (no relabelling happens):

  * the size of a GT object is its number of non-ignored points; it is dropped when thresh > 0 and size < thresh; the labels of
    ignored points are never read;
  * the size of a slot is sum_g tab + ign, its ignored area ign + the points of dropped objects; a prediction is invalid when
    strictly more than half of it is ignored area or nothing else is left of it;
  * IoU = inter / (object size + kept slot size - inter), maximum over the kept objects; n_gt = kept objects;
  * the confidence of the j-th valid slot is its mask column averaged over ALL points (ignored ones included) of the j-th
    present slot: the reference's column shift (seg_metric.py:53, :78, :84);
  * mean IoU: the float32 score m / ((a_g + b_p - m) + 1e-8) of the rows g <= largest label that are not dropped, zero-padded
    to square, under the best assignment, divided by the number of those rows (absent labels are zero rows when thresh is 0);
  * Rand index over the pairs of non-ignored points of objects that are not dropped.

This is the numpy path: it serves the CPU, and ogc_amd.metrics.seg_eval falls back to it for a sample whose labels do not fit
the kernel's table.  The reference's interface has threshold 0 (the Waymo reader folds its threshold into the mask); the
`ignore_npoint_thresh` keyword is this package's addition.  On the GPU use ogc_amd.metrics.seg_eval.accumulate_seg_eval(ignore=).
"""
import numpy as np

from .seg_metric import calculate_AP, calculate_PQ_F1  # noqa: F401  (the reference's module has both)


def _numpy(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _tables(segm, mask, ignore, thresh):
    """One sample: segm (n,), mask (n, k), ignore (n,) -> hard, tab (L, k), ign (k,), object sizes, dropped (L,) — L = largest
    non-ignored label + 1 (0 when every point is ignored)."""
    n, k = mask.shape
    if segm.shape != (n,) or ignore.shape != (n,):
        raise ValueError("segm and ignore must be (n,) for a mask (n, k), got %s, %s and %s" % (segm.shape, ignore.shape, mask.shape))
    hard = np.argmax(mask, axis=1)
    seen = ignore == 0
    labels = segm[seen].astype(np.int64)
    if labels.size and labels.min() < 0:
        raise ValueError("a point that is not ignored holds a negative GT label")
    L = int(labels.max()) + 1 if labels.size else 0
    tab = np.bincount(labels * k + hard[seen], minlength=L * k).reshape(L, k).astype(np.int64)
    ign = np.bincount(hard[~seen], minlength=k).astype(np.int64)
    sizes = tab.sum(1)
    dropped = sizes < thresh if thresh > 0 else np.zeros(L, bool)
    return hard, tab, ign, sizes, dropped


def eval_segm(segm, mask, ignore, ignore_npoint_thresh=0):
    """One sample -> pred_iou, pred_matched, confidence (one entry per valid prediction, slot order), n_gt_inst."""
    segm, mask, ignore = _numpy(segm), _numpy(mask), _numpy(ignore)
    hard, tab, ign, sizes, dropped = _tables(segm, mask, ignore, int(ignore_npoint_thresh))
    keep = (sizes > 0) & ~dropped
    psize = tab.sum(0) + ign
    ignored_area = ign + tab[dropped].sum(0)
    kept = psize - ignored_area
    valid = (psize > 0) & (kept > 0) & ~(2 * ignored_area > psize)
    present = np.nonzero(psize > 0)[0]
    confidence = np.array([np.mean(mask[hard == present[c], j], dtype=np.float64) for c, j in enumerate(np.nonzero(valid)[0])],
                          dtype=np.float64)
    inter = tab[keep][:, valid].astype(np.float64)
    union = sizes[keep][:, None] + kept[valid][None, :] - inter
    pred_iou = (inter / union).max(axis=0) if inter.shape[0] else np.zeros(int(valid.sum()))
    return pred_iou, (pred_iou >= 0.5).astype(float), confidence, int(keep.sum())


def accumulate_eval_results(segm, mask, ignore, ignore_npoint_thresh=0):
    """segm (B, N), mask (B, N, K), ignore (B, N), non-zero = ignored (tensors or arrays) -> Pred_IoU, Pred_Matched, Confidence
    over all valid predictions of the batch (sample-major, slot order) and N_GT_Inst."""
    segm, mask, ignore = _numpy(segm), _numpy(mask), _numpy(ignore)
    parts = [eval_segm(segm[b], mask[b], ignore[b], ignore_npoint_thresh) for b in range(segm.shape[0])]
    cat = [np.concatenate([p[i] for p in parts]) if parts else np.zeros(0) for i in range(3)]
    return cat[0], cat[1], cat[2], int(sum(p[3] for p in parts))


class ClusteringMetrics:
    """``forward(mask, segm, ignore)`` -> {'iou': [per sample], 'ri': [per sample]}: mean IoU under the best one-to-one matching
    and Rand index, ignored points left out of both.  A sample with no row left has 'iou' NaN, one with no point left 'ri' NaN."""
    IOU = 1
    RI = 2

    def __init__(self, spec=None):
        self.spec = [self.IOU, self.RI] if spec is None else spec

    def forward(self, mask, segm, ignore, ignore_npoint_thresh=0):
        from scipy.optimize import linear_sum_assignment
        mask, segm, ignore = _numpy(mask), _numpy(segm), _numpy(ignore)
        n_batch, k = mask.shape[0], mask.shape[-1]
        mask, segm, ignore = mask.reshape(n_batch, -1, k), segm.reshape(n_batch, -1), ignore.reshape(n_batch, -1)
        ious, ris = [], []
        for b in range(n_batch):
            _, tab, _, sizes, dropped = _tables(segm[b], mask[b], ignore[b], int(ignore_npoint_thresh))
            tab = tab[~dropped]                                                  # absent labels stay as zero rows when thresh is 0
            a, c = tab.sum(1), tab.sum(0)                                        # c: the kept size of every slot
            if self.IOU in self.spec:
                rows = tab.shape[0]
                score = np.zeros((rows, max(rows, k)), np.float32)
                m = tab.astype(np.float32)
                score[:, :k] = m / ((a.astype(np.float32)[:, None] + c.astype(np.float32)[None, :] - m) + np.float32(1e-8))
                r, col = linear_sum_assignment(score, maximize=True)
                ious.append(float(np.mean(score[r, col])) if rows else float("nan"))
            if self.RI in self.spec:
                n_v = int(tab.sum())
                agree = n_v * n_v - sum(int(x) ** 2 for x in a) - sum(int(x) ** 2 for x in c) + 2 * sum(int(x) ** 2 for x in tab.reshape(-1))
                ris.append(agree / (n_v * n_v) if n_v else float("nan"))
        out = {}
        if self.IOU in self.spec:
            out["iou"] = ious
        if self.RI in self.spec:
            out["ri"] = ris
        return out

    __call__ = forward

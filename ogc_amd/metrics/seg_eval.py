"""Segmentation evaluation of a batch on the device (reference: metrics/seg_metric.py:8-93 and :167-243, test_seg.py's loop).

`seg_eval_batch` is the operator: one launch of ogc_seg_eval (csrc/seg_eval.hip: arg-max, the (GT label x slot) table, the AP
table, the float32 IoU matrix and the Rand index of every sample), one launch of ogc_lsap_maximize on the zero-padded 64 x 64
IoU matrices, and a few (B, 64)-sized tensor operations for the per-sample mean IoU — all on the current stream, nothing read
back, so it can be captured in a torch.cuda.graph.  `accumulate_seg_eval` adds the ONE device->host copy of a packed table and
returns what `accumulate_eval_results` and `ClusteringMetrics` of metrics/seg_metric.py return together.  There is no CPU path.

With `ignore=` (a per-point mask, non-zero = ignored) both go through ogc_seg_eval_ignore instead: the metric of
metrics/seg_metric_ignmask.py, which is this package's definition (the reference ships none).  `ignore=None` is the
path above, call for call.
"""
from collections import namedtuple

import numpy as np
import torch

from .. import pointnet2_cuda as _native
from . import seg_metric_ignmask as _ign
from .seg_metric import ClusteringMetrics, accumulate_eval_results

MAX_LABELS = 64     # OGC_SEG_EVAL_MAX_LABELS of include/ogc_ops.h: table rows, and the side of the score matrix
STATUS_LABEL_TOO_LARGE = 1
STATUS_LABEL_NEGATIVE = 2

SegEval = namedtuple("SegEval", "hard counts pred_iou confidence valid n_gt score rows ri status col miou ignored")


def seg_eval_batch(segm, mask, ignore_npoint_thresh=0, ignore=None):
    """segm (B, n) integer CUDA tensor of GT labels in [0, 64), mask (B, n, k) fp32 CUDA tensor, 1 <= k <= 64 -> SegEval of
    device tensors: hard (B, n) i32, counts (B, 64, k) i32, pred_iou / confidence (B, k) f64, valid (B, k) bool, n_gt (B,) i32,
    score (B, 64, 64) f32, rows (B,) i32, ri (B,) f64, status (B,) i32 (0 ok, bit 0 a label >= 64, bit 1 a negative label:
    every other output of such a sample is zero), col (B, 64) i32 the assignment, miou (B,) f64 (NaN where rows is 0), ignored
    (B, k) i32 (zeros without `ignore`).  ignore: None, or a (B, n) CUDA tensor of an integer or bool dtype, non-zero = the point
    is ignored: its label is not read, `counts` leaves it out and `ignored` counts it per slot (ogc_seg_eval_ignore).
    No synchronisation."""
    for t, name in ((segm, "segm"), (mask, "mask")):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor" % name)
    if mask.dtype != torch.float32:
        raise TypeError("mask must be float32, got %s" % mask.dtype)
    if segm.dtype.is_floating_point or segm.dtype.is_complex or segm.dtype == torch.bool:
        raise TypeError("segm must have an integer dtype, got %s" % segm.dtype)
    if mask.device.type != "cuda" or segm.device.type != "cuda":
        raise RuntimeError("segm and mask must be CUDA tensors (HIP device); ogc_amd has no CPU path")
    if segm.device != mask.device:
        raise RuntimeError("segm and mask must be on one device, got %s and %s" % (segm.device, mask.device))
    if mask.dim() != 3 or segm.dim() != 2 or tuple(segm.shape) != tuple(mask.shape[:2]):
        raise ValueError("segm must be (B, n) and mask (B, n, k), got %s and %s" % (tuple(segm.shape), tuple(mask.shape)))
    if int(ignore_npoint_thresh) < 0:
        raise ValueError("ignore_npoint_thresh must be >= 0, got %s" % (ignore_npoint_thresh,))
    if ignore is not None:
        if not isinstance(ignore, torch.Tensor):
            raise TypeError("ignore must be a torch.Tensor or None")
        if ignore.dtype.is_floating_point or ignore.dtype.is_complex:
            raise TypeError("ignore must have an integer or bool dtype, got %s" % ignore.dtype)
        if ignore.device != mask.device:
            raise RuntimeError("ignore must be on the device of mask, got %s and %s" % (ignore.device, mask.device))
        if tuple(ignore.shape) != tuple(segm.shape):
            raise ValueError("ignore must be (B, n) as segm %s, got %s" % (tuple(segm.shape), tuple(ignore.shape)))
    B, n, k = mask.shape
    dev = mask.device
    if segm.dtype != torch.int32:
        # labels beyond int32 must keep their sign and their "too large" for the kernel's range check
        segm = segm.clamp(-1, MAX_LABELS).to(torch.int32)
    i32 = dict(dtype=torch.int32, device=dev)
    f64 = dict(dtype=torch.float64, device=dev)
    hard = torch.empty(B, n, **i32)
    counts = torch.empty(B, MAX_LABELS, k, **i32)
    pred_iou, confidence = torch.empty(B, k, **f64), torch.empty(B, k, **f64)
    valid, n_gt = torch.empty(B, k, **i32), torch.empty(B, **i32)
    score = torch.empty(B, MAX_LABELS, MAX_LABELS, dtype=torch.float32, device=dev)
    rows, ri, status = torch.empty(B, **i32), torch.empty(B, **f64), torch.empty(B, **i32)
    col = torch.empty(B, MAX_LABELS, **i32)
    if ignore is None:
        ignored = torch.zeros(B, k, **i32)
        _native.seg_eval_wrapper(B, n, k, segm.contiguous(), mask.detach().contiguous(), int(ignore_npoint_thresh), hard, counts,
                                 pred_iou, confidence, valid, n_gt, score, rows, ri, status)
    else:
        ignored = torch.empty(B, k, **i32)
        _native.seg_eval_ignore_wrapper(B, n, k, segm.contiguous(), mask.detach().contiguous(),
                                        (ignore != 0).to(torch.int32).contiguous(), int(ignore_npoint_thresh), hard, counts,
                                        ignored, pred_iou, confidence, valid, n_gt, score, rows, ri, status)
    _native.lsap_maximize_wrapper(B, MAX_LABELS, score, col)
    # rows that are not kept are zero rows of `score`: the sum over all 64 rows is the sum over the kept ones
    matched = torch.gather(score, 2, col.long().unsqueeze(2)).squeeze(2).to(torch.float64)
    miou = matched.sum(dim=1) / rows.to(torch.float64)
    miou = torch.where(rows > 0, miou, torch.full_like(miou, float("nan")))
    return SegEval(hard, counts, pred_iou, confidence, valid.bool(), n_gt, score, rows, ri, status, col, miou, ignored)


def accumulate_seg_eval(segm, mask, ignore_npoint_thresh=0, result=None, ignore=None):
    """-> (Pred_IoU, Pred_Matched, Confidence, N_GT_Inst, miou_per_sample, ri_per_sample): the first four as
    `accumulate_eval_results` (valid predictions only, sample-major, slot order), the last two numpy arrays (B,) as the 'iou' and
    'ri' lists of `ClusteringMetrics`.  One device->host copy.  A sample with a label >= 64 goes through the tensor path of
    metrics/seg_metric.py on its own; a negative label raises ValueError.  `result`: what seg_eval_batch returned for the same
    arguments, for a caller that also needs its device tensors (test_seg.py saves `hard`).  `ignore` as in seg_eval_batch; with
    it the fallback of a sample is metrics/seg_metric_ignmask.py, and only labels of points that are not ignored count."""
    res = seg_eval_batch(segm, mask, ignore_npoint_thresh, ignore) if result is None else result
    B, k = res.pred_iou.shape
    table = torch.cat([res.pred_iou, res.confidence, res.valid.to(torch.float64), res.n_gt.to(torch.float64).unsqueeze(1),
                       res.miou.unsqueeze(1), res.ri.unsqueeze(1), res.status.to(torch.float64).unsqueeze(1)],
                      dim=1).cpu().numpy()                                       # (B, 3k + 4): the only copy to the host
    status = table[:, 3 * k + 3].astype(np.int64)
    negative = np.nonzero(status & STATUS_LABEL_NEGATIVE)[0]
    if negative.size:
        raise ValueError("sample %d of the batch holds a negative GT label" % int(negative[0]))
    ious, confs, n_gt = [], [], 0
    miou, ri = table[:, 3 * k + 1].copy(), table[:, 3 * k + 2].copy()
    for b in range(B):
        if status[b] & STATUS_LABEL_TOO_LARGE and ignore is not None:
            iou_b, _, conf_b, n_b = _ign.accumulate_eval_results(segm[b:b + 1], mask[b:b + 1], ignore[b:b + 1], ignore_npoint_thresh)
            cm = _ign.ClusteringMetrics()(mask[b:b + 1], segm[b:b + 1], ignore[b:b + 1], ignore_npoint_thresh)
            miou[b], ri[b] = cm["iou"][0], cm["ri"][0]
        elif status[b] & STATUS_LABEL_TOO_LARGE:
            iou_b, _, conf_b, n_b = accumulate_eval_results(segm[b:b + 1], mask[b:b + 1], ignore_npoint_thresh)
            cm = ClusteringMetrics()(mask[b:b + 1], segm[b:b + 1], ignore_npoint_thresh)
            miou[b], ri[b] = cm["iou"][0], cm["ri"][0]
        else:
            keep = table[b, 2 * k:3 * k] > 0
            iou_b, conf_b, n_b = table[b, :k][keep], table[b, k:2 * k][keep], int(round(table[b, 3 * k]))
        ious.append(iou_b)
        confs.append(conf_b)
        n_gt += n_b
    iou = np.concatenate(ious) if ious else np.zeros(0)
    conf = np.concatenate(confs) if confs else np.zeros(0)
    return iou, (iou >= 0.5).astype(float), conf, n_gt, miou, ri

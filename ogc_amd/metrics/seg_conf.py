"""Confidences of PREDICTED segmentations on the device, for training on them (datasets.py: `load_prediction`,
`load_confidence`).  The reference reads <id>/conf.npy (datasets/dataset_kittidet.py:63-70) and ships no writer of it; the value
is the one its evaluation gives a prediction (metrics/seg_metric.py:81-85): the mean of an object's own mask column over the
object's own points — here without the validity filter of eval_segm, which needs ground truth.

`slot_confidence_batch` is the operator: one launch of ogc_slot_confidence (csrc/seg_conf.hip) on the current stream, nothing
read back, so it can be captured in a torch.cuda.graph.  `pseudo_label_confidences` adds the ONE device->host copy and returns
what `_save_predsegm(..., conf=...)` writes.  There is no CPU path.
"""
from collections import namedtuple

import torch

from .. import pointnet2_cuda as _native

MAX_SLOTS = 64  # OGC_SLOT_CONF_MAX_K
SlotConfidence = namedtuple("SlotConfidence", "hard slots sizes conf n_object")


def slot_confidence_batch(mask):
    """mask (B, N, K) fp32 CUDA tensor of soft masks -> SlotConfidence(hard (B, N) i32 the arg-max labels, slots (B, K) i32 the
    slots that own at least one point in ascending order (-1 behind them), sizes (B, K) i32 their points, conf (B, K) f32 the
    mean of mask[b, p, slot] over the slot's own points, n_object (B,) i32).  Entry j of slots / sizes / conf belongs to the
    label j that compress_label_id gives the saved arg-max labels.  No synchronisation."""
    if not isinstance(mask, torch.Tensor):
        raise TypeError("mask must be a torch.Tensor")
    if mask.dtype != torch.float32:
        raise TypeError("mask must be float32, got %s" % mask.dtype)
    if mask.device.type != "cuda":
        raise RuntimeError("mask must be a CUDA tensor (HIP device); ogc_amd has no CPU path")
    if mask.dim() != 3:
        raise ValueError("mask must be (B, N, K), got %s" % (tuple(mask.shape),))
    B, N, K = mask.shape
    if not 1 <= K <= MAX_SLOTS:
        raise ValueError("mask has %d slots, ogc_slot_confidence takes 1 to %d" % (K, MAX_SLOTS))
    dev = mask.device
    hard = torch.empty(B, N, dtype=torch.int32, device=dev)
    slots = torch.empty(B, K, dtype=torch.int32, device=dev)
    sizes = torch.empty(B, K, dtype=torch.int32, device=dev)
    conf = torch.empty(B, K, dtype=torch.float32, device=dev)
    n_object = torch.empty(B, dtype=torch.int32, device=dev)
    _native.slot_confidence_wrapper(B, N, K, mask.detach().contiguous(), hard, slots, sizes, conf, n_object)
    return SlotConfidence(hard, slots, sizes, conf, n_object)


def pseudo_label_confidences(mask):
    """-> a list of B float32 numpy arrays, the b-th of length n_object[b]: the confidence of every object of sample b's arg-max
    segmentation, in the order of its compressed labels.  One device->host copy."""
    return confidences_to_host(slot_confidence_batch(mask))


def confidences_to_host(res):
    """The list pseudo_label_confidences returns, from a SlotConfidence already computed (a caller that also wants `hard`)."""
    K = res.conf.shape[1]
    # n_object <= K <= 64 is exact in float32, so one (B, K + 1) table goes over
    table = torch.cat([res.conf, res.n_object.to(torch.float32).unsqueeze(1)], dim=1).cpu().numpy()   # the only copy to the host
    return [table[b, :int(table[b, K])].copy() for b in range(table.shape[0])]

"""Scene-flow evaluation of a batch on the device (reference: metrics/flow_metric.py:4-25, the loops of test_flow.py and
test_flow_kittisf_benchmark.py).

`flow_eval_batch` is the operator: one launch of ogc_flow_eval (csrc/flow_eval.hip) gives, per sample, the fp64 sum of the
end-point errors and the integer numbers of strict-accurate, relaxed-accurate and outlier points — on the current stream,
nothing read back, so it can be captured in a torch.cuda.graph.  `eval_flow_device` adds the ONE device->host copy of a
(B, 4) table and returns the reference's four floats for the batch together with the per-sample table.  There is no CPU path;
`metrics/flow_metric.py` (the tensor path the KITTI-SF and Waymo drivers use) is unchanged.
"""
from collections import namedtuple

import torch

from .. import pointnet2_cuda as _native

FlowEval = namedtuple("FlowEval", "epe_sum counts n_point")


def flow_eval_batch(gt_flow, flow_pred, epe_norm_thresh=0.05, eps=1e-10):
    """gt_flow, flow_pred (B, N, 3) fp32 CUDA tensors -> FlowEval(epe_sum (B,) f64, counts (B, 3) i32, n_point = N): per sample
    the sum of the end-point errors and the strict-accurate / relaxed-accurate / outlier points.  No synchronisation."""
    for t, name in ((gt_flow, "gt_flow"), (flow_pred, "flow_pred")):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor" % name)
        if t.dtype != torch.float32:
            raise TypeError("%s must be float32, got %s" % (name, t.dtype))
    if gt_flow.device.type != "cuda" or flow_pred.device.type != "cuda":
        raise RuntimeError("gt_flow and flow_pred must be CUDA tensors (HIP device); ogc_amd has no CPU path")
    if gt_flow.device != flow_pred.device:
        raise RuntimeError("gt_flow and flow_pred must be on one device, got %s and %s" % (gt_flow.device, flow_pred.device))
    if gt_flow.dim() != 3 or gt_flow.shape[2] != 3 or tuple(gt_flow.shape) != tuple(flow_pred.shape):
        raise ValueError("gt_flow and flow_pred must both be (B, N, 3), got %s and %s"
                         % (tuple(gt_flow.shape), tuple(flow_pred.shape)))
    B, N, _ = gt_flow.shape
    epe_sum = torch.empty(B, dtype=torch.float64, device=gt_flow.device)
    counts = torch.empty(B, 3, dtype=torch.int32, device=gt_flow.device)
    _native.flow_eval_wrapper(B, N, gt_flow.detach().contiguous(), flow_pred.detach().contiguous(), float(epe_norm_thresh),
                              float(eps), epe_sum, counts)
    return FlowEval(epe_sum, counts, N)


def eval_flow_device(gt_flow, flow_pred, epe_norm_thresh=0.05, eps=1e-10):
    """-> ((EPE3D, Acc3DS, Acc3DR, Outliers3D), per_sample): the four Python floats of the reference's `eval_flow` for the whole
    batch — each a total over all samples divided by B * N in float64 — and the (B, 4) float64 numpy table of the same four
    quantities per sample.  One device->host copy."""
    res = flow_eval_batch(gt_flow, flow_pred, epe_norm_thresh, eps)
    table = torch.cat([res.epe_sum.unsqueeze(1), res.counts.to(torch.float64)], dim=1).cpu().numpy()   # the only copy to the host
    B = table.shape[0]
    per_sample = table / float(res.n_point)
    total = table.sum(axis=0) / float(B * res.n_point) if B else table.sum(axis=0) * float("nan")
    return tuple(float(v) for v in total), per_sample

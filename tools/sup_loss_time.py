"""Time of forward + backward of SupervisedMaskLoss (ogc_amd/losses/seg_loss_sup.py) on the GPU, at two shapes:

  kittisf   B = 16 clouds x n = 8192 points, k = 15 slots, BCE, weights [2.0, 0]  (config/seg/kittisf/kittisf_sup.yaml)
  ogcdr     B = 32 x n = 2048, k = 8, BCE, weights [2.0, 0]                        (config/seg/ogcdr/ogcdr_sup.yaml)

  kernel path   ogc_sup_match_cost + ogc_lsap_maximize + ogc_sup_mask_loss_fwd, backward ogc_sup_mask_loss_bwd
  tensor path   the package's restatement of the reference's formula in framework operators (pinned to the reference on the
                CPU by tests/test_sup_loss_cpu.py), on the same GPU tensors — the kernels switched off

Inputs: masks = soft-max of random logits peaked on the slot of the point's object, one-hot labels of six (kittisf) or four
(ogcdr) objects, valid with every eighth point out.  Both paths run with sync=True (they end in the copy of the three monitored
scalars, as the reference's `.item()` calls do); wall time per call with a device synchronisation before and after, the two
paths alternating call by call in one process, after warm-up and after a check that loss and gradient agree.  The kernel path
is also timed with sync=False (as the trainer calls it), and its four launches one by one with HIP events.  Needs the GPU.

    python tools/sup_loss_time.py [--calls 100] [--warmup 10] [--out profiles/sup_loss_time.txt]"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ogc_amd import pointnet2_cuda as nat  # noqa: E402
from ogc_amd.losses import seg_loss_sup as S  # noqa: E402

SHAPES = (("kittisf", 16, 8192, 15, 6), ("ogcdr", 32, 2048, 8, 4))
WEIGHTS = [2.0, 0]


def summary(ms):
    ms = sorted(ms)
    return "median %.4f ms, min %.4f, p90 %.4f over %d calls" % (statistics.median(ms), ms[0], ms[int(0.9 * len(ms))], len(ms))


def inputs(B, n, k, n_object):
    g = torch.Generator().manual_seed(0)
    segm = torch.randint(0, n_object, (B, n), generator=g)
    gt = torch.eye(k)[segm]
    slot = torch.stack([torch.randperm(k, generator=g) for _ in range(B)])           # object j is predicted in slot slot[b, j]
    logits = 4.0 * torch.eye(k)[torch.gather(slot, 1, segm)] + torch.rand(B, n, k, generator=g)
    valid = torch.ones(B, n)
    valid[:, 7::8] = 0.0
    return torch.softmax(logits, 2).cuda(), gt.cuda(), valid.cuda()


def measure(name, B, n, k, n_object, calls, warmup):
    mask, gt, valid = inputs(B, n, k, n_object)
    crit = S.SupervisedMaskLoss(S.CrossEntropyLoss(), S.DiceLoss(), WEIGHTS)
    assert crit.kernels_apply(mask, gt, valid)

    def run(kernels, sync=True):
        S.KERNELS = kernels
        m = mask.detach().requires_grad_(True)
        loss, loss_dict = crit(m, gt, valid, sync=sync)
        loss.backward()
        return loss, loss_dict, m.grad

    try:
        (la, da, ga), (lb, db, gb) = run(True), run(False)
        assert abs(float(la) - float(lb)) <= 1e-5 * abs(float(lb)), (float(la), float(lb))
        assert float((ga - gb).abs().max()) <= 1e-5 * float(gb.abs().max())
        for _ in range(warmup):
            run(True), run(False), run(True, sync=False)
        wall = {"kernel": [], "tensor": [], "kernel_nosync": []}
        for _ in range(calls):
            for key, kernels, sync in (("kernel", True, True), ("tensor", False, True), ("kernel_nosync", True, False)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(kernels, sync)
                torch.cuda.synchronize()
                wall[key].append((time.perf_counter() - t0) * 1e3)
    finally:
        S.KERNELS = True

    # the launches one by one, on buffers allocated once
    ws = nat.sup_loss_workspace(B, n, k, mask.device)
    cost_ce, cost_dice = torch.empty(B, k, k, device="cuda"), torch.empty(B, k, k, device="cuda")
    cols = torch.empty(B, k, dtype=torch.int32, device="cuda")
    sums, terms = torch.empty(B, k, 4, dtype=torch.float64, device="cuda"), torch.empty(2, device="cuda")
    grad, gout = torch.empty_like(mask), torch.ones(1, device="cuda")
    neg = torch.empty(B, k, k, device="cuda")
    steps = (("ogc_sup_match_cost", lambda: nat.sup_match_cost_wrapper(B, n, k, mask, gt, valid, None, ws, cost_ce, cost_dice)),
             ("ogc_lsap_maximize", lambda: nat.lsap_maximize_wrapper(B, k, neg, cols)),
             ("ogc_sup_mask_loss_fwd", lambda: nat.sup_mask_loss_fwd_wrapper(B, n, k, mask, gt, valid, cols, None, ws, sums, terms)),
             ("ogc_sup_mask_loss_bwd", lambda: nat.sup_mask_loss_bwd_wrapper(B, n, k, mask, gt, valid, cols, None, sums, 2.0, 0.0,
                                                                             gout, grad)))
    launches = {}
    for label, fn in steps:
        if label == "ogc_lsap_maximize":
            torch.mul(cost_ce, -2.0, out=neg)
        ms = []
        for i in range(warmup + calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= warmup:
                ms.append(e0.elapsed_time(e1))
        launches[label] = ms
    assert abs(float(terms[0]) * 2.0 - float(la)) <= 1e-6 * abs(float(la))

    k_med, t_med = statistics.median(wall["kernel"]), statistics.median(wall["tensor"])
    lines = ["%s: B=%d n=%d k=%d, %d objects, BCE, weights %s; mask bytes %.1f MB (a (B, n, k, k) tensor: %.1f MB)"
             % (name, B, n, k, n_object, WEIGHTS, mask.numel() * 4 / 1e6, mask.numel() * k * 4 / 1e6),
             "  kernel path, forward + backward, wall per call: %s" % summary(wall["kernel"]),
             "  tensor path, forward + backward, wall per call: %s" % summary(wall["tensor"]),
             "  tensor / kernel (medians): %.2f" % (t_med / k_med),
             "  kernel path with sync=False, wall per call: %s" % summary(wall["kernel_nosync"])]
    lines += ["  %s alone, HIP events: %s" % (label, summary(ms)) for label, ms in launches.items()]
    return lines, t_med / k_med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "sup_loss_time.py measures on the GPU"
    lines = ["device: %s" % torch.cuda.get_device_name(0)]
    for shape in SHAPES:
        lines += measure(*shape, args.calls, args.warmup)[0]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

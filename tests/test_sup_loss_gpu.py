"""The supervised-loss kernels (csrc/sup_loss.hip: ogc_sup_match_cost, ogc_sup_mask_loss_fwd / _bwd) and SupervisedMaskLoss on
the MI355X.

Kernel tests: the truth is the package's tensor path on float64 CPU tensors (tests/sup_cases.py: tensor_path), the yardstick
the same path in float32 — the reference's own arithmetic, pinned to the reference by tests/test_sup_loss_cpu.py.  A kernel
result passes when its distance from the truth is at most TWICE the float32 tensor path's largest distance from the truth on
the same inputs, plus 4 float32 ulps of the value (of the largest entry, for the gradient): sup_cases.within.  The kernels sum
in fp64, so they should sit below the yardstick; the margin covers the device's logf / log1pf differing from the host's by an
ulp.  Assignments are compared through the permuted labels only (empty GT columns tie).  The fwd / bwd kernels get the truth's
assignment, so that a kernel is judged on its own arithmetic.  Every test prints its ratios as SUP_LOSS_PARITY.

Loss tests: SupervisedMaskLoss on the GPU against tests/golden/sup_loss.npz (the reference's own class, make_sup_golden.py)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import sup_cases as sc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TILE = 64   # OGC_SUP_LOSS_TILE
KS = (1, 2, 15, 22, 32)
# 1; one fewer than, exactly and one more than a tile; the same around two tiles; 193: three full tiles, the fourth workgroup of
# the sample holds a single point
NS = (1, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 3 * TILE + 1)
FOCAL = (0.25, 2)


def kernels(mask, gt, valid, focal, weights, cols=None, grad_out=1.0):
    """The three entry points on GPU copies of CPU tensors -> the dictionary sup_cases.tensor_path returns (numpy)."""
    from ogc_amd import pointnet2_cuda as nat
    m, g = mask.cuda(), gt.cuda()
    v = None if valid is None else valid.cuda()
    b, n, k = m.shape
    ws = nat.sup_loss_workspace(b, n, k, m.device).fill_(float("nan"))   # its contents must not matter
    cost_ce = torch.full((b, k, k), -7.0, device=m.device)
    cost_dice = torch.full((b, k, k), -7.0, device=m.device)
    nat.sup_match_cost_wrapper(b, n, k, m, g, v, focal, ws, cost_ce, cost_dice)
    own = torch.empty((b, k), dtype=torch.int32, device=m.device)
    nat.lsap_maximize_wrapper(b, k, -(weights[0] * cost_ce + weights[1] * cost_dice.mean()), own)
    use = own if cols is None else cols.to(torch.int32).cuda()
    sums = torch.full((b, k, 4), -7.0, dtype=torch.float64, device=m.device)
    terms = torch.full((2,), -7.0, device=m.device)
    nat.sup_mask_loss_fwd_wrapper(b, n, k, m, g, v, use, focal, ws, sums, terms)
    grad = torch.full_like(m, -7.0)
    nat.sup_mask_loss_bwd_wrapper(b, n, k, m, g, v, use, focal, sums, weights[0], weights[1],
                                  torch.tensor([grad_out], device=m.device), grad)
    torch.cuda.synchronize()
    out = dict(cost_ce=cost_ce, cost_dice=cost_dice, cols=own.long(), sums=sums, terms=terms, grad=grad)
    return {key: val.cpu() for key, val in out.items()}


def check(tag, mask, gt, valid, focal, weights=(2.0, 0.1), grad_out=1.0):
    """One input through the kernels, the truth and the yardstick; returns the largest ratio kernel / float32 path."""
    truth = sc.tensor_path(mask, gt, valid, focal, weights, torch.float64)
    yard = sc.tensor_path(mask, gt, valid, focal, weights, torch.float32, cols=truth["cols"])
    got = kernels(mask, gt, valid, focal, weights, cols=truth["cols"], grad_out=grad_out)
    # the kernels' own cost decides the same labels
    assert torch.equal(sc.S().permute_labels(gt, got["cols"]), truth["perm_gt"].float()), "%s: permuted labels" % tag
    worst = 0.0
    for key in ("cost_ce", "cost_dice", "sums", "terms"):
        ok, ratio = sc.within(got[key], truth[key], yard[key])
        assert ok, "%s: %s outside the bound (kernel / float32 path = %.2f)" % (tag, key, ratio)
        worst = max(worst, ratio if np.isfinite(ratio) else 0.0)
    scale = float(truth["grad"].abs().max())
    ok, ratio = sc.within(got["grad"] / grad_out, truth["grad"], yard["grad"], scale=scale)
    assert ok, "%s: gradient outside the bound (kernel / float32 path = %.2f)" % (tag, ratio)
    return max(worst, ratio if np.isfinite(ratio) else 0.0)


@pytest.mark.parametrize("n", NS)
def test_every_shape_against_the_float64_truth(n):
    """k x B at this n; the loss (BCE / focal), valid (none / partial) and fractional labels rotate through the cases."""
    worst, i = 0.0, 0
    for k in KS:
        for B in (1, 3):
            focal = FOCAL if i % 2 else None
            valid = "partial" if (i // 2) % 2 else "none"
            mask, gt, v = sc.make_inputs(B, n, k, 100 * n + k + B, fractional=bool((i // 4) % 2) or k == 15, valid=valid)
            worst = max(worst, check("B=%d n=%d k=%d focal=%s valid=%s" % (B, n, k, focal, valid), mask, gt, v, focal,
                                     grad_out=0.5 if i % 3 == 0 else 1.0))
            i += 1
    print("SUP_LOSS_PARITY shapes n=%d: worst kernel / float32-path distance ratio %.3f" % (n, worst))


@pytest.mark.parametrize("focal", [None, FOCAL])
def test_a_sample_without_valid_points(focal):
    """valid all zero for sample 0: its costs are 0, its Dice entries 1 - 1 / (0 + 0 + 1) = 0, the other samples are untouched."""
    mask, gt, v = sc.make_inputs(3, 2 * TILE + 5, 15, 7, valid="zero0")
    ratio = check("zero0", mask, gt, v, focal)
    got = kernels(mask, gt, v, focal, (2.0, 0.1))
    assert torch.equal(got["cost_ce"][0], torch.zeros(15, 15)) and torch.equal(got["cost_dice"][0], torch.zeros(15, 15))
    v2 = v.clone()
    v2[0] = 1.0
    other = kernels(mask, gt, v2, focal, (2.0, 0.1))
    assert torch.equal(got["cost_ce"][1:], other["cost_ce"][1:]) and torch.equal(got["cost_dice"][1:], other["cost_dice"][1:])
    print("SUP_LOSS_PARITY zero0 focal=%s: ratio %.3f" % (focal, ratio))


@pytest.mark.parametrize("focal", [None, FOCAL, (-1, 3)])
def test_exact_zeros_and_ones_in_the_mask(focal):
    """The -100 clamp of both logarithms, the 1e-12 clamp of the gradient, and a gradient of exactly 0 where p == t in {0, 1}."""
    mask, gt, v = sc.make_inputs(2, TILE + 9, 4, 11)
    mask, gt = mask.clone(), gt.clone()
    hot = mask > 0.5                                  # the slot of the point's object (~0.9 there): the matched label
    mask[:, 0::3] = hot[:, 0::3].float()             # p == t in {0, 1}
    mask[:, 1::13] = 1.0 - hot[:, 1::13].float()     # p == 1 - t: e = 100 exactly
    ratio = check("exact01", mask, gt, None, focal, weights=(2.0, 0.0))
    truth = sc.tensor_path(mask, gt, None, focal, (2.0, 0.0), torch.float64)
    got = kernels(mask, gt, None, focal, (2.0, 0.0), cols=truth["cols"])
    perm = truth["perm_gt"].float()
    same = (mask == perm) & ((perm == 0) | (perm == 1))
    assert same.any() and torch.equal(got["grad"][same], torch.zeros(int(same.sum())))
    wrong = (mask == 1 - perm) & ((perm == 0) | (perm == 1))
    assert wrong.any() and torch.isfinite(got["grad"][wrong]).all() and (got["grad"][wrong].abs() > 0).all()
    if focal is None:   # one slot, one point, p = 0 against t = 1: the cost is exactly 100
        one = kernels(torch.zeros(1, 1, 1), torch.ones(1, 1, 1), None, None, (2.0, 0.0))
        assert float(one["cost_ce"]) == 100.0 and float(one["terms"][0]) == 100.0
    print("SUP_LOSS_PARITY exact01 focal=%s: ratio %.3f" % (focal, ratio))


def test_fractional_labels():
    mask, gt, v = sc.make_inputs(3, 3 * TILE + 1, 22, 5, fractional=True, valid="partial")
    assert ((gt > 0) & (gt < 1)).any()
    print("SUP_LOSS_PARITY fractional: ratio %.3f / %.3f" % (check("fractional bce", mask, gt, v, None),
                                                           check("fractional focal", mask, gt, v, FOCAL)))


@pytest.mark.parametrize("alpha", [0.25, -1])
@pytest.mark.parametrize("gamma", [2, 3])
def test_focal_variants(alpha, gamma):
    mask, gt, v = sc.make_inputs(3, TILE + 1, 15, 3, fractional=True, valid="partial")
    print("SUP_LOSS_PARITY focal alpha=%s gamma=%s: ratio %.3f" % (alpha, gamma, check("focal", mask, gt, v, (alpha, gamma))))


@pytest.mark.parametrize("bad", [float("nan"), 1.5, -0.25])
def test_a_nan_or_out_of_range_mask_entry_stays_in_its_sample(bad):
    """That sample's costs are NaN, its assignment -1, both terms NaN; nothing faults; the other samples' sums are those of a
    clean run."""
    from ogc_amd import pointnet2_cuda as nat
    mask, gt, v = sc.make_inputs(3, 2 * TILE + 1, 15, 9, valid="partial")
    clean = kernels(mask, gt, v, None, (2.0, 0.0))
    dirty_mask = mask.clone()
    dirty_mask[1, TILE + 3, 4] = bad
    m, g, vv = dirty_mask.cuda(), gt.cuda(), v.cuda()
    ws = nat.sup_loss_workspace(3, m.shape[1], 15, m.device)
    cost_ce, cost_dice = torch.empty(3, 15, 15, device=m.device), torch.empty(3, 15, 15, device=m.device)
    nat.sup_match_cost_wrapper(3, m.shape[1], 15, m, g, vv, None, ws, cost_ce, cost_dice)
    assert torch.isnan(cost_ce[1, 4]).all() and torch.isnan(cost_dice[1, 4]).all()
    assert torch.equal(cost_ce[[0, 2]].cpu(), clean["cost_ce"][[0, 2]]) and torch.equal(cost_dice[[0, 2]].cpu(), clean["cost_dice"][[0, 2]])
    cols = torch.empty(3, 15, dtype=torch.int32, device=m.device)
    nat.lsap_maximize_wrapper(3, 15, -cost_ce, cols)
    assert (cols[1] == -1).all() and torch.equal(cols[[0, 2]].cpu().long(), clean["cols"][[0, 2]])
    sums = torch.empty(3, 15, 4, dtype=torch.float64, device=m.device)
    terms = torch.empty(2, device=m.device)
    nat.sup_mask_loss_fwd_wrapper(3, m.shape[1], 15, m, g, vv, cols, None, ws, sums, terms)
    grad = torch.empty_like(m)
    nat.sup_mask_loss_bwd_wrapper(3, m.shape[1], 15, m, g, vv, cols, None, sums, 2.0, 0.1, torch.ones(1, device=m.device), grad)
    torch.cuda.synchronize()
    assert torch.isnan(terms).all() and torch.isnan(sums[1]).all() and torch.isnan(grad[1]).all()
    assert torch.equal(sums[[0, 2]].cpu(), clean["sums"][[0, 2]]) and torch.isfinite(grad[[0, 2]]).all()


def test_two_calls_give_identical_bits():
    mask, gt, v = sc.make_inputs(3, 3 * TILE + 1, 22, 13, fractional=True, valid="partial")
    a = kernels(mask, gt, v, FOCAL, (2.0, 0.1))
    b = kernels(mask, gt, v, FOCAL, (2.0, 0.1))
    for key in a:
        assert torch.equal(a[key], b[key]), key


def test_every_invalid_argument_is_refused():
    """OGC_ERR_INVALID_ARG (-1), nothing launched: the outputs keep their fill."""
    from ogc_amd import _lib
    lib = _lib.load()
    B, n, k = 2, 70, 4
    mask, gt, v = (t.cuda() for t in sc.make_inputs(B, n, k, 1, valid="partial"))
    ws = torch.zeros(int(lib.ogc_sup_loss_ws_doubles(B, n, k)), dtype=torch.float64, device="cuda")
    cost = torch.full((2, B, k, k), -7.0, device="cuda")
    cols = torch.zeros(B, k, dtype=torch.int32, device="cuda")
    sums = torch.full((B, k, 4), -7.0, dtype=torch.float64, device="cuda")
    terms = torch.full((2,), -7.0, device="cuda")
    grad = torch.full_like(mask, -7.0)
    gout = torch.ones(1, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    dbl = ctypes.c_double

    def cost_args(B=B, n=n, k=k, mask=P(mask), gt=P(gt), alpha=0.25, gamma=2.0, ws=P(ws), c0=P(cost[0]), c1=P(cost[1])):
        return ("ogc_sup_match_cost", B, n, k, mask, gt, P(v), 1, dbl(alpha), dbl(gamma), ws, c0, c1, None)

    def fwd_args(B=B, n=n, k=k, mask=P(mask), gt=P(gt), cols=P(cols), alpha=0.25, gamma=2.0, ws=P(ws), sums=P(sums), terms=P(terms)):
        return ("ogc_sup_mask_loss_fwd", B, n, k, mask, gt, P(v), cols, 1, dbl(alpha), dbl(gamma), ws, sums, terms, None)

    def bwd_args(B=B, n=n, k=k, mask=P(mask), gt=P(gt), cols=P(cols), alpha=0.25, gamma=2.0, sums=P(sums), gout=P(gout), grad=P(grad)):
        return ("ogc_sup_mask_loss_bwd", B, n, k, mask, gt, P(v), cols, 1, dbl(alpha), dbl(gamma), sums, dbl(2.0), dbl(0.1), gout, grad,
                None)

    common = [dict(B=-1), dict(n=0), dict(k=0), dict(k=33), dict(gamma=0.5), dict(gamma=float("nan")), dict(gamma=float("inf")),
              dict(alpha=float("nan")), dict(mask=None), dict(gt=None)]
    bad = [cost_args(**kw) for kw in common + [dict(ws=None), dict(c0=None), dict(c1=None)]]
    bad += [fwd_args(**kw) for kw in common + [dict(cols=None), dict(ws=None), dict(sums=None), dict(terms=None)]]
    bad += [bwd_args(**kw) for kw in common + [dict(cols=None), dict(sums=None), dict(gout=None), dict(grad=None)]]
    for name, *args in bad:
        assert getattr(lib, name)(*args) == -1, (name, args)
    for name, *args in (cost_args(B=0, mask=None), fwd_args(B=0, mask=None), bwd_args(B=0, mask=None)):   # B == 0: a no-op
        assert getattr(lib, name)(*args) == 0
    assert lib.ogc_sup_loss_ws_doubles(B, n, 33) == 0 and lib.ogc_sup_loss_ws_doubles(B, 0, k) == 0
    torch.cuda.synchronize()
    for t in (cost, sums, terms, grad):
        assert bool((t == -7.0).all())


# ---- SupervisedMaskLoss against the fixture recorded from the reference's own class ----------------------------------------

@pytest.fixture(scope="module")
def golden():
    data = np.load(os.path.join(HERE, "golden", "sup_loss.npz"))
    return data, json.loads(str(data["meta"]))


def test_loss_on_the_gpu_reproduces_the_reference(golden):
    from ogc_amd.losses import seg_loss_sup as S
    data, meta = golden
    mask, gt, valid = (torch.from_numpy(data[key]) for key in ("mask", "gt_mask", "valid"))
    for case in meta["cases"]:
        tag = case["tag"]
        ce_loss, dice_loss = sc.make_losses(case["focal"])
        crit = S.SupervisedMaskLoss(ce_loss, dice_loss, case["weights"])
        v = valid.cuda() if case["valid"] else None
        m = mask.cuda().requires_grad_(True)
        assert crit.kernels_apply(m, gt.cuda(), v)
        loss, loss_dict = crit(m, gt.cuda(), v)
        loss.backward()
        # the labels the kernel path matched, through the assignment its own cost decides
        _, _, cols = S._FusedMaskLoss.apply(m.detach(), gt.cuda(), v, ce_loss.focal, *map(float, case["weights"]))
        assert np.array_equal(S.permute_labels(gt, cols.long().cpu()).numpy(), data[tag + "/perm_gt"]), tag
        names = ("cross_entropy", "dice", "sum")
        got = np.array([loss_dict[key] for key in names] + [float(loss)])
        ref32 = np.append(data[tag + "/loss_dict"], data[tag + "/loss"])
        truth = np.append(data[tag + "/loss_dict64"], data[tag + "/loss64"])
        ok, ratio = sc.within(got, truth, ref32)
        assert ok, "%s: loss terms %r, reference fp32 %r, float64 truth %r" % (tag, got, ref32, truth)
        g64 = data[tag + "/grad64"]
        ok, gratio = sc.within(m.grad.cpu().numpy(), g64, data[tag + "/grad"], scale=np.abs(g64).max())
        assert ok, "%s: gradient (kernel / reference fp32 distance = %.2f)" % (tag, gratio)
        print("SUP_LOSS_PARITY fixture %s: loss ratio %.3f, gradient ratio %.3f" % (tag, ratio, gratio))


def test_sync_false_makes_no_host_round_trip(golden):
    """Forward and backward with sync=False under torch's sync debug mode "error": any synchronising call (.item(), a blocking
    copy) raises.  The monitored values arrive through PendingLossDict afterwards."""
    from ogc_amd.losses import seg_loss_sup as S
    data, meta = golden
    crit = S.SupervisedMaskLoss(*sc.make_losses(FOCAL), [2.0, 0.1])
    m = torch.from_numpy(data["mask"]).cuda().requires_grad_(True)
    gt, valid = torch.from_numpy(data["gt_mask"]).cuda(), torch.from_numpy(data["valid"]).cuda()
    crit(m, gt, valid, sync=False)[0].backward()   # first call: allocations, library load
    m.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss, pending = crit(m, gt, valid, sync=False)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert isinstance(pending, S.PendingLossDict)
    d = pending.resolve()
    assert set(d) == {"cross_entropy", "dice", "sum"} and d["sum"] == float(loss)
    assert abs(d["sum"] - (2.0 * d["cross_entropy"] + 0.1 * d["dice"])) <= 1e-6 * abs(d["sum"])
    # and the tensor path (kernels switched off) agrees on the same GPU tensors
    S_KERNELS = S.KERNELS
    try:
        S.KERNELS = False
        m2 = m.detach().clone().requires_grad_(True)
        loss2, d2 = crit(m2, gt, valid)
        loss2.backward()
    finally:
        S.KERNELS = S_KERNELS
    assert abs(float(loss2) - float(loss)) <= 1e-5 * abs(float(loss))
    assert float((m2.grad - m.grad).abs().max()) <= 1e-5 * float(m.grad.abs().max())

"""The first two layers of a set-abstraction MLP without the first convolution's output y1 = conv(x0, W1) or its gradient in
memory (csrc/first_conv.h, fused._FirstPairConv): every kernel of the pair against the kernel it replaces on a stored y1 — the
same coefficient tensors fed to both sides — and against float64 sums; the whole node against pointwise_conv + _NormActConv;
one SA level with the route on and off.

Bounds.  y2 must equal, bit for bit, what ogc_conv1x1_gemm_affine gives on the stored y1.  Sums (statistics, moment matrices,
dW1, dW2, dgamma1, dbeta1) may differ from the parent path only in how partial sums are grouped and in which order atomics
land: their error against float64 truth must stay within 2x the parent path's error on the same inputs, plus one float32
ulp of the tensor's largest magnitude.  Every case prints both errors."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GROUPS = 4          # the models' GroupNorm grouping (models/_segnet.py: BN_CONFIG)
EPS = 1e-5
ULP = float(np.finfo(np.float32).eps)


def _inputs(B, c0, c1, c2, hw, edge):
    g = torch.Generator().manual_seed(1000 * c0 + 10 * c1 + B + hw)
    x0 = torch.randn(B, c0, hw, generator=g)
    w1 = torch.randn(c1, c0, generator=g) / c0 ** 0.5
    w2 = torch.randn(c2, c1, generator=g) / c1 ** 0.5
    gamma = 1.0 + 0.25 * torch.randn(c1, generator=g)
    beta = 0.25 * torch.randn(c1, generator=g)
    gy = torch.randn(B, c2, hw, generator=g)
    if edge:
        # a negative scale, and one sample whose x0 is all zeros with beta = 0 on half of the channels: y1 = 0 there, its
        # GroupNorm maps it to beta exactly, so those pre-activations sit exactly on the ReLU gate
        gamma[1::3] = -gamma[1::3].abs()
        beta[::2] = 0.0
        x0[B - 1] = 0.0
    return [t.cuda().contiguous() for t in (x0, w1, w2, gamma, beta, gy)]


def _bounded(name, new, parent, truth):
    truth = truth.double()
    e_new = (new.double() - truth).abs().max().item()
    e_par = (parent.double() - truth).abs().max().item()
    floor = ULP * truth.abs().max().item()
    print("%-10s new %.3e  parent %.3e  floor %.3e" % (name, e_new, e_par, floor))
    assert e_new <= 2.0 * e_par + floor, "%s: error %.3e > 2 x %.3e + %.3e" % (name, e_new, e_par, floor)


def _slot_sum(stats, B):
    return stats.view(-1, B, GROUPS, 2).sum(0)


CASES = [(B, c0, cc, hw) for B in (1, 3) for c0 in (3, 6, 8) for cc in ((32, 32), (16, 64)) for hw in (64, 320, 4096)]


@pytest.mark.parametrize("B,c0,cc,hw", CASES)
def test_kernels_and_node_against_the_stored_path(B, c0, cc, hw):
    _run_case(B, c0, cc, hw, False)


@pytest.mark.parametrize("cc", [(32, 32), (16, 64)])
def test_pre_activations_on_the_relu_gate(cc):
    _run_case(3, 6, cc, 320, True)


def _run_case(B, c0, cc, hw, edge):
    import ogc_amd  # noqa: F401
    import ogc_amd.fused as fused
    from ogc_amd.pointnet2 import pointnet2 as api
    nat = api._native
    c1, c2 = cc
    x0, w1, w2, gamma, beta, gy = _inputs(B, c0, c1, c2, hw, edge)
    dev = x0.device
    slots = nat.conv1x1_gn_slots()
    f32 = dict(dtype=torch.float32, device=dev)

    # ---- statistics of y1: the matrix kernel's epilogue on a stored y1 / the pass that stores nothing
    y1 = torch.empty(B, c1, hw, **f32)
    st_par = torch.zeros(slots * B * GROUPS * 2, dtype=torch.float64, device=dev)
    nat.conv1x1_gemm_gnstats_wrapper(B, c1, c0, hw, GROUPS, w1, x0, y1, st_par)
    st_new = torch.full_like(st_par, 7.0)   # (overwritten)
    nat.first_conv_stats_wrapper(B, c1, c0, hw, GROUPS, x0, w1, st_new)
    yg = y1.double().view(B, GROUPS, -1)
    truth = torch.stack([yg.sum(-1), (yg * yg).sum(-1)], dim=-1)
    _bounded("stats", _slot_sum(st_new, B), _slot_sum(st_par, B), truth)

    # ---- one set of coefficients for both sides
    mean, rstd = torch.empty(B * GROUPS, **f32), torch.empty(B * GROUPS, **f32)
    a, bb = torch.empty(B * c1, **f32), torch.empty(B * c1, **f32)
    nat.group_norm_coeffs_wrapper(B, c1, hw, GROUPS, EPS, None, gamma, beta, st_par, slots, None, mean, rstd, a, bb)

    # ---- forward: bit-identical y2
    y2_par, y2_new = torch.empty(B, c2, hw, **f32), torch.empty(B, c2, hw, **f32)
    s2_par = torch.zeros(slots * B * GROUPS * 2, dtype=torch.float64, device=dev)
    s2_new = torch.full_like(s2_par, 7.0)
    nat.conv1x1_gemm_affine_wrapper(B, c2, c1, hw, True, GROUPS, w2, y1, a, bb, y2_par, s2_par)
    nat.conv1x1_gemm_affine_first_wrapper(B, c2, c1, hw, True, GROUPS, c0, w2, x0, w1, a, bb, y2_new, s2_new)
    assert torch.equal(y2_new, y2_par)
    yg2 = y2_par.double().view(B, GROUPS, -1)
    _bounded("stats2", _slot_sum(s2_new, B), _slot_sum(s2_par, B), torch.stack([yg2.sum(-1), (yg2 * yg2).sum(-1)], dim=-1))

    # ---- moment matrices against float64 (the sign of the exact a y + b is the sign of its fp32 fused multiply-add)
    mo_par = torch.zeros(B, 2, c2, c1, **f32)
    mo_new = torch.full_like(mo_par, 7.0)
    nat.conv1x1_wgrad_moments_wrapper(B, c1, c2, hw, True, y1, a, bb, gy, mo_par)
    nat.conv1x1_wgrad_moments_first_wrapper(B, c1, c2, hw, True, c0, x0, w1, a, bb, gy, mo_new)
    y64 = y1.double()
    mask = ((a.double().view(B, c1, 1) * y64 + bb.double().view(B, c1, 1)) > 0).double()
    truth_m = torch.stack([gy.double() @ mask.transpose(1, 2), gy.double() @ (mask * y64).transpose(1, 2)], dim=1)
    _bounded("moments", mo_new, mo_par, truth_m)

    # ---- dW1: the adjoint's result stored and fed to the weight-gradient kernel / folded in the adjoint's epilogue
    dw2 = torch.zeros(c2, c1, **f32)
    coef = torch.empty(B, c1, 3, **f32)
    ggb = torch.zeros(2, c1, **f32)
    nat.gn_moments_combine_wrapper(B, c1, c2, hw, GROUPS, mo_par, w2, a, bb, mean, rstd, gamma, dw2, coef, ggb[0], ggb[1])
    g1 = torch.empty(B, c1, hw, **f32)
    nat.conv1x1_dgrad_adjoint_wrapper(B, c1, c2, hw, True, w2, gy, y1, a, bb, coef, g1)
    dw1_par = torch.zeros(c1, c0, **f32)
    nat.conv1x1_wgrad_wrapper(B, c0, c1, hw, x0, g1, dw1_par)
    dw1_new = torch.full_like(dw1_par, 7.0)
    nat.conv1x1_dgrad_adjoint_first_wrapper(B, c1, c2, hw, True, c0, w2, gy, x0, w1, a, bb, coef, dw1_new)
    truth_w = torch.einsum("bmp,bcp->mc", g1.double(), x0.double())
    _bounded("dW1", dw1_new, dw1_par, truth_w)

    # ---- the whole node against pointwise_conv + _NormActConv, truth: the same op sequence in float64
    x4 = x0.view(B, c0, hw // 16, 16)
    probe = gy.view(B, c2, hw // 16, 16)

    def grads(route):
        p = [t.clone().requires_grad_(True) for t in (w1.view(c1, c0, 1, 1), gamma, beta, w2.view(c2, c1, 1, 1))]
        if route == "new":
            y2, _ = fused._FirstPairConv.apply(x4, p[0], p[1], p[2], p[3], GROUPS, EPS, True, GROUPS)
        elif route == "parent":
            y1_, st = fused._PointwiseConv.apply(x4, p[0], GROUPS)
            y2, _ = fused._NormActConv.apply(y1_, st, p[1], p[2], p[3], GROUPS, EPS, True, GROUPS)
        else:
            p = [t.detach().double().requires_grad_(True) for t in p]
            h = torch.nn.functional.conv2d(x4.double(), p[0])
            h = torch.relu(torch.nn.functional.group_norm(h, GROUPS, p[1], p[2], EPS))
            y2 = torch.nn.functional.conv2d(h, p[3])
        (y2 * probe.to(y2.dtype)).sum().backward()
        return y2.detach(), [t.grad for t in p]

    (y_new, g_new), (y_par, g_par), (_, g_64) = grads("new"), grads("parent"), grads("truth")
    assert (y_new - y_par).abs().max().item() <= 1e-5 * y_par.abs().max().item()   # (coefficients from two statistics passes)
    for name, gn_, gp_, gt_ in zip(("dW1", "dgamma1", "dbeta1", "dW2"), g_new, g_par, g_64):
        _bounded("node/" + name, gn_, gp_, gt_)


def test_preconditions_are_reported():
    import ogc_amd  # noqa: F401
    from ogc_amd import _lib
    from ogc_amd.pointnet2 import pointnet2 as api
    nat = api._native
    x0 = torch.randn(1, 9, 64).cuda()
    w1 = torch.randn(32, 9).cuda()
    stats = torch.zeros(nat.conv1x1_gn_slots() * GROUPS * 2, dtype=torch.float64).cuda()
    with pytest.raises(_lib.OgcOpsError):   # c0 > 8
        nat.first_conv_stats_wrapper(1, 32, 9, 64, GROUPS, x0, w1, stats)
    x0 = torch.randn(1, 6, 48).cuda()
    with pytest.raises(_lib.OgcOpsError):   # hw % 64 != 0
        nat.first_conv_stats_wrapper(1, 32, 6, 48, GROUPS, x0, torch.randn(32, 6).cuda(), stats)


class _Counting:
    """Stands in for the native module and counts the calls of two wrappers."""

    def __init__(self, native, names):
        self._native, self.calls = native, {n: 0 for n in names}

    def __getattr__(self, name):
        fn = getattr(self._native, name)
        if name in self.calls:
            def counted(*args, **kwargs):
                self.calls[name] += 1
                return fn(*args, **kwargs)
            return counted
        return fn


def test_sa_level_with_and_without_the_pair(monkeypatch):
    """The first level of segnet_kitti at N = 512, B = 2: outputs at the golden module tolerance, parameter gradients at the golden
    gradient tolerance of the segnets; with the pair no stored first convolution and no weight-gradient launch for it."""
    import ogc_amd  # noqa: F401
    import ogc_amd.fused as fused
    from ogc_amd.pointnet2 import pointnet2 as api
    from ogc_amd.utils.pointnet2_util import PointnetSAModuleMSG
    torch.manual_seed(3)
    bn = {"class": "GroupNorm", "num_groups": 4}
    sa = PointnetSAModuleMSG(npoint=128, radii=[1, 2], nsamples=[64, 64], mlps=[[3, 32, 32, 32], [3, 32, 32, 64]], bn=bn).cuda()
    xyz = ((torch.rand(2, 512, 3) - 0.5) * 8).cuda()
    feats = xyz.transpose(1, 2).contiguous()
    probe = torch.randn(2, 96, 128).cuda()
    counting = _Counting(api._native, ("conv1x1_gemm_gnstats_wrapper", "conv1x1_wgrad_wrapper"))
    monkeypatch.setattr(api, "_native", counting)
    runs = {}
    for on in (True, False):
        monkeypatch.setattr(fused, "FIRST_PAIR_FUSED", on)
        for k in counting.calls:
            counting.calls[k] = 0
        sa.zero_grad()
        out = sa(xyz, feats)[1]
        (out * probe).sum().backward()
        runs[on] = (out.detach().clone(), {n: p.grad.clone() for n, p in sa.named_parameters()}, dict(counting.calls))
    assert runs[True][2] == {"conv1x1_gemm_gnstats_wrapper": 0, "conv1x1_wgrad_wrapper": 0}
    assert runs[False][2]["conv1x1_gemm_gnstats_wrapper"] == 2 and runs[False][2]["conv1x1_wgrad_wrapper"] >= 2
    rtol, atol, grad_rtol = 1e-5, 1e-6, 1e-3   # tests/golden_cases.py: run_modules, run_segnet
    assert torch.allclose(runs[True][0], runs[False][0], rtol=rtol, atol=atol)
    for n, g_off in runs[False][1].items():
        g_on = runs[True][1][n]
        err, scale = (g_on - g_off).abs().max().item(), g_off.abs().max().item()
        print("%-40s err %.3e  scale %.3e" % (n, err, scale))
        assert err <= grad_rtol * scale + 1e-8, n

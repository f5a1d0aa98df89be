"""The backward of a deeper level's chain (grouped first layer -> one middle layer -> pooled tail) over the LIVE steps of its
neighbour lists (fused.LIVE_DEEP_LEVELS): the middle layer's plain list forms (ogc_conv1x1_wgrad_moments_live,
ogc_conv1x1_dgrad_adjoint_live_fill) against the dense forms and float64 sums, the pooled list forms at the tail's width
(cin = 64, cout = 128), one level with the switch on and off, preconditions.  Lists, bound and constructions:
tests/test_live_steps_gpu.py.

Bounds.  Moments: a list form and its dense form are fp32 groupings of one sum, so the list form's error against the float64
evaluation may exceed the dense form's by at most a factor of 2 (every case prints both errors and their ratio).  Gradients with
respect to the layer's input: the same expression per position, so bit-equal to the dense form given the same coefficients."""
import pytest
import torch

from test_live_steps_gpu import B, EPS, GROUPS, NPTS, P, SHIFT, _Counting, _err, _idx, _mask64, _native, _rule

pytestmark = pytest.mark.gpu

C0 = 6


def _keep(idx_np, hw):
    """(B, hw) bool: the positions of live steps."""
    keep = torch.zeros(B, hw, dtype=torch.bool)
    for b, entries in enumerate(_rule(idx_np)):
        for e in entries:
            st = e & ((1 << SHIFT) - 1)
            keep[b, 16 * st:16 * st + 16] = True
    return keep.cuda()


def _gathered(src, idx, S):
    c = src.shape[1]
    return torch.gather(src.unsqueeze(2).expand(B, c, P, NPTS), 3, idx.long().unsqueeze(1).expand(B, c, P, S)).contiguous()


def _coeffs(nat, y, c, gamma, beta, hw):
    f32 = dict(dtype=torch.float32, device=y.device)
    mean, rstd = torch.empty(B * GROUPS, **f32), torch.empty(B * GROUPS, **f32)
    a, bb = torch.empty(B * c, **f32), torch.empty(B * c, **f32)
    ws = nat.group_norm_ws(B, c, GROUPS, False, y.device)
    nat.group_norm_coeffs_wrapper(B, c, hw, GROUPS, EPS, y, gamma, beta, None, 0, ws, mean, rstd, a, bb)
    return mean, rstd, a, bb


@pytest.mark.parametrize("S", [64, 32])
@pytest.mark.parametrize("cin,cout", [(64, 64), (20, 36)])
def test_plain_list_forms_against_dense_forms(S, cin, cout):
    """y_prev: a dense forward convolution of gathered points (repeats bit-equal); grad_y: gathered as well.  The list forms get
    copies that hold NaN at every skipped position: a read there would show in the moments or in grad_prev."""
    nat = _native()
    idx_np = _idx(S)
    idx = torch.from_numpy(idx_np).cuda()
    g = torch.Generator().manual_seed(1000 * S + 10 * cin + cout)
    hw = P * S
    f32 = dict(dtype=torch.float32, device="cuda")
    x0 = _gathered(torch.randn(B, C0, NPTS, generator=g).cuda(), idx, S)
    w0 = (torch.randn(cin, C0, generator=g) / C0 ** 0.5).cuda()
    w = (torch.randn(cout, cin, generator=g) / cin ** 0.5).cuda()
    gamma, beta = (1.0 + 0.25 * torch.randn(cin, generator=g)).cuda(), (0.25 * torch.randn(cin, generator=g)).cuda()
    y_prev = torch.empty(B, cin, P, S, **f32)
    nat.conv1x1_gemm_wrapper(B, cin, C0, hw, 0, w0, x0.view(B, C0, hw), y_prev)
    grad_y = _gathered(torch.randn(B, cout, NPTS, generator=g).cuda(), idx, S)
    mean, rstd, a, bb = _coeffs(nat, y_prev, cin, gamma, beta, hw)
    live, n_live = nat.live_steps_wrapper(idx)
    keep = _keep(idx_np, hw)
    assert 0 < int((~keep).sum()) < keep.numel()
    nan = torch.tensor(float("nan"), **f32)
    y_nan = torch.where(keep.view(B, 1, P, S), y_prev, nan)
    g_nan = torch.where(keep.view(B, 1, P, S), grad_y, nan)

    mo_d, mo_l = torch.zeros(B, 2, cout, cin, **f32), torch.full((B, 2, cout, cin), 7.0, **f32)
    nat.conv1x1_wgrad_moments_wrapper(B, cin, cout, hw, True, y_prev, a, bb, grad_y, mo_d)
    nat.conv1x1_wgrad_moments_live_wrapper(B, cin, cout, hw, True, S, y_nan, a, bb, g_nan, live, n_live, mo_l)
    m, y64 = _mask64(a, bb, y_prev, cin)
    gy = grad_y.double().view(B, cout, hw)
    _err("plain moments", mo_l, mo_d, torch.stack([gy @ m.transpose(1, 2), gy @ (m * y64).transpose(1, 2)], dim=1))

    coef = torch.empty(B, cin, 3, **f32)
    ggb = torch.zeros(2, cin, **f32)
    nat.gn_moments_combine_wrapper(B, cin, cout, hw, GROUPS, mo_d, w, a, bb, mean, rstd, gamma, torch.empty(cout, cin, **f32),
                                   coef, ggb[0], ggb[1])
    gp_d = torch.empty(B, cin, P, S, **f32)
    gp_l = torch.full((B, cin, P, S), float("nan"), **f32)
    nat.conv1x1_dgrad_adjoint_wrapper(B, cin, cout, hw, True, w, grad_y, y_prev, a, bb, coef, gp_d)
    nat.conv1x1_dgrad_adjoint_live_fill_wrapper(B, cin, cout, hw, True, S, w, g_nan, y_nan, a, bb, coef, live, n_live, gp_l)
    assert torch.isfinite(gp_d).all()
    assert torch.equal(gp_l, gp_d)   # live positions and filled positions


def _tail_chain(S, cin, c3):
    """A pooled tail cin -> c3 behind a dense forward convolution of gathered points, kernel by kernel (fused._NormActConvPool)."""
    import ogc_amd.fused as fused
    nat = _native()
    idx_np = _idx(S)
    idx = torch.from_numpy(idx_np).cuda()
    g = torch.Generator().manual_seed(7 * S + c3)
    hw, dev = P * S, idx.device
    f32 = dict(dtype=torch.float32, device=dev)
    slots = nat.conv1x1_gn_slots()
    x0 = _gathered(torch.randn(B, C0, NPTS, generator=g).cuda(), idx, S)
    w2 = (torch.randn(cin, C0, generator=g) / C0 ** 0.5).cuda()
    w3 = (torch.randn(c3, cin, generator=g) / cin ** 0.5).cuda()
    gam = [(1.0 + 0.25 * torch.randn(c, generator=g)).cuda() for c in (cin, c3)]
    bet = [(0.25 * torch.randn(c, generator=g)).cuda() for c in (cin, c3)]
    grad_out = torch.randn(B, c3, P, generator=g).cuda()
    y2 = torch.empty(B, cin, P, S, **f32)
    st2 = torch.zeros(slots * B * GROUPS * 2, dtype=torch.float64, device=dev)
    nat.conv1x1_gemm_gnstats_wrapper(B, cin, C0, hw, GROUPS, w2, x0.view(B, C0, hw), y2, st2)
    y3, st3, ext, mean2, rstd2, a2, bb2 = fused._norm_act_conv_forward(y2, st2, gam[0], bet[0], w3.view(c3, cin, 1, 1), GROUPS, EPS,
                                                                       True, GROUPS, S, gam[1])
    assert ext is not None
    out = torch.empty(B, c3, P, **f32)
    arg = torch.empty(B, c3, P, dtype=torch.int32, device=dev)
    mean3, rstd3 = torch.empty(B * GROUPS, **f32), torch.empty(B * GROUPS, **f32)
    nat.group_norm_pool_extremes_wrapper(B, c3, P, S, GROUPS, EPS, True, ext[0], ext[1], gam[1], bet[1], out, arg, mean3, rstd3,
                                         st3, st3.numel() // (2 * B * GROUPS))
    coef2 = torch.empty(B, c3, 2, **f32)
    inj = torch.empty(B, c3, P, 2, **f32)
    ws = nat.group_norm_ws(B, c3, GROUPS, True, dev)
    nat.group_norm_maxpool_bwd_sparse_wrapper(B, c3, P, S, GROUPS, True, y3, gam[1], mean3, rstd3, out, arg, grad_out, coef2, inj,
                                              torch.empty(c3, **f32), torch.empty(c3, **f32), ws, ext[0])
    live, n_live = nat.live_steps_wrapper(idx)
    return dict(y2=y2, y3=y3, w3=w3, gam=gam, arg=arg, mean2=mean2, rstd2=rstd2, a2=a2, bb2=bb2, coef2=coef2, inj=inj, live=live,
                n_live=n_live, keep=_keep(idx_np, hw), hw=hw)


@pytest.mark.parametrize("S", [64, 32])
def test_pooled_list_forms_at_the_tail_width(S):
    """cin = 64, cout = 128: the instantiations the second level's tail reaches."""
    nat = _native()
    cin, c3 = 64, 128
    k = _tail_chain(S, cin, c3)
    hw, y2, y3, w3, live, n_live = k["hw"], k["y2"], k["y3"], k["w3"], k["live"], k["n_live"]
    f32 = dict(dtype=torch.float32, device=y2.device)
    mo_d, mo_l = torch.zeros(B, 2, c3, cin, **f32), torch.full((B, 2, c3, cin), 7.0, **f32)
    nat.conv1x1_wgrad_moments_pooled_wrapper(B, cin, c3, hw, True, S, y2, k["a2"], k["bb2"], y3, k["coef2"], k["inj"], mo_d)
    nat.conv1x1_wgrad_moments_pooled_live_wrapper(B, cin, c3, hw, True, S, y2, k["a2"], k["bb2"], y3, k["coef2"], k["inj"], live,
                                                  n_live, mo_l)
    c2_, c3_ = k["coef2"].double()[..., 0].view(B, c3, 1, 1), k["coef2"].double()[..., 1].view(B, c3, 1, 1)
    hit = torch.arange(S, device=y2.device).view(1, 1, 1, S) == k["arg"].long().unsqueeze(-1)
    gy3 = (c2_ * y3.double() + c3_ + hit.double() * k["inj"].double()[..., 0].unsqueeze(-1)).view(B, c3, hw)
    m2, y2_64 = _mask64(k["a2"], k["bb2"], y2, cin)
    _err("pooled moments", mo_l, mo_d, torch.stack([gy3 @ m2.transpose(1, 2), gy3 @ (m2 * y2_64).transpose(1, 2)], dim=1))

    coef = torch.empty(B, cin, 3, **f32)
    ggb = torch.zeros(2, cin, **f32)
    nat.gn_moments_combine_wrapper(B, cin, c3, hw, GROUPS, mo_d, w3, k["a2"], k["bb2"], k["mean2"], k["rstd2"], k["gam"][0],
                                   torch.empty(c3, cin, **f32), coef, ggb[0], ggb[1])
    gp_d = torch.empty(B, cin, P, S, **f32)
    gp_l = torch.full((B, cin, P, S), float("nan"), **f32)
    nat.conv1x1_dgrad_adjoint_pooled_wrapper(B, cin, c3, hw, True, S, w3, y3, k["coef2"], k["inj"], y2, k["a2"], k["bb2"], coef, gp_d)
    nat.conv1x1_dgrad_adjoint_pooled_live_wrapper(B, cin, c3, hw, True, S, w3, y3, k["coef2"], k["inj"], y2, k["a2"], k["bb2"],
                                                  coef, live, n_live, gp_l)
    keep = k["keep"].unsqueeze(1).expand(B, cin, hw)
    assert torch.isnan(gp_l.view(B, cin, hw)[~keep]).all()   # written at live positions only
    assert torch.isfinite(gp_d).all()
    assert torch.equal(gp_l.view(B, cin, hw)[keep], gp_d.view(B, cin, hw)[keep])


DEEP_WRAPPERS = ("conv1x1_wgrad_moments_pooled_live_wrapper", "conv1x1_dgrad_adjoint_pooled_live_wrapper",
                 "conv1x1_wgrad_moments_live_wrapper", "conv1x1_dgrad_adjoint_live_fill_wrapper")


def test_deep_level_with_and_without_the_list(monkeypatch):
    """One level shaped as the second of the segmentation nets: outputs bit-identical (the forward pass is untouched), parameter
    and feature gradients at the golden gradient tolerance of the segnets; with the switch on each of the four list forms runs
    once, with it off none."""
    import ogc_amd  # noqa: F401
    import ogc_amd.fused as fused
    from ogc_amd.pointnet2 import pointnet2 as api
    from ogc_amd.utils.pointnet2_util import PointnetSAModule
    torch.manual_seed(11)
    bn = {"class": "GroupNorm", "num_groups": 4}
    sa = PointnetSAModule(npoint=64, radius=4, nsample=64, mlp=[96, 64, 64, 128], bn=bn).cuda()
    xyz = ((torch.rand(2, 256, 3) - 0.5) * 16).cuda()
    feats = torch.randn(2, 96, 256).cuda().requires_grad_(True)
    probe = torch.randn(2, 128, 64).cuda()
    # the clouds give a mix: centres with one, two and more live steps of four
    geometry = sa.plan_geometry(xyz)
    assert geometry["live"][0] is not None and len(geometry["live"][0]) == 2   # (the backward list alone)
    live, n_live = geometry["live"][0]
    per_centre = torch.zeros(2, 64, dtype=torch.int64)
    for b in range(2):
        steps = (live[b, :int(n_live[b])] & ((1 << SHIFT) - 1)).cpu().long()
        per_centre[b] = torch.bincount(steps // 4, minlength=64)
    print("live steps per centre:", torch.bincount(per_centre.flatten(), minlength=5).tolist())
    assert per_centre.min() >= 1 and len(torch.unique(per_centre)) >= 2 and int(n_live.max()) < 64 * 4
    counting = _Counting(api._native, DEEP_WRAPPERS)
    monkeypatch.setattr(api, "_native", counting)
    runs = {}
    for on in (True, False):
        monkeypatch.setattr(fused, "LIVE_DEEP_LEVELS", on)
        for name in counting.calls:
            counting.calls[name] = 0
        sa.zero_grad()
        feats.grad = None
        out = sa(xyz, feats)[1]
        (out * probe).sum().backward()
        grads = {n: p.grad.clone() for n, p in sa.named_parameters()}
        grads["features"] = feats.grad.clone()
        runs[on] = (out.detach().clone(), grads, dict(counting.calls))
    assert runs[True][2] == {n: 1 for n in DEEP_WRAPPERS} and runs[False][2] == {n: 0 for n in DEEP_WRAPPERS}
    assert torch.equal(runs[True][0], runs[False][0])
    grad_rtol = 1e-3   # tests/golden_cases.py: run_segnet
    for n, g_off in runs[False][1].items():
        g_on = runs[True][1][n]
        err, scale = (g_on - g_off).abs().max().item(), g_off.abs().max().item()
        print("%-40s err %.3e  scale %.3e" % (n, err, scale))
        assert torch.isfinite(g_on).all() and err <= grad_rtol * scale + 1e-8, n


def test_switch_follows_skip_repeat_steps(monkeypatch):
    """LIVE_DEEP_LEVELS is off whenever SKIP_REPEAT_STEPS is: no list is planned for the level."""
    import ogc_amd  # noqa: F401
    import ogc_amd.fused as fused
    from ogc_amd.utils.pointnet2_util import PointnetSAModule
    torch.manual_seed(11)
    sa = PointnetSAModule(npoint=64, radius=4, nsample=64, mlp=[96, 64, 64, 128], bn={"class": "GroupNorm", "num_groups": 4}).cuda()
    xyz = ((torch.rand(2, 256, 3) - 0.5) * 16).cuda()
    monkeypatch.setattr(fused, "SKIP_REPEAT_STEPS", False)
    assert sa.plan_geometry(xyz)["live"] == [None]


def test_preconditions_are_reported():
    """Null list, nsample 16 or 48, a list without room for the worst case: an error status each, and the output keeps its fill."""
    from ogc_amd import _lib
    nat = _native()
    S, cin, cout = 64, 64, 64
    hw = P * S
    f32 = dict(dtype=torch.float32, device="cuda")
    live, n_live = nat.live_steps_wrapper(torch.from_numpy(_idx(S)).cuda())
    short = live[:, :hw // 16 - 1].contiguous()
    y_prev, grad_y, w = torch.randn(B, cin, P, S, **f32), torch.randn(B, cout, P, S, **f32), torch.randn(cout, cin, **f32)
    a, bb, coef = torch.randn(B * cin, **f32), torch.randn(B * cin, **f32), torch.randn(B, cin, 3, **f32)
    for lv, nl, ns in ((None, None, S), (live, None, S), (live, n_live, 16), (live, n_live, 48), (short, n_live, S)):
        mo, gp = torch.full((B, 2, cout, cin), 7.0, **f32), torch.full((B, cin, P, S), 7.0, **f32)
        with pytest.raises(_lib.OgcOpsError):
            nat.conv1x1_wgrad_moments_live_wrapper(B, cin, cout, hw, True, ns, y_prev, a, bb, grad_y, lv, nl, mo)
        with pytest.raises(_lib.OgcOpsError):
            nat.conv1x1_dgrad_adjoint_live_fill_wrapper(B, cin, cout, hw, True, ns, w, grad_y, y_prev, a, bb, coef, lv, nl, gp)
        assert mo.eq(7.0).all() and gp.eq(7.0).all()

"""The backward of a first level's chain (first pair -> pooled tail) over the LIVE steps of its neighbour lists only
(ogc_live_steps and the four *_live kernels of csrc/gn_fused_bwd.hip, fused.SKIP_REPEAT_STEPS): the list against a numpy
restatement of its rule; every list form against its dense form on the same inputs and against float64 sums; nothing reads a
skipped position; the forward arg-max lies in a live step; one SA level with the switch on and off; preconditions.

Bounds.  A list form and its dense form are fp32 groupings of one sum (the weighted form has fewer roundings): the list form's
error against the float64 evaluation of that sum may exceed the dense form's by at most a factor of 2.  Every case prints both
errors and their ratio."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GROUPS = 4
EPS = 1e-5
B, P, NPTS, C0, C1, C2 = 2, 12, 200, 6, 32, 32
FILLS = (1, 1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)   # (the first 1: an all-zero row)
SHIFT = 28


def _idx(S, fills=FILLS, seed=5):
    """(B, P, S) int32: row r ends in repeats of its first entry from column fill on; column fill - 1 differs from column 0,
    the columns in between are arbitrary (repeats of column 0 among them)."""
    rng = np.random.RandomState(seed + S)
    idx = np.zeros((B * P, S), dtype=np.int32)
    for r in range(B * P):
        fill = min(fills[r % len(fills)], S)
        first = 0 if r == 0 else rng.randint(NPTS)
        idx[r, :] = first
        if fill > 1:
            idx[r, 1:fill] = rng.randint(NPTS, size=fill - 1)
            idx[r, 1:fill:5] = first                                   # repeats of column 0 inside the live part
            idx[r, fill - 1] = (first + 1 + rng.randint(NPTS - 1)) % NPTS   # != first
    return idx.reshape(B, P, S)


def _rule(idx):
    """numpy restatement: per sample the ascending packed entries, and their number."""
    Bn, Pn, S = idx.shape
    T = S // 16
    lists = []
    for b in range(Bn):
        out = []
        for c in range(Pn):
            differs = np.nonzero(idx[b, c] != idx[b, c, 0])[0]
            fill = 1 + int(differs.max()) if differs.size else 1
            s_star = min(fill // 16, T - 1)
            for st in range(s_star + 1):
                out.append((c * T + st) | (((T - 1 - s_star) << SHIFT) if st == s_star else 0))
        lists.append(out)
    return lists


def _native():
    import ogc_amd  # noqa: F401
    from ogc_amd.pointnet2 import pointnet2 as api
    return api._native


@pytest.mark.parametrize("S", [64, 32, 16])
def test_list_equals_the_rule(S):
    nat = _native()
    idx = _idx(S)
    live, n_live = nat.live_steps_wrapper(torch.from_numpy(idx).cuda())
    want = _rule(idx)
    assert live.shape == (B, P * S // 16) and n_live.tolist() == [len(w) for w in want]
    for b in range(B):
        assert live[b, :len(want[b])].tolist() == want[b]
    if S == 16:   # one step per centre: all live, weight 1
        assert n_live.tolist() == [P] * B and live.tolist() == [list(range(P))] * B


def test_full_neighbourhoods_keep_every_step():
    nat = _native()
    idx = _idx(64, fills=(64,))
    live, n_live = nat.live_steps_wrapper(torch.from_numpy(idx).cuda())
    assert n_live.tolist() == [P * 4] * B and live.tolist() == [list(range(P * 4))] * B


def _err(name, new, parent, truth):
    truth = truth.double()
    e_new = (new.double() - truth).abs().max().item()
    e_par = (parent.double() - truth).abs().max().item()
    print("%-16s list %.3e  dense %.3e  ratio %.3f" % (name, e_new, e_par, e_new / e_par if e_par > 0 else float(e_new > 0)))
    assert torch.isfinite(new).all(), name
    assert e_new <= 2.0 * e_par, "%s: list-form error %.3e > 2 x dense-form error %.3e" % (name, e_new, e_par)


def _chain(S, c3):
    """The chain's forward pass and the sparse pooled gradient on hand-made neighbour lists, kernel by kernel."""
    import ogc_amd.fused as fused
    nat = _native()
    idx_np = _idx(S)
    g = torch.Generator().manual_seed(100 * S + c3)
    idx = torch.from_numpy(idx_np).cuda()
    pts = torch.randn(B, C0, NPTS, generator=g).cuda()
    x0 = torch.gather(pts.unsqueeze(2).expand(B, C0, P, NPTS), 3, idx.long().unsqueeze(1).expand(B, C0, P, S)).contiguous()
    w1 = (torch.randn(C1, C0, generator=g) / C0 ** 0.5).cuda()
    w2 = (torch.randn(C2, C1, generator=g) / C1 ** 0.5).cuda()
    w3 = (torch.randn(c3, C2, generator=g) / C2 ** 0.5).cuda()
    gam = [(1.0 + 0.25 * torch.randn(c, generator=g)).cuda() for c in (C1, C2, c3)]
    bet = [(0.25 * torch.randn(c, generator=g)).cuda() for c in (C1, C2, c3)]
    grad_out = torch.randn(B, c3, P, generator=g).cuda()
    hw, dev = P * S, x0.device
    f32 = dict(dtype=torch.float32, device=dev)
    slots = nat.conv1x1_gn_slots()
    k = dict(idx_np=idx_np, idx=idx, x0=x0, w1=w1, w2=w2, w3=w3, gam=gam, hw=hw, S=S, c3=c3)

    # first pair forwards
    st1 = torch.zeros(slots * B * GROUPS * 2, dtype=torch.float64, device=dev)
    nat.first_conv_stats_wrapper(B, C1, C0, hw, GROUPS, x0, w1, st1)
    mean1, rstd1 = torch.empty(B * GROUPS, **f32), torch.empty(B * GROUPS, **f32)
    a1, bb1 = torch.empty(B * C1, **f32), torch.empty(B * C1, **f32)
    nat.group_norm_coeffs_wrapper(B, C1, hw, GROUPS, EPS, None, gam[0], bet[0], st1, slots, None, mean1, rstd1, a1, bb1)
    y2 = torch.empty(B, C2, P, S, **f32)
    st2 = torch.zeros(slots * B * GROUPS * 2, dtype=torch.float64, device=dev)
    nat.conv1x1_gemm_affine_first_wrapper(B, C2, C1, hw, True, GROUPS, C0, w2, x0, w1, a1, bb1, y2, st2)
    y1 = torch.empty(B, C1, hw, **f32)   # (stored, for the float64 sums only)
    nat.conv1x1_gemm_gnstats_wrapper(B, C1, C0, hw, GROUPS, w1, x0.view(B, C0, hw), y1,
                                     torch.zeros(slots * B * GROUPS * 2, dtype=torch.float64, device=dev))
    k.update(mean1=mean1, rstd1=rstd1, a1=a1, bb1=bb1, y1=y1, y2=y2)

    # pooled tail forwards (fused._NormActConvPool.forward) and its sparse pooled gradient
    y3, st3, ext, mean2, rstd2, a2, bb2 = fused._norm_act_conv_forward(y2, st2, gam[1], bet[1], w3.view(c3, C2, 1, 1), GROUPS, EPS,
                                                                       True, GROUPS, S, gam[2])
    assert ext is not None
    out = torch.empty(B, c3, P, **f32)
    arg = torch.empty(B, c3, P, dtype=torch.int32, device=dev)
    mean3, rstd3 = torch.empty(B * GROUPS, **f32), torch.empty(B * GROUPS, **f32)
    nat.group_norm_pool_extremes_wrapper(B, c3, P, S, GROUPS, EPS, True, ext[0], ext[1], gam[2], bet[2], out, arg, mean3, rstd3,
                                         st3, st3.numel() // (2 * B * GROUPS))
    coef2 = torch.empty(B, c3, 2, **f32)
    inj = torch.empty(B, c3, P, 2, **f32)
    ws = nat.group_norm_ws(B, c3, GROUPS, True, dev)
    nat.group_norm_maxpool_bwd_sparse_wrapper(B, c3, P, S, GROUPS, True, y3, gam[2], mean3, rstd3, out, arg, grad_out, coef2, inj,
                                              torch.empty(c3, **f32), torch.empty(c3, **f32), ws, ext[0])
    k.update(y3=y3, arg=arg, mean2=mean2, rstd2=rstd2, a2=a2, bb2=bb2, coef2=coef2, inj=inj)
    k["live"], k["n_live"] = nat.live_steps_wrapper(idx)
    # positions of live steps
    keep = torch.zeros(B, hw, dtype=torch.bool)
    for b, entries in enumerate(_rule(idx_np)):
        for e in entries:
            st = e & ((1 << SHIFT) - 1)
            keep[b, 16 * st:16 * st + 16] = True
    k["keep"] = keep.cuda()
    return k


def _mask64(a, bb, y, c):
    """[a y + bb > 0] (the sign of the exact value is the sign of its fp32 fused multiply-add), and y, in float64."""
    y64 = y.double().view(B, c, -1)
    return ((a.double().view(B, c, 1) * y64 + bb.double().view(B, c, 1)) > 0).double(), y64


_CACHE = {}


def _checked_chain(S, c3):
    """All four list forms of one case against their dense forms (checks 2 and 3); the tensors, for the other tests."""
    if (S, c3) in _CACHE:
        return _CACHE[(S, c3)]
    nat = _native()
    k = _chain(S, c3)
    hw, dev = k["hw"], k["x0"].device
    f32 = dict(dtype=torch.float32, device=dev)
    live, n_live = k["live"], k["n_live"]
    y2, y3, w3, w2, w1, x0 = k["y2"], k["y3"], k["w3"], k["w2"], k["w1"], k["x0"]

    # ---- pooled tail: moment matrices
    mo_d, mo_l = torch.zeros(B, 2, c3, C2, **f32), torch.full((B, 2, c3, C2), 7.0, **f32)
    nat.conv1x1_wgrad_moments_pooled_wrapper(B, C2, c3, hw, True, S, y2, k["a2"], k["bb2"], y3, k["coef2"], k["inj"], mo_d)
    nat.conv1x1_wgrad_moments_pooled_live_wrapper(B, C2, c3, hw, True, S, y2, k["a2"], k["bb2"], y3, k["coef2"], k["inj"], live,
                                                  n_live, mo_l)
    c2_, c3_ = k["coef2"].double()[..., 0].view(B, c3, 1, 1), k["coef2"].double()[..., 1].view(B, c3, 1, 1)
    ag = k["inj"].double()[..., 0]
    hit = torch.arange(S, device=dev).view(1, 1, 1, S) == k["arg"].long().unsqueeze(-1)
    gy3 = (c2_ * y3.double() + c3_ + hit.double() * ag.unsqueeze(-1)).view(B, c3, hw)
    m2, y2_64 = _mask64(k["a2"], k["bb2"], y2, C2)
    _err("pooled moments", mo_l, mo_d, torch.stack([gy3 @ m2.transpose(1, 2), gy3 @ (m2 * y2_64).transpose(1, 2)], dim=1))

    # ---- pooled tail: the gradient of the pair's output, at live positions (one set of coefficients for both forms)
    coef = torch.empty(B, C2, 3, **f32)
    ggb = torch.zeros(2, C2, **f32)
    nat.gn_moments_combine_wrapper(B, C2, c3, hw, GROUPS, mo_d, w3, k["a2"], k["bb2"], k["mean2"], k["rstd2"], k["gam"][1],
                                   torch.empty(c3, C2, **f32), coef, ggb[0], ggb[1])
    gp_d = torch.empty(B, C2, P, S, **f32)
    gp_l = torch.full((B, C2, P, S), float("nan"), **f32)   # (check 3: a skipped position stays NaN)
    nat.conv1x1_dgrad_adjoint_pooled_wrapper(B, C2, c3, hw, True, S, w3, y3, k["coef2"], k["inj"], y2, k["a2"], k["bb2"], coef, gp_d)
    nat.conv1x1_dgrad_adjoint_pooled_live_wrapper(B, C2, c3, hw, True, S, w3, y3, k["coef2"], k["inj"], y2, k["a2"], k["bb2"],
                                                  coef, live, n_live, gp_l)
    cf = coef.double()
    gp_64 = (cf[..., 0].unsqueeze(-1) * m2 * (w3.double().t() @ gy3) + cf[..., 1].unsqueeze(-1) * y2_64 + cf[..., 2].unsqueeze(-1))
    keep = k["keep"].unsqueeze(1).expand(B, C2, hw)
    assert torch.isnan(gp_l.view(B, C2, hw)[~keep]).all()   # written at live positions only
    _err("g_prev (live)", gp_l.view(B, C2, hw)[keep], gp_d.view(B, C2, hw)[keep], gp_64[keep])

    # ---- first pair: moment matrices — the list form reads the buffer the pooled list form wrote (NaN wherever it did not)
    mo1_d, mo1_l = torch.zeros(B, 2, C2, C1, **f32), torch.full((B, 2, C2, C1), 7.0, **f32)
    nat.conv1x1_wgrad_moments_first_wrapper(B, C1, C2, hw, True, C0, x0, w1, k["a1"], k["bb1"], gp_d, mo1_d)
    nat.conv1x1_wgrad_moments_first_live_wrapper(B, C1, C2, hw, True, C0, S, x0, w1, k["a1"], k["bb1"], gp_l, live, n_live, mo1_l)
    m1, y1_64 = _mask64(k["a1"], k["bb1"], k["y1"], C1)
    g2 = gp_d.double().view(B, C2, hw)
    _err("first moments", mo1_l, mo1_d, torch.stack([g2 @ m1.transpose(1, 2), g2 @ (m1 * y1_64).transpose(1, 2)], dim=1))

    # ---- first pair: dW1
    coef1 = torch.empty(B, C1, 3, **f32)
    ggb1 = torch.zeros(2, C1, **f32)
    nat.gn_moments_combine_wrapper(B, C1, C2, hw, GROUPS, mo1_d, w2, k["a1"], k["bb1"], k["mean1"], k["rstd1"], k["gam"][0],
                                   torch.empty(C2, C1, **f32), coef1, ggb1[0], ggb1[1])
    dw1_d, dw1_l = torch.full((C1, C0), 7.0, **f32), torch.full((C1, C0), 7.0, **f32)
    nat.conv1x1_dgrad_adjoint_first_wrapper(B, C1, C2, hw, True, C0, w2, gp_d, x0, w1, k["a1"], k["bb1"], coef1, dw1_d)
    nat.conv1x1_dgrad_adjoint_first_live_wrapper(B, C1, C2, hw, True, C0, S, w2, gp_l, x0, w1, k["a1"], k["bb1"], coef1, live,
                                                 n_live, dw1_l)
    cf1 = coef1.double()
    g1 = cf1[..., 0].unsqueeze(-1) * m1 * (w2.double().t() @ g2) + cf1[..., 1].unsqueeze(-1) * y1_64 + cf1[..., 2].unsqueeze(-1)
    _err("dW1", dw1_l, dw1_d, torch.einsum("bmp,bcp->mc", g1, x0.double().view(B, C0, hw)))
    _CACHE[(S, c3)] = k
    return k


@pytest.mark.parametrize("S,c3", [(64, 32), (64, 64), (32, 64)])
def test_list_forms_against_dense_forms(S, c3):
    """Checks 2 and 3: moments, dW1 and g_prev at live positions; the pair's list forms fed from a NaN-filled buffer."""
    _checked_chain(S, c3)


@pytest.mark.parametrize("S,c3", [(64, 32), (64, 64), (32, 64)])
def test_forward_argmax_lies_in_a_live_step(S, c3):
    """Repeats are bit-equal and the smallest index wins a tie, so no arg-max may lie in a skipped step."""
    k = _chain(S, c3) if (S, c3) not in _CACHE else _CACHE[(S, c3)]
    arg = k["arg"].long()                                                 # (B, c3, P), column inside the neighbourhood
    assert int(arg.min()) >= 0 and int(arg.max()) < S
    pos = torch.arange(P, device=arg.device).view(1, 1, P) * S + arg
    assert k["keep"].unsqueeze(1).expand(B, c3, P * S).gather(2, pos).all()


def test_sixteen_neighbours_keep_the_dense_walk():
    """S = 16: every step is live with weight 1 (the list), and the list forms are not offered."""
    import ogc_amd.fused as fused
    nat = _native()
    idx = torch.from_numpy(_idx(16)).cuda()
    live, n_live = nat.live_steps_wrapper(idx)
    assert (live >> SHIFT).eq(0).all() and n_live.tolist() == [P] * B
    assert fused.live_steps(idx) is None
    assert not fused.LiveLink((live, n_live)).fits(B, P, 16)


class _Counting:
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


LIVE_WRAPPERS = ("conv1x1_wgrad_moments_pooled_live_wrapper", "conv1x1_dgrad_adjoint_pooled_live_wrapper",
                 "conv1x1_wgrad_moments_first_live_wrapper", "conv1x1_dgrad_adjoint_first_live_wrapper")


def test_sa_level_with_and_without_the_list(monkeypatch):
    """The first level of segnet_kitti at N = 512, B = 2 (tests/test_first_pair_gpu.py): outputs bit-identical — the forward
    pass is untouched —, parameter gradients at the golden gradient tolerance of the segnets; with the switch on both scales
    run all four list forms, with it off none."""
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
    counting = _Counting(api._native, LIVE_WRAPPERS)
    monkeypatch.setattr(api, "_native", counting)
    runs = {}
    for on in (True, False):
        monkeypatch.setattr(fused, "SKIP_REPEAT_STEPS", on)
        for name in counting.calls:
            counting.calls[name] = 0
        sa.zero_grad()
        out = sa(xyz, feats)[1]
        (out * probe).sum().backward()
        runs[on] = (out.detach().clone(), {n: p.grad.clone() for n, p in sa.named_parameters()}, dict(counting.calls))
    assert runs[True][2] == {n: 2 for n in LIVE_WRAPPERS} and runs[False][2] == {n: 0 for n in LIVE_WRAPPERS}
    assert torch.equal(runs[True][0], runs[False][0])
    grad_rtol = 1e-3   # tests/golden_cases.py: run_segnet
    for n, g_off in runs[False][1].items():
        g_on = runs[True][1][n]
        err, scale = (g_on - g_off).abs().max().item(), g_off.abs().max().item()
        print("%-40s err %.3e  scale %.3e" % (n, err, scale))
        assert torch.isfinite(g_on).all() and err <= grad_rtol * scale + 1e-8, n


def test_preconditions_are_reported():
    """Null list, bad nsample, a list without room for the worst case: an error status each, and no kernel (nor the memset in
    front of it) has run — the output keeps its fill."""
    from ogc_amd import _lib
    nat = _native()
    S, c3 = 64, 32
    hw = P * S
    f32 = dict(dtype=torch.float32, device="cuda")
    idx = torch.from_numpy(_idx(S)).cuda()
    live, n_live = nat.live_steps_wrapper(idx)
    short = live[:, :hw // 16 - 1].contiguous()
    y2, y3 = torch.randn(B, C2, P, S, **f32), torch.randn(B, c3, P, S, **f32)
    x0, w1, w2, w3 = torch.randn(B, C0, P, S, **f32), torch.randn(C1, C0, **f32), torch.randn(C2, C1, **f32), torch.randn(c3, C2, **f32)
    a2, bb2, a1, bb1 = torch.randn(B * C2, **f32), torch.randn(B * C2, **f32), torch.randn(B * C1, **f32), torch.randn(B * C1, **f32)
    coef2, inj = torch.randn(B, c3, 2, **f32), torch.zeros(B, c3, P, 2, **f32)
    coef, coef1 = torch.randn(B, C2, 3, **f32), torch.randn(B, C1, 3, **f32)
    for lv, nl, ns in ((None, None, S), (live, None, S), (live, n_live, 16), (live, n_live, 48), (short, n_live, S)):
        mo, gp = torch.full((B, 2, c3, C2), 7.0, **f32), torch.full((B, C2, P, S), 7.0, **f32)
        mo1, dw1 = torch.full((B, 2, C2, C1), 7.0, **f32), torch.full((C1, C0), 7.0, **f32)
        with pytest.raises(_lib.OgcOpsError):
            nat.conv1x1_wgrad_moments_pooled_live_wrapper(B, C2, c3, hw, True, ns, y2, a2, bb2, y3, coef2, inj, lv, nl, mo)
        with pytest.raises(_lib.OgcOpsError):
            nat.conv1x1_dgrad_adjoint_pooled_live_wrapper(B, C2, c3, hw, True, ns, w3, y3, coef2, inj, y2, a2, bb2, coef, lv, nl, gp)
        with pytest.raises(_lib.OgcOpsError):
            nat.conv1x1_wgrad_moments_first_live_wrapper(B, C1, C2, hw, True, C0, ns, x0, w1, a1, bb1, gp, lv, nl, mo1)
        with pytest.raises(_lib.OgcOpsError):
            nat.conv1x1_dgrad_adjoint_first_live_wrapper(B, C1, C2, hw, True, C0, ns, w2, gp, x0, w1, a1, bb1, coef1, lv, nl, dw1)
        for t in (mo, gp, mo1, dw1):
            assert t.eq(7.0).all()
    bad = torch.zeros(B, P, 48, dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.OgcOpsError):   # nsample not 16, 32 or 64
        nat.live_steps_wrapper(bad)

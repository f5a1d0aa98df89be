"""The GroupNorm kernels (csrc/group_norm.hip) against a float64 reference on DECIDED inputs (tests/gn_cases.py): no ReLU gate and
no arg-max of any case is within rounding of its threshold, so every tensor is compared whole — no masks, no "if unambiguous".

Tolerance, per output tensor.  The yardstick is torch's own fp32 composition on the GPU (native_group_norm, ReLU, gather at the
reference arg-max, autograd), measured against the same float64 truth:
    err_kernel <= max(4 * err_torch32, 8 * 2**-24 * max|truth|)
for the max-abs error, and for the 2-norm of the error with the floor taken per element (times sqrt(numel)); dividing both sides
by |truth|_2 gives the relative 2-norm form.  4 is the project's yardstick margin (test_fused_loss_gpu.py,
test_gn_fused_bwd_gpu.py); the floor is a few fp32 roundings of the largest element, for tensors where torch happens to be exact.
argmax must EQUAL the reference.  Every forward test also asserts max-abs error < GATE_MARGIN / 8: "decided" needs it.

Relations inside the family are bit for bit (same statistics pass, same fmaf(a, x, bb), same sums in the same order):
  maxpool_fwd            == max / first maximum over the neighbourhood of group_norm_fwd on x viewed (B, C, P * S)
  *_fwd_stats(ws, slots) == the plain call that wrote ws
  pool_extremes          == maxpool_fwd, from host-built extremes of x (exact: x is exact) and the same statistics
  maxpool_bwd_ext        == maxpool_bwd with x gathered at argmax
  maxpool_bwd_sparse     grad_gamma / grad_beta == maxpool_bwd; inj[..., 1] bits == argmax; inj[..., 0] == fp32(rstd * gamma) * gated
                         grad_out (two single multiplications); coef2 and the dense gradient rebuilt from it in float64 meet the truth
  maxpool_bwd_sparse_h   == the fp32 entry, all five outputs (x -> bf16 is exact on the lattice)

The shapes (gn_cases.PLAIN_CASES / POOLED_CASES) are the smallest that reach each launch-geometry branch; each line there names its
branch.  The plain bf16 form ogc_group_norm_bwd_h is not covered here (its output is rounded to 16 bits).
"""
import math

import numpy as np
import pytest
import torch

import gn_cases as gc

gpu = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
IDS = [gc.case_id(c) for c in gc.ALL_CASES]


@pytest.fixture(scope="module")
def nat():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    import ogc_amd  # noqa: F401  (fails loudly if libogc_ops.so is missing)
    from ogc_amd import pointnet2_cuda
    return pointnet2_cuda


# ---- the generator's guarantees (CPU) --------------------------------------------------------------------------------------------
def _first_max(act):
    m = act.max(dim=-1, keepdim=True)[0]
    pos = torch.arange(act.shape[-1], device=act.device).expand_as(act)
    return torch.where(act == m, pos, act.shape[-1]).min(dim=-1)[0]


@pytest.mark.parametrize("c", gc.ALL_CASES + [gc.STATS_PLAIN, gc.STATS_POOLED], ids=IDS + ["stats-plain", "stats-pooled"])
def test_case_is_decided(c):
    """Re-checks, with torch's own float64 group_norm, what gn_cases.make asserts: lattice values, distinct rows, the special
    channels, the gate margin of every element and the top-2 gap of every row that is no tie by construction."""
    d = gc.make(c)
    x = torch.from_numpy(d["x"])
    gamma, beta = torch.from_numpy(d["gamma"]), torch.from_numpy(d["beta"])
    cg = c.C // c.groups
    if c.data == "lattice":
        q = (x.double() - c.shift) * 8
        assert bool((q == q.round()).all()) and float(q.abs().max()) <= 255
        if not c.shift:
            assert torch.equal(x.bfloat16().float(), x)
    assert torch.equal(gamma[4::5] < 0, torch.ones_like(gamma[4::5], dtype=torch.bool))
    assert bool(((gamma.abs() >= 0.5) & (gamma.abs() <= 1.5) | (gamma == 0)).all())
    sp = gc.special_channels(c.C)
    assert bool(sp) == (c.C >= 8)
    if sp:
        assert gamma[sp[0]] == 0 and beta[sp[1]] == -40 and beta[sp[2]] == 40 and (gamma == 0).sum() == 1
    if c.const:
        b, g = gc.const_row(c)
        assert bool((x[b, g * cg:(g + 1) * cg] == 0.125).all())
    y = torch.nn.functional.group_norm(x.double().reshape(c.B, c.C, -1), c.groups, gamma.double(), beta.double(), gc.EPS)
    gate = float(y.abs().min())
    if c.relu:
        assert gate >= gc.GATE_MARGIN, gate
    gap = float("inf")
    if c.kind == "pooled":
        P, S = c.dims
        rows = x.reshape(-1, S).sort(dim=1)[0]
        distinct = (rows[:, 1:] != rows[:, :-1]).all(dim=1).reshape(c.B, c.C, P)
        y = y.reshape(c.B, c.C, P, S)
        act = torch.relu(y) if c.relu else y
        tie = torch.zeros(c.B, c.C, P, dtype=torch.bool)
        tie[:, gamma == 0] = True
        if c.relu:
            tie |= (act == 0).all(dim=3)
        if c.const:
            tie[b, g * cg:(g + 1) * cg] = True
            distinct[b, g * cg:(g + 1) * cg] = True
        assert bool(distinct.all())
        top = act.topk(2, dim=3)[0]
        gap = float((top[..., 0] - top[..., 1])[~tie].min())
        assert gap >= gc.GAP_MARGIN, gap
        assert bool(tie[:, sp[0]].all()) and (not c.relu or bool(tie[:, sp[1]].all()))     # the ties are really there
    print("%-34s min|y64| %.3e  gap %.3e" % (gc.case_id(c), gate, gap))
    assert abs(gate - d["gate"]) <= 1e-9 and (gap == d["gap"] or abs(gap - d["gap"]) <= 1e-9)


def test_reference_is_torch_group_norm():
    """gn_cases.reference against torch's float64 group_norm and its autograd (an independent route to the same truth)."""
    for c in (gc.PLAIN_CASES[1], gc.POOLED_CASES[5], gc.PLAIN_CASES[12]):
        d = gc.make(c)
        ref = gc.reference(c, d)
        x = torch.from_numpy(d["x"]).double().requires_grad_(True)
        w = torch.from_numpy(d["gamma"]).double().requires_grad_(True)
        b = torch.from_numpy(d["beta"]).double().requires_grad_(True)
        y = torch.nn.functional.group_norm(x.reshape(c.B, c.C, -1), c.groups, w, b, gc.EPS).reshape(x.shape)
        act = torch.relu(y) if c.relu else y
        if c.kind == "pooled":
            arg = _first_max(act.detach())
            assert torch.equal(arg.int(), ref["arg"])
            act = act.gather(3, arg.unsqueeze(3)).squeeze(3)
        gx, gw, gb = torch.autograd.grad((act * torch.from_numpy(d["grad"]).double()).sum(), [x, w, b])
        for name, got, want in (("y", ref["y"], act.detach()), ("dx", ref["dx"], gx), ("dgamma", ref["dgamma"], gw),
                                ("dbeta", ref["dbeta"], gb)):
            assert float((got - want).abs().max()) <= 1e-9 * max(1.0, float(want.abs().max())), (gc.case_id(c), name)


@pytest.mark.parametrize("slots", gc.STATS_SLOTS)
def test_host_partials_add_up(slots):
    for c in (gc.STATS_PLAIN, gc.STATS_POOLED):
        x = gc.make(c)["x"].astype(np.float64).reshape(c.B * c.groups, -1)
        part = gc.host_partials(c, gc.make(c)["x"], slots)
        assert part.shape == (slots, c.B * c.groups, 2)
        assert np.array_equal(part[..., 0].sum(axis=0), x.sum(axis=1))          # lattice values: exact in any grouping
        assert np.array_equal(part[..., 1].sum(axis=0), (x * x).sum(axis=1))
        assert slots == 1 or np.count_nonzero(part[:, 0, 1]) > 1


# ---- GPU helpers ------------------------------------------------------------------------------------------------------------------
def _empty(shape, off=0, dtype=torch.float32):
    """A contiguous device tensor that starts `off` elements into its buffer."""
    n = int(np.prod(shape))
    return torch.empty(n + off, dtype=dtype, device=DEV)[off:].view(shape)


def _dev(a, off=0):
    t = _empty(a.shape, off, torch.from_numpy(a[:0]).dtype)
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return t


def stats_slots(rows, row_len):
    """Slots written by the statistics pass (launch_gn_stats in csrc/group_norm.hip)."""
    chunks = 1
    while rows * chunks < 2048 and row_len // (chunks * 2) >= 16384 and chunks < 32:
        chunks *= 2
    chunk_len = (-(-row_len // chunks) + 3) // 4 * 4
    return -(-row_len // chunk_len)


class Table:
    """Per-tensor errors of kernel and yardstick; prints every line, asserts at the end."""

    def __init__(self, c):
        self.name, self.bad = gc.case_id(c), []

    def check(self, tensor, got, truth, yard):
        t = truth.double().reshape(-1)
        ek, et = got.double().reshape(-1) - t, yard.double().reshape(-1) - t
        floor = 8 * U * float(t.abs().max())
        kmax, tmax, k2, t2 = float(ek.abs().max()), float(et.abs().max()), float(ek.norm()), float(et.norm())
        nrm = max(float(t.norm()), 1e-300)
        ok = kmax <= max(4 * tmax, floor) and k2 <= max(4 * t2, floor * math.sqrt(t.numel()))
        print("%-34s %-10s max-abs %.3e (torch32 %.3e, floor %.1e)  rel-2 %.3e (torch32 %.3e)%s"
              % (self.name, tensor, kmax, tmax, floor, k2 / nrm, t2 / nrm, "" if ok else "   <-- FAILS"))
        if not ok:
            self.bad.append(tensor)
        return kmax

    def same(self, what, got, want):
        if not torch.equal(got, want):
            diff = (got != want)
            print("%-34s %-10s differs in %d of %d" % (self.name, what, int(diff.sum()), diff.numel()))
            self.bad.append(what)

    def done(self):
        assert not self.bad, (self.name, self.bad)


def yardstick(c, d, ref):
    """torch's fp32 composition on the GPU: y / out, mean, rstd, a, bb, dx, dgamma, dbeta, c2, c3."""
    B, C, G = c.B, c.C, c.groups
    cg, n = C // G, int(np.prod(c.dims))
    x = _dev(d["x"]).requires_grad_(True)
    w, b = _dev(d["gamma"]).requires_grad_(True), _dev(d["beta"]).requires_grad_(True)
    grad = _dev(d["grad"])
    y, mean, rstd = torch.native_group_norm(x.reshape(B, C, n, 1), w, b, B, C, n, G, gc.EPS)
    act = (torch.relu(y) if c.relu else y).reshape(x.shape)
    if c.kind == "pooled":
        act = act.gather(3, ref["arg"].long().unsqueeze(3)).squeeze(3)
    gx, gw, gb = torch.autograd.grad((act * grad).sum(), [x, w, b])
    mean, rstd, x, w, b = mean.detach().reshape(B, G), rstd.detach().reshape(B, G), x.detach(), w.detach(), b.detach()
    a = rstd.repeat_interleave(cg, dim=1) * w[None, :]
    bb = b[None, :] - mean.repeat_interleave(cg, dim=1) * a
    dyp = ref["dyp"].float()
    ds = ((dyp * x).reshape(B, C, -1).sum(dim=2) * w[None, :]).reshape(B, G, cg).sum(dim=2)
    db = (dyp.reshape(B, C, -1).sum(dim=2) * w[None, :]).reshape(B, G, cg).sum(dim=2)
    c2 = (db * mean - ds) * rstd * rstd * rstd / (cg * n)
    c3 = -c2 * mean - db * rstd / (cg * n)
    return dict(y=act.detach(), mean=mean, rstd=rstd, a=a, bb=bb, dx=gx, dgamma=gw, dbeta=gb, c2=c2, c3=c3)


def _forward_checks(tab, c, ref, yard, y, mean, rstd):
    err = tab.check("y", y, ref["y"], yard["y"])
    tab.check("mean", mean, ref["mean"], yard["mean"])
    tab.check("rstd", rstd, ref["rstd"], yard["rstd"])
    if err >= gc.GATE_MARGIN / 8:
        print("%-34s forward error %.3e is not below GATE_MARGIN / 8" % (tab.name, err))
        tab.bad.append("y within the gate margin")


# ---- plain GroupNorm --------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("c", gc.PLAIN_CASES, ids=IDS[:len(gc.PLAIN_CASES)])
def test_plain_truth(nat, c):
    """ogc_group_norm_fwd / _fwd_stats / _coeffs / _bwd against the float64 truth."""
    d = gc.make(c)
    ref, B, C, G, relu, off = gc.reference(c, d, DEV), c.B, c.C, c.groups, c.relu, c.offset
    hw = c.dims[0]
    yard, tab = yardstick(c, d, ref), Table(c)
    x, grad, gamma, beta = _dev(d["x"], off), _dev(d["grad"], off), _dev(d["gamma"]), _dev(d["beta"])
    assert (x.data_ptr() % 16 != 0) == bool(off)
    y, mean, rstd = _empty((B, C, hw), off), _empty((B * G,)), _empty((B * G,))
    ws = nat.group_norm_ws(B, C, G, False, DEV)
    nat.group_norm_fwd_wrapper(B, C, hw, G, gc.EPS, relu, x, gamma, beta, y, mean, rstd, ws)
    _forward_checks(tab, c, ref, yard, y, mean.view(B, G), rstd.view(B, G))
    # the statistics just written, supplied
    slots = stats_slots(B * G, (C // G) * hw)
    y2, mean2, rstd2 = _empty((B, C, hw), off), _empty((B * G,)), _empty((B * G,))
    nat.group_norm_fwd_stats_wrapper(B, C, hw, G, gc.EPS, relu, x, gamma, beta, y2, mean2, rstd2, ws, slots)
    tab.same("fwd_stats y", y2, y), tab.same("fwd_stats mean", mean2, mean), tab.same("fwd_stats rstd", rstd2, rstd)
    # the same map as coefficients, from x and from the statistics
    for stats in (None, ws):
        a, bb, mean3, rstd3 = _empty((B, C)), _empty((B, C)), _empty((B * G,)), _empty((B * G,))
        ws3 = nat.group_norm_ws(B, C, G, False, DEV)
        nat.group_norm_coeffs_wrapper(B, C, hw, G, gc.EPS, None if stats is not None else x, gamma, beta, stats,
                                      slots if stats is not None else 0, None if stats is not None else ws3, mean3, rstd3, a, bb)
        tab.check("a", a, ref["a"], yard["a"])
        tab.check("bb", bb, ref["bb"], yard["bb"])
        tab.same("coeffs mean", mean3, mean), tab.same("coeffs rstd", rstd3, rstd)
    # backward
    dx, gg, gb = _empty((B, C, hw), off), _empty((C,)), _empty((C,))
    wsb = nat.group_norm_ws(B, C, G, True, DEV)
    nat.group_norm_bwd_wrapper(B, C, hw, G, relu, x, gamma, beta, mean, rstd, grad, dx, gg, gb, wsb)
    tab.check("dx", dx, ref["dx"], yard["dx"])
    tab.check("dgamma", gg, ref["dgamma"], yard["dgamma"])
    tab.check("dbeta", gb, ref["dbeta"], yard["dbeta"])
    tab.done()


# ---- supplied statistics ----------------------------------------------------------------------------------------------------------
def host_extremes(d):
    """yext, aext as the pooled convolution records them: per neighbourhood the largest x where gamma >= 0, the smallest where
    gamma < 0, and the first position attaining it."""
    x = torch.from_numpy(d["x"])
    neg = (torch.from_numpy(d["gamma"]) < 0)[None, :, None]
    key = torch.where(neg.unsqueeze(3), -x, x)
    aext = _first_max(key)
    return x.gather(3, aext.unsqueeze(3)).squeeze(3).contiguous(), aext.int().contiguous()


@gpu
@pytest.mark.parametrize("slots", gc.STATS_SLOTS)
def test_supplied_statistics(nat, slots):
    """fwd_stats, coeffs, maxpool_fwd_stats and pool_extremes on float64 partial sums made on the host, `slots` of them: the slot
    loop of gn_mean_rstd with counts that are no multiple of 8, one more than 8, and the most the library writes."""
    c = gc.STATS_PLAIN
    d = gc.make(c)
    ref, B, C, G, hw = gc.reference(c, d, DEV), c.B, c.C, c.groups, c.dims[0]
    yard, tab = yardstick(c, d, ref), Table(c)
    x, gamma, beta = _dev(d["x"]), _dev(d["gamma"]), _dev(d["beta"])
    stats = _dev(gc.host_partials(c, d["x"], slots))
    y, mean, rstd = _empty((B, C, hw)), _empty((B * G,)), _empty((B * G,))
    nat.group_norm_fwd_stats_wrapper(B, C, hw, G, gc.EPS, c.relu, x, gamma, beta, y, mean, rstd, stats, slots)
    _forward_checks(tab, c, ref, yard, y, mean.view(B, G), rstd.view(B, G))
    a, bb, mean2, rstd2 = _empty((B, C)), _empty((B, C)), _empty((B * G,)), _empty((B * G,))
    nat.group_norm_coeffs_wrapper(B, C, hw, G, gc.EPS, None, gamma, beta, stats, slots, None, mean2, rstd2, a, bb)
    tab.check("a", a, ref["a"], yard["a"])
    tab.check("bb", bb, ref["bb"], yard["bb"])
    tab.same("coeffs mean", mean2, mean), tab.same("coeffs rstd", rstd2, rstd)
    tab.done()

    c = gc.STATS_POOLED
    d = gc.make(c)
    ref, B, C, G, (P, S) = gc.reference(c, d, DEV), c.B, c.C, c.groups, c.dims
    yard, tab = yardstick(c, d, ref), Table(c)
    x, gamma, beta = _dev(d["x"]), _dev(d["gamma"]), _dev(d["beta"])
    stats = _dev(gc.host_partials(c, d["x"], slots))
    out, arg, mean, rstd = _empty((B, C, P)), _empty((B, C, P), dtype=torch.int32), _empty((B * G,)), _empty((B * G,))
    nat.group_norm_maxpool_fwd_stats_wrapper(B, C, P, S, G, gc.EPS, c.relu, x, gamma, beta, out, arg, mean, rstd, stats, slots)
    _forward_checks(tab, c, ref, yard, out, mean.view(B, G), rstd.view(B, G))
    tab.same("argmax", arg, ref["arg"])
    yext, aext = (_dev(t.numpy()) for t in host_extremes(d))
    out2, arg2, mean2, rstd2 = _empty((B, C, P)), _empty((B, C, P), dtype=torch.int32), _empty((B * G,)), _empty((B * G,))
    nat.group_norm_pool_extremes_wrapper(B, C, P, S, G, gc.EPS, c.relu, yext, aext, gamma, beta, out2, arg2, mean2, rstd2, stats,
                                         slots)
    tab.same("extremes out", out2, out), tab.same("extremes argmax", arg2, arg)
    tab.same("extremes mean", mean2, mean), tab.same("extremes rstd", rstd2, rstd)
    tab.done()


# ---- GroupNorm + max over the neighbourhood -----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("c", gc.POOLED_CASES, ids=IDS[len(gc.PLAIN_CASES):])
def test_pooled_truth(nat, c):
    """ogc_group_norm_maxpool_fwd / _fwd_stats / _bwd / _bwd_ext / _bwd_sparse / _bwd_sparse_h and ogc_group_norm_pool_extremes."""
    d = gc.make(c)
    ref, B, C, G, relu, (P, S) = gc.reference(c, d, DEV), c.B, c.C, c.groups, c.relu, c.dims
    yard, tab = yardstick(c, d, ref), Table(c)
    x, grad, gamma, beta = _dev(d["x"]), _dev(d["grad"]), _dev(d["gamma"]), _dev(d["beta"])

    def outputs():
        return _empty((B, C, P)), _empty((B, C, P), dtype=torch.int32), _empty((B * G,)), _empty((B * G,))

    out, arg, mean, rstd = outputs()
    ws = nat.group_norm_ws(B, C, G, False, DEV)
    nat.group_norm_maxpool_fwd_wrapper(B, C, P, S, G, gc.EPS, relu, x, gamma, beta, out, arg, mean, rstd, ws)
    _forward_checks(tab, c, ref, yard, out, mean.view(B, G), rstd.view(B, G))
    tab.same("argmax", arg, ref["arg"])
    # the unpooled kernel on the same memory
    yfull, mean1, rstd1 = _empty((B, C, P * S)), _empty((B * G,)), _empty((B * G,))
    ws1 = nat.group_norm_ws(B, C, G, False, DEV)
    nat.group_norm_fwd_wrapper(B, C, P * S, G, gc.EPS, relu, x.view(B, C, P * S), gamma, beta, yfull, mean1, rstd1, ws1)
    yfull = yfull.view(B, C, P, S)
    tab.same("out = max(fwd)", out, yfull.max(dim=3)[0]), tab.same("argmax = first max(fwd)", arg, _first_max(yfull).int())
    tab.same("mean = fwd", mean, mean1), tab.same("rstd = fwd", rstd, rstd1)
    del yfull
    # supplied statistics; the extremes
    slots = stats_slots(B * G, (C // G) * P * S)
    o2, a2, m2, r2 = outputs()
    nat.group_norm_maxpool_fwd_stats_wrapper(B, C, P, S, G, gc.EPS, relu, x, gamma, beta, o2, a2, m2, r2, ws, slots)
    tab.same("fwd_stats out", o2, out), tab.same("fwd_stats argmax", a2, arg)
    tab.same("fwd_stats mean", m2, mean), tab.same("fwd_stats rstd", r2, rstd)
    yext, aext = (_dev(t.numpy()) for t in host_extremes(d))
    o3, a3, m3, r3 = outputs()
    nat.group_norm_pool_extremes_wrapper(B, C, P, S, G, gc.EPS, relu, yext, aext, gamma, beta, o3, a3, m3, r3, ws, slots)
    tab.same("extremes out", o3, out), tab.same("extremes argmax", a3, arg)
    tab.same("extremes mean", m3, mean), tab.same("extremes rstd", r3, rstd)
    # backward, dense
    dx, gg, gb = _empty((B, C, P, S)), _empty((C,)), _empty((C,))
    wsb = nat.group_norm_ws(B, C, G, True, DEV)
    nat.group_norm_maxpool_bwd_wrapper(B, C, P, S, G, relu, x, gamma, mean, rstd, out, arg, grad, dx, gg, gb, wsb)
    tab.check("dx", dx, ref["dx"], yard["dx"])
    tab.check("dgamma", gg, ref["dgamma"], yard["dgamma"])
    tab.check("dbeta", gb, ref["dbeta"], yard["dbeta"])
    x_at = x.gather(3, arg.long().unsqueeze(3)).squeeze(3).contiguous()
    dx2, gg2, gb2 = _empty((B, C, P, S)), _empty((C,)), _empty((C,))
    nat.group_norm_maxpool_bwd_ext_wrapper(B, C, P, S, G, relu, x, x_at, gamma, mean, rstd, out, arg, grad, dx2, gg2, gb2,
                                           nat.group_norm_ws(B, C, G, True, DEV))
    tab.same("bwd_ext dx", dx2, dx), tab.same("bwd_ext dgamma", gg2, gg), tab.same("bwd_ext dbeta", gb2, gb)
    del dx2
    # backward, sparse
    def sparse(xin, x_at_argmax):
        coef2, inj, g1, g2 = _empty((B, C, 2)), _empty((B, C, P, 2)), _empty((C,)), _empty((C,))
        nat.group_norm_maxpool_bwd_sparse_wrapper(B, C, P, S, G, relu, xin, gamma, mean, rstd, out, arg, grad, coef2, inj, g1, g2,
                                                  nat.group_norm_ws(B, C, G, True, DEV), x_at_argmax)
        return coef2, inj, g1, g2

    coef2, inj, gg3, gb3 = sparse(x, None)
    tab.same("sparse dgamma", gg3, gg), tab.same("sparse dbeta", gb3, gb)
    tab.same("inj arg bits", inj.view(torch.int32)[..., 1], arg)
    a32 = np.repeat(rstd.cpu().numpy().reshape(B, G), C // G, axis=1) * d["gamma"][None, :]
    assert a32.dtype == np.float32
    gated = np.where(out.cpu().numpy() > 0, d["grad"], np.float32(0)) if relu else d["grad"]
    tab.same("inj ag", inj[..., 0].cpu(), torch.from_numpy(a32[:, :, None] * gated))
    cg = C // G
    tab.check("c2", coef2[..., 0], ref["c2"].repeat_interleave(cg, dim=1), yard["c2"].repeat_interleave(cg, dim=1))
    tab.check("c3", coef2[..., 1], ref["c3"].repeat_interleave(cg, dim=1), yard["c3"].repeat_interleave(cg, dim=1))
    rebuilt = coef2[..., 0].double()[:, :, None, None] * x.double() + coef2[..., 1].double()[:, :, None, None]
    rebuilt.scatter_add_(3, arg.long().unsqueeze(3), inj[..., 0].double().unsqueeze(3))
    tab.check("dx(sparse)", rebuilt, ref["dx"], yard["dx"])
    del rebuilt
    # x at the EXTREME handed in, as the pooled convolution does: arg differs from that position only where the kernel says so
    for name, got, want in zip(("coef2", "inj", "dgamma", "dbeta"), sparse(x, yext), (coef2, inj, gg3, gb3)):
        tab.same("sparse+yext " + name, got, want)
    for name, got, want in zip(("coef2", "inj", "dgamma", "dbeta"), sparse(x.bfloat16(), None), (coef2, inj, gg3, gb3)):
        tab.same("sparse_h " + name, got, want)
    for name, got, want in zip(("coef2", "inj", "dgamma", "dbeta"), sparse(x.bfloat16(), yext), (coef2, inj, gg3, gb3)):
        tab.same("sparse_h+yext " + name, got, want)
    tab.done()

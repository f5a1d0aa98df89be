"""The BatchNorm kernels (csrc/batch_norm.hip: ogc_batch_norm_fwd / _bwd / _maxpool_fwd / _maxpool_bwd) against a float64
reference on DECIDED inputs (tests/bn_cases.py): no ReLU gate and no arg-max of any case is within rounding of its threshold, so
every tensor is compared whole — no masks, no "if unambiguous".  The twin of test_group_norm_truth_gpu.py.

Tolerance, per output tensor (test_group_norm_truth_gpu.Table).  The yardstick is torch's own fp32 composition (native_batch_norm,
ReLU, gather at the reference arg-max, autograd), measured against the same float64 truth:
    err_kernel <= max(4 * err_torch32, 8 * 2**-24 * max|truth|)
for the max-abs error, and for the 2-norm of the error with the floor taken per element.  The yardstick runs on the HOST: on the
device it is MIOpen's batch-norm backward, which has aborted the process on this stack (see test_ops_gpu.test_batch_norm_act_fused).
argmax must EQUAL the reference.  Every forward also asserts max-abs error < GATE_MARGIN / 8: "decided" needs it.  Both errors
are printed per tensor; nothing measured is written into this file.

Relations inside the family, bit for bit, on lattice cases only — there the sums of x, x * x, dy' and dy' * x are exact in fp32
groups of four and in fp64, so neither the order of the fp64 atomics nor the route to the sums can matter:
  1  maxpool_fwd out / arg / mean / rstd / running buffers == max / first maximum of batch_norm_fwd on x viewed (B, C, P * S)
  2  stats = host partial sums, slots in (1, 3, 32)         == the call that computed its own statistics
  3  evaluation with mean = rstd = None (one launch)        == the evaluation call that returns mean, rstd
  4  maxpool_bwd dgamma / dbeta == batch_norm_bwd fed the scattered gradient, BIT FOR BIT: both reduce the same exact products
     to the same two doubles and push them through the same expressions.  dx only meets the truth in both: the dense kernel
     forms fmaf(a, dy', fmaf(c2, x, c3)), the pooled one fmaf(c2, x, c3) + a * dy' — two roundings against one.
  5  deterministic mode == default mode, every output of all four entry points, on a chunked plain and a halved-grid pooled case
     (pins the slab index (z * gridDim.x + x) * 2c against the atomics)
  6  fold on / off: tests/test_bn_fold_gpu.py (child processes).

The shapes (bn_cases.PLAIN_CASES / POOLED_CASES) are the smallest that reach each launch-geometry branch; each line there names
its branch, and test_case_list_reaches_its_branches re-derives them from the launch arithmetic.  Out of scope: count == 1 (torch
itself refuses to train), non-finite inputs, and for the randn case everything but the truth / yardstick comparison.
"""
import numpy as np
import pytest
import torch

import bn_cases as bc
from test_group_norm_truth_gpu import Table as _Table, _dev, _empty

gpu = pytest.mark.gpu
DEV = "cuda"
IDS = [bc.case_id(c) for c in bc.ALL_CASES]


@pytest.fixture(scope="module")
def nat():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    import ogc_amd  # noqa: F401  (fails loudly if libogc_ops.so is missing)
    from ogc_amd import pointnet2_cuda
    return pointnet2_cuda


# ---- the generator's guarantees (CPU) --------------------------------------------------------------------------------------------
def _modes(c):
    return (True, False) if c.ev else (True,)


@pytest.mark.parametrize("c", bc.ALL_CASES + [bc.STATS_POOLED], ids=IDS + ["stats-pooled"])
def test_case_is_decided(c):
    """Re-checks, with torch's own float64 batch_norm, what bn_cases.make asserts: lattice values, distinct rows, the special
    channels, the gate margin of EVERY element and the top-2 gap of every row that is no tie by construction — in each mode the
    case is run in."""
    d = bc.make(c)
    x = torch.from_numpy(d["x"])
    gamma, beta = torch.from_numpy(d["gamma"]), torch.from_numpy(d["beta"])
    grad = torch.from_numpy(d["grad"]).double() * 16
    assert bool((grad == grad.round()).all()) and float(grad.abs().max()) <= 32 and float(grad.abs().min()) >= 1
    if c.data == "lattice":
        q = (x.double() - c.shift) * 8
        assert bool((q == q.round()).all()) and float(q.abs().max()) <= 255
    assert torch.equal(gamma[4::5] < 0, torch.ones_like(gamma[4::5], dtype=torch.bool))
    assert bool(((gamma.abs() >= 0.5) & (gamma.abs() <= 1.5) | (gamma == 0)).all())
    rv = torch.from_numpy(d["running_var"])
    assert bool(((rv >= 0.5) & (rv <= 1.5)).all()) and float(torch.from_numpy(d["running_mean"]).abs().max()) > 0
    sp = bc.special_channels(c.C)
    assert bool(sp) == (c.C >= 8)
    if sp:
        assert gamma[sp[0]] == 0 and beta[sp[1]] == -40 and beta[sp[2]] == 40 and (gamma == 0).sum() == 1
    if c.const:
        assert bool((x[:, bc.CONST_CHANNEL] == 0.125).all())
    gate, gap = float("inf"), float("inf")
    for training in _modes(c):
        y = torch.nn.functional.batch_norm(x.double().reshape(c.B, c.C, -1), torch.from_numpy(d["running_mean"]).double(),
                                           rv.double(), gamma.double(), beta.double(), training, bc.MOMENTUM, bc.EPS)
        gate = min(gate, float(y.abs().min()))
        if c.kind != "pooled":
            continue
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
            tie[:, bc.CONST_CHANNEL] = True
            distinct[:, bc.CONST_CHANNEL] = True
        assert bool(distinct.all())
        top = act.topk(2, dim=3)[0]
        gap = min(gap, float((top[..., 0] - top[..., 1])[~tie].min()))
        assert bool(tie[:, sp[0]].all()) and (not (c.relu and training) or bool(tie[:, sp[1]].all()))   # the ties are really there
    print("%-34s min|y64| %.3e  gap %.3e" % (bc.case_id(c), gate, gap))
    if c.relu:
        assert gate >= bc.GATE_MARGIN, gate
    if c.kind == "pooled":
        assert gap >= bc.GAP_MARGIN, gap
    assert abs(gate - d["gate"]) <= 1e-9 and (gap == d["gap"] or abs(gap - d["gap"]) <= 1e-9)


REFERENCE_CASES = [bc.plain(2, 8, 185, 1, ev=True), bc.plain(3, 8, 260, 0), bc.plain(2, 8, 260, 1, const=True),
                   bc.plain(2, 8, 260, 1, running=False), bc.pooled(2, 8, 257, 4, 1, ev=True), bc.pooled(2, 8, 5, 256, 1, ev=True),
                   bc.pooled(2, 8, 33, 32, 0, const=True)]


@pytest.mark.parametrize("c", REFERENCE_CASES, ids=[bc.case_id(c) for c in REFERENCE_CASES])
def test_reference_is_torch_batch_norm(c):
    """bn_cases.reference against torch's float64 batch_norm and its autograd (an independent route to the same truth), in
    training and in evaluation mode, to 1e-9 relative."""
    d = bc.make(c)
    for training in (True, False):
        ref = bc.reference(c, d, training)
        x = torch.from_numpy(d["x"]).double().requires_grad_(True)
        w = torch.from_numpy(d["gamma"]).double().requires_grad_(True)
        b = torch.from_numpy(d["beta"]).double().requires_grad_(True)
        rm, rv = torch.from_numpy(d["running_mean"]).double(), torch.from_numpy(d["running_var"]).double()
        buffers = (rm, rv) if (c.running or not training) else (None, None)
        y = torch.nn.functional.batch_norm(x.reshape(c.B, c.C, -1), *buffers, w, b, training, bc.MOMENTUM, bc.EPS).reshape(x.shape)
        act = torch.relu(y) if c.relu else y
        if c.kind == "pooled":
            arg = bc.first_max(act.detach())
            assert torch.equal(arg.int(), ref["arg"])
            act = act.gather(3, arg.unsqueeze(3)).squeeze(3)
        gx, gw, gb = torch.autograd.grad((act * torch.from_numpy(d["grad"]).double()).sum(), [x, w, b])
        xs = x.detach().reshape(c.B, c.C, -1)
        want_mean = xs.mean(dim=(0, 2)) if training else torch.from_numpy(d["running_mean"]).double()
        want_var = xs.var(dim=(0, 2), unbiased=False) if training else torch.from_numpy(d["running_var"]).double()
        for name, got, want in (("y", ref["y"], act.detach()), ("dx", ref["dx"], gx), ("dgamma", ref["dgamma"], gw),
                                ("dbeta", ref["dbeta"], gb), ("mean", ref["mean"], want_mean),
                                ("rstd", ref["rstd"], (want_var + bc.EPS).rsqrt()),
                                ("running_mean", ref["running_mean"], rm), ("running_var", ref["running_var"], rv)):
            assert got.shape == want.shape, (name, got.shape, want.shape)
            assert float((got - want).abs().max()) <= 1e-9 * max(1.0, float(want.abs().max())), (bc.case_id(c), training, name)
        changed = not torch.equal(rm, torch.from_numpy(d["running_mean"]).double())
        assert changed == bool(training and c.running)


@pytest.mark.parametrize("slots", bc.STATS_SLOTS)
def test_host_partials_add_up(slots):
    for c in (bc.STATS_PLAIN, bc.STATS_POOLED, bc.plain(2, 8, 1028, 1, shift=64.0)):
        x = np.moveaxis(bc.make(c)["x"].astype(np.float64).reshape(c.B, c.C, -1), 1, 0).reshape(c.C, -1)
        part = bc.host_partials(c, bc.make(c)["x"], slots)
        assert part.shape == (slots, c.C, 2)
        assert np.array_equal(part[..., 0].sum(axis=0), x.sum(axis=1))          # lattice values: exact in any grouping
        assert np.array_equal(part[..., 1].sum(axis=0), (x * x).sum(axis=1))
        assert slots == 1 or np.count_nonzero(part[:, 0, 1]) > 1


def bn_chunks(b, c, hw):
    """bn_chunks of csrc/batch_norm.hip."""
    chunks = 1
    while b * c * chunks < 2048 and hw // (chunks * 2) >= 4096:
        chunks *= 2
    return chunks


def pool_grids(b, c, p, s):
    """(rows per workgroup, bx before and after halving, the backward sums' bs before and after) of the pooled entry points."""
    rows = 256 // (s // 4)
    bx0 = bx = -(-p // rows)
    while bx > 1 and bx * c * b > 8192:
        bx = (bx + 1) // 2
    bs0 = bs = -(-p // 256)
    while bs > 1 and bs * c * b > 4096:
        bs = (bs + 1) // 2
    return rows, bx0, bx, bs0, bs


def test_case_list_reaches_its_branches():
    """The launch arithmetic of csrc/batch_norm.hip, replayed on the case list: every branch its comments name is there."""
    chunks = {bc.case_id(c): bn_chunks(c.B, c.C, c.dims[0]) for c in bc.PLAIN_CASES}
    assert sorted(set(chunks.values())) == [1, 2, 16, 32]
    assert [c.dims[0] % 4 for c in bc.PLAIN_CASES if bn_chunks(c.B, c.C, c.dims[0]) == 2] == [0, 2, 0]
    assert {c.misalign for c in bc.PLAIN_CASES if c.dims[0] % 4 == 0} == {"", "all", "out"}
    assert any(c.dims[0] % 4 == 0 and c.dims[0] > 1024 and bn_chunks(c.B, c.C, c.dims[0]) == 1 for c in bc.PLAIN_CASES)
    assert {c.relu for c in bc.PLAIN_CASES} == {0, 1} and any(not c.running for c in bc.PLAIN_CASES)
    grids = [pool_grids(c.B, c.C, *c.dims) for c in bc.POOLED_CASES]
    assert {256 // r for r, *_ in grids} == {1, 2, 4, 8, 16, 32, 64}                                  # every L
    assert all(bx == 2 and c.dims[0] % r == 1 for c, (r, _, bx, _, _) in zip(bc.POOLED_CASES[:14], grids))   # ragged last workgroup
    assert any(c.dims[0] == 1 for c in bc.POOLED_CASES)
    assert pool_grids(2, 1024, 300, 16) == (64, 5, 3, 2, 2) and pool_grids(2, 1024, 520, 4) == (256, 3, 3, 3, 2)
    assert bc.DET_POOLED in bc.POOLED_CASES and bc.DET_PLAIN in bc.PLAIN_CASES and bn_chunks(2, 2, 8192) == 2 and bc.DET_PLAIN.B == 2
    assert all(c in bc.ALL_CASES for c in REFERENCE_CASES + [bc.STATS_PLAIN, bc.plain(2, 8, 1028, 1, shift=64.0)])
    ev = bc.EVAL_CASES
    assert sorted((c.kind, c.dims) for c in ev) == [("plain", (185,)), ("plain", (1028,)), ("plain", (8192,)), ("pooled", (5, 256)),
                                                    ("pooled", (257, 4))]
    assert all(c.relu for c in ev)
    for c in bc.ALL_CASES:      # what the entry points accept, and the size the suite can afford
        assert c.C * int(np.prod(c.dims)) < 2 ** 31 and c.B * c.C * int(np.prod(c.dims)) <= 10 * 2 ** 20
        assert c.B * int(np.prod(c.dims)) > 1


# ---- GPU helpers ------------------------------------------------------------------------------------------------------------------
class Table(_Table):
    def __init__(self, c, mode=""):
        self.name, self.bad = bc.case_id(c) + mode, []


def yardstick(c, d, ref, training):
    """torch's fp32 composition ON THE HOST, results moved to the device: y / out, mean, rstd, the running buffers after the
    call, dx, dgamma, dbeta."""
    B, C = c.B, c.C
    x = torch.from_numpy(d["x"]).reshape(B, C, -1).clone().requires_grad_(True)
    w, b = torch.from_numpy(d["gamma"]).clone().requires_grad_(True), torch.from_numpy(d["beta"]).clone().requires_grad_(True)
    rm, rv = torch.from_numpy(d["running_mean"]).clone(), torch.from_numpy(d["running_var"]).clone()
    use = c.running or not training
    y, mean, rstd = torch.native_batch_norm(x, w, b, rm if use else None, rv if use else None, training, bc.MOMENTUM, bc.EPS)
    if not training:
        mean, rstd = rm.clone(), (rv + np.float32(bc.EPS)).rsqrt()
    act = torch.relu(y) if c.relu else y
    if c.kind == "pooled":
        act = act.reshape(d["x"].shape).gather(3, ref["arg"].cpu().long().unsqueeze(3)).squeeze(3)
    else:
        act = act.reshape(d["x"].shape)
    gx, gw, gb = torch.autograd.grad((act * torch.from_numpy(d["grad"])).sum(), [x, w, b])
    out = dict(y=act.detach(), mean=mean.detach(), rstd=rstd.detach(), running_mean=rm, running_var=rv, dx=gx.reshape(d["x"].shape),
               dgamma=gw, dbeta=gb)
    return {k: v.to(DEV) for k, v in out.items()}


def _forward_checks(tab, ref, yard, y, mean, rstd):
    err = tab.check("y", y, ref["y"], yard["y"])
    tab.check("mean", mean, ref["mean"], yard["mean"])
    tab.check("rstd", rstd, ref["rstd"], yard["rstd"])
    if err >= bc.GATE_MARGIN / 8:
        print("%-34s forward error %.3e is not below GATE_MARGIN / 8" % (tab.name, err))
        tab.bad.append("y within the gate margin")


def _backward_checks(tab, ref, yard, dx, gg, gb):
    tab.check("dx", dx, ref["dx"], yard["dx"])
    tab.check("dgamma", gg, ref["dgamma"], yard["dgamma"])
    tab.check("dbeta", gb, ref["dbeta"], yard["dbeta"])


def _running(c, d, training=True):
    if not (c.running or not training):
        return None, None
    return _dev(d["running_mean"]), _dev(d["running_var"])


def _ws(C):
    return torch.zeros(3 * C, dtype=torch.float64, device=DEV)


def _vec(C):
    return _empty((C,)), _empty((C,))


def plain_fwd(nat, c, d, x, training=True, stats=None, slots=0, lean=False, hw=None):
    """ogc_batch_norm_fwd on fresh outputs and fresh running buffers: (y, mean, rstd, running_mean, running_var)."""
    B, C = c.B, c.C
    hw = hw or c.dims[0]
    y = _empty((B, C, hw), 1 if c.misalign else 0)
    mean, rstd = (None, None) if lean else _vec(C)
    rm, rv = _running(c, d, training)
    nat.batch_norm_fwd_wrapper(B, C, hw, bc.EPS, c.relu, int(training), bc.MOMENTUM, x, _dev(d["gamma"]), _dev(d["beta"]), rm, rv, y,
                               mean, rstd, None if stats is not None else _ws(C), stats, slots)
    return y, mean, rstd, rm, rv


def pooled_fwd(nat, c, d, x, training=True, stats=None, slots=0, lean=False):
    """ogc_batch_norm_maxpool_fwd likewise: (out, arg, mean, rstd, running_mean, running_var)."""
    B, C, (P, S) = c.B, c.C, c.dims
    out, arg = _empty((B, C, P)), _empty((B, C, P), dtype=torch.int32)
    mean, rstd = (None, None) if lean else _vec(C)
    rm, rv = _running(c, d, training)
    nat.batch_norm_maxpool_fwd_wrapper(B, C, P, S, bc.EPS, c.relu, int(training), bc.MOMENTUM, x, _dev(d["gamma"]), _dev(d["beta"]),
                                       rm, rv, out, arg, mean, rstd, None if stats is not None else _ws(C), stats, slots)
    return out, arg, mean, rstd, rm, rv


def plain_bwd(nat, c, d, x, grad, mean, rstd, training=True, hw=None):
    B, C = c.B, c.C
    hw = hw or c.dims[0]
    dx, (gg, gb) = _empty((B, C, hw), 1 if c.misalign else 0), _vec(C)
    nat.batch_norm_bwd_wrapper(B, C, hw, c.relu, int(training), x, _dev(d["gamma"]), _dev(d["beta"]), mean, rstd, grad, dx, gg, gb,
                               _ws(C))
    return dx, gg, gb


def pooled_bwd(nat, c, d, x, grad, mean, rstd, out, arg, training=True):
    B, C, (P, S) = c.B, c.C, c.dims
    dx, (gg, gb) = _empty((B, C, P, S)), _vec(C)
    nat.batch_norm_maxpool_bwd_wrapper(B, C, P, S, c.relu, int(training), x, _dev(d["gamma"]), mean, rstd, out, arg, grad, dx, gg, gb,
                                       _ws(C))
    return dx, gg, gb


def _eval_checks(tab, c, d, ref, yard, mean, rstd, rm, rv):
    """Evaluation mode: the running buffers bit-unchanged, mean their copy, rstd against the truth."""
    tab.same("running_mean untouched", rm.cpu(), torch.from_numpy(d["running_mean"]))
    tab.same("running_var untouched", rv.cpu(), torch.from_numpy(d["running_var"]))
    tab.same("mean = running_mean", mean, rm)
    tab.check("rstd", rstd, ref["rstd"], yard["rstd"])


# ---- plain BatchNorm --------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("c", bc.PLAIN_CASES, ids=IDS[:len(bc.PLAIN_CASES)])
def test_plain_truth(nat, c):
    """ogc_batch_norm_fwd / _bwd against the float64 truth: training mode, and evaluation mode (both routes) where the case
    says so."""
    d = bc.make(c)
    off_in = 1 if c.misalign == "all" else 0
    x, grad = _dev(d["x"], off_in), _dev(d["grad"], off_in)
    assert (x.data_ptr() % 16 != 0) == bool(off_in) and (grad.data_ptr() % 16 != 0) == bool(off_in)
    for training in _modes(c):
        ref = bc.reference(c, d, training, DEV)
        yard, tab = yardstick(c, d, ref, training), Table(c, "" if training else " eval")
        y, mean, rstd, rm, rv = plain_fwd(nat, c, d, x, training)
        assert (y.data_ptr() % 16 != 0) == bool(c.misalign)
        if training:
            _forward_checks(tab, ref, yard, y, mean, rstd)
            if c.running:
                tab.check("run_mean", rm, ref["running_mean"], yard["running_mean"])
                tab.check("run_var", rv, ref["running_var"], yard["running_var"])
        else:
            err = tab.check("y", y, ref["y"], yard["y"])
            assert err < bc.GATE_MARGIN / 8
            _eval_checks(tab, c, d, ref, yard, mean, rstd, rm, rv)
            y1, _, _, rm1, rv1 = plain_fwd(nat, c, d, x, False, lean=True)          # relation 3: the one-launch route
            tab.same("inline y", y1, y), tab.same("inline running_mean", rm1, rm), tab.same("inline running_var", rv1, rv)
        dx, gg, gb = plain_bwd(nat, c, d, x, grad, mean, rstd, training)
        assert (dx.data_ptr() % 16 != 0) == bool(c.misalign)
        _backward_checks(tab, ref, yard, dx, gg, gb)
        tab.done()


# ---- BatchNorm + max over the neighbourhood ---------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("c", bc.POOLED_CASES, ids=IDS[len(bc.PLAIN_CASES):])
def test_pooled_truth(nat, c):
    """ogc_batch_norm_maxpool_fwd / _bwd against the float64 truth, and relations 1, 3 and 4."""
    d = bc.make(c)
    B, C, (P, S) = c.B, c.C, c.dims
    x, grad = _dev(d["x"]), _dev(d["grad"])
    for training in _modes(c):
        ref = bc.reference(c, d, training, DEV)
        yard, tab = yardstick(c, d, ref, training), Table(c, "" if training else " eval")
        out, arg, mean, rstd, rm, rv = pooled_fwd(nat, c, d, x, training)
        tab.same("argmax", arg, ref["arg"])
        if training:
            _forward_checks(tab, ref, yard, out, mean, rstd)
            tab.check("run_mean", rm, ref["running_mean"], yard["running_mean"])
            tab.check("run_var", rv, ref["running_var"], yard["running_var"])
        else:
            err = tab.check("y", out, ref["y"], yard["y"])
            assert err < bc.GATE_MARGIN / 8
            _eval_checks(tab, c, d, ref, yard, mean, rstd, rm, rv)
            o1, a1, _, _, rm1, rv1 = pooled_fwd(nat, c, d, x, False, lean=True)     # relation 3
            tab.same("inline out", o1, out), tab.same("inline argmax", a1, arg)
            tab.same("inline running_mean", rm1, rm), tab.same("inline running_var", rv1, rv)
        # relation 1: the unpooled kernel on the same memory
        yfull, mean1, rstd1, rm1, rv1 = plain_fwd(nat, c, d, x.view(B, C, P * S), training, hw=P * S)
        yfull = yfull.view(B, C, P, S)
        tab.same("out = max(fwd)", out, yfull.max(dim=3)[0]), tab.same("argmax = first max(fwd)", arg, bc.first_max(yfull).int())
        tab.same("mean = fwd", mean, mean1), tab.same("rstd = fwd", rstd, rstd1)
        tab.same("running_mean = fwd", rm, rm1), tab.same("running_var = fwd", rv, rv1)
        del yfull
        dx, gg, gb = pooled_bwd(nat, c, d, x, grad, mean, rstd, out, arg, training)
        _backward_checks(tab, ref, yard, dx, gg, gb)
        # relation 4: the dense backward fed the scattered (ungated: it gates by itself) gradient
        scattered = torch.zeros(B, C, P, S, device=DEV).scatter_(3, arg.long().unsqueeze(3), grad.unsqueeze(3))
        dx2, gg2, gb2 = plain_bwd(nat, c, d, x.view(B, C, P * S), scattered.view(B, C, P * S), mean, rstd, training, hw=P * S)
        tab.check("dx(dense)", dx2.view(B, C, P, S), ref["dx"], yard["dx"])
        tab.same("dgamma = dense bwd", gg, gg2), tab.same("dbeta = dense bwd", gb, gb2)
        tab.done()


# ---- supplied statistics ----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("slots", bc.STATS_SLOTS)
def test_supplied_statistics(nat, slots):
    """Relation 2: both forward entry points on float64 partial sums made on the host, `slots` of them (the slot loop of bn_fin),
    against the truth and, bit for bit, against the call that took its own statistics."""
    for c, fwd in ((bc.STATS_PLAIN, plain_fwd), (bc.STATS_POOLED, pooled_fwd)):
        d = bc.make(c)
        ref = bc.reference(c, d, True, DEV)
        yard, tab = yardstick(c, d, ref, True), Table(c, " slots=%d" % slots)
        x = _dev(d["x"])
        own = fwd(nat, c, d, x)
        got = fwd(nat, c, d, x, stats=_dev(bc.host_partials(c, d["x"], slots)), slots=slots)
        names = ("y", "mean", "rstd", "running_mean", "running_var") if c.kind == "plain" else \
            ("out", "argmax", "mean", "rstd", "running_mean", "running_var")
        for name, a, b in zip(names, got, own):
            tab.same("stats " + name, a, b)
        _forward_checks(tab, ref, yard, got[0], got[-4], got[-3])
        tab.check("run_mean", got[-2], ref["running_mean"], yard["running_mean"])
        tab.check("run_var", got[-1], ref["running_var"], yard["running_var"])
        if c.kind == "pooled":
            tab.same("argmax", got[1], ref["arg"])
        tab.done()


# ---- deterministic mode -------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("c", [bc.DET_PLAIN, bc.DET_POOLED], ids=[bc.case_id(bc.DET_PLAIN), bc.case_id(bc.DET_POOLED)])
def test_deterministic_mode_has_the_same_bits(nat, c):
    """Relation 5: every output of the entry points in the deterministic mode (one slab of partial sums per workgroup, summed in
    slab order) equals the default mode's (fp64 atomics) bit for bit — the sums are exact on the lattice."""
    from ogc_amd import _lib
    d = bc.make(c)
    x, grad = _dev(d["x"]), _dev(d["grad"])

    def run():
        if c.kind == "plain":
            f = plain_fwd(nat, c, d, x)
            return list(f) + list(plain_bwd(nat, c, d, x, grad, f[1], f[2]))
        f = pooled_fwd(nat, c, d, x)
        return list(f) + list(pooled_bwd(nat, c, d, x, grad, f[2], f[3], f[0], f[1]))

    before = _lib.DETERMINISTIC
    try:
        _lib.set_deterministic(False)
        fast = run()
        _lib.set_deterministic(True)
        assert _lib.load().ogc_get_deterministic() == 1
        det = run()
    finally:
        _lib.set_deterministic(before)
    torch.cuda.synchronize()
    tab = Table(c, " det")
    names = (("y", "mean", "rstd") if c.kind == "plain" else ("out", "argmax", "mean", "rstd")) + \
        ("running_mean", "running_var", "dx", "dgamma", "dbeta")
    assert len(names) == len(fast) == len(det)
    for name, a, b in zip(names, det, fast):
        tab.same(name, a, b)
    ref = bc.reference(c, d, True, DEV)       # and the mode's own results meet the truth
    yard = yardstick(c, d, ref, True)
    _forward_checks(tab, ref, yard, det[0], det[-7], det[-6])
    _backward_checks(tab, ref, yard, det[-3], det[-2], det[-1])
    tab.done()

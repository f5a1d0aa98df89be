"""The two kernel families of the MaskFormer head — csrc/small_linear.hip (ogc_small_linear_fwd / _bwd) and csrc/attention.hip
(ogc_attention_fwd / _bwd) — and the routes of ogc_amd/fused.py between them, against float64 on DECIDED inputs
(tests/head_cases.py).  tests/test_attention_gpu.py holds them to torch's fp32 result within 2e-5 of the largest element; that hides
a dropped last key of one lane's share at lk = 991, a wrong tail of the four-way unrolled dQ loop, a db that misses the zero-column
tiles of a frozen weight, a dW write that strays into another projection's rows of a packed parameter.  Here:

A  small_linear: inputs on the lattice +-{1..8}/4, every sum exact in fp32 in any order, so y, dx, dW and db EQUAL float64 — no
   tolerance.  Every case of head_cases.LIN_CASES (one factor at a time around (33, 65, 33); each edge of the 32 x 32 tiles and of
   the 64-deep slices) through the wrappers, outputs NaN-prefilled heads of larger allocations whose sentinel tails must survive,
   with and without bias, with a frozen weight (the zero-column tiles), every subset of the gradients on three cases, slices of
   packed parameters on two, no rows at all; then the autograd routes small_linear / _CrossProjections / many_rows_linear.
B  the attention core against the float64 op sequence, gated per tensor and row class by test_group_norm_truth_gpu.Table:
       err_kernel <= max(4 * err_torch32, 8 * 2**-24 * max|truth|)      (max-abs, and 2-norm with the floor per element)
   with the yardstick the same op sequence in fp32 on the host.  head_cases.att_make asserts that a key left out of a softmax, a
   query left out of dV or dK, a key left out of dQ each move a tensor by >= 32 gates.  Nothing measured from the kernels is
   written into these files.  Should a part miss: the scores are exact at D = 16, expf and the library's exp are both within 1-2
   ulp, a lane adds at most 24 terms and the butterfly 6 steps, and the dQ loop keeps four accumulators over lk / 4 terms each.
C  memory contract and isolation, bit for bit: guard bands behind every operand, batch independence, NaN in one sample or one
   head staying there.
D  the refusals of the C ABI (before any launch: NaN-prefilled outputs stay NaN) and the Python gate, which must never admit a
   shape the backward refuses.
E  multihead_attention's routes against the module in float64 on the host (yardstick: the module in fp32 on the host), the route
   asserted by the classes of the autograd nodes.
"""
import copy

import numpy as np
import pytest
import torch

import head_cases as hc
from test_group_norm_truth_gpu import Table as _Table, _dev, U

gpu = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
SENT = -12345.0
PAD = 97


@pytest.fixture(scope="module")
def nat():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    import ogc_amd  # noqa: F401  (fails loudly if libogc_ops.so is missing)
    from ogc_amd import pointnet2_cuda
    return pointnet2_cuda


class Table(_Table):
    def __init__(self, name):
        self.name, self.bad = name, []

    def nan(self, what, t):
        if not bool(torch.isnan(t).all()):
            print("%-34s %-10s is not NaN throughout" % (self.name, what))
            self.bad.append(what)


LIN_IDS = [hc.lin_id(c) for c in hc.LIN_CASES]
ATT_IDS = [hc.att_id(c) for c in hc.ATT_CASES]


# ---- the generators' guarantees and the launch arithmetic (CPU) --------------------------------------------------------------------
def test_linear_cases_are_decided():
    """lin_make's assertions on every case, and by another route: numpy's float64 products of the fp32 arrays."""
    for c in hc.LIN_CASES + [hc.Lin(1025, 8, 8), hc.Lin(4096, 8, 16), hc.Lin(15, 32, 32), hc.Lin(210, 32, 64)]:
        d = hc.lin_make(c)
        x, w, dy = d["x"].astype(np.float64), d["w"].astype(np.float64), d["dy"].astype(np.float64)
        assert not (x == 0).any() and not (w == 0).any() and not (dy == 0).any() and not (d["b"] == 0).any()
        assert np.array_equal(d["y"], np.einsum("ri,oi->ro", x, w) + d["b"]) and np.array_equal(d["dx"], np.einsum("ro,oi->ri", dy, w))
        assert np.array_equal(d["dw"], np.einsum("ro,ri->oi", dy, x)) and np.array_equal(d["db"], dy.sum(0))
        # a dropped or doubled term moves a sum by at least 1/16
        assert min(float(np.abs(a).min()) * float(np.abs(b).min()) for a, b in ((x, w), (dy, w), (dy, x))) >= 1.0 / 16
        print("%-20s max|y| %g  max|dx| %g  max|dW| %g  max|db| %g" % (
            hc.lin_id(c), np.abs(d["y"]).max(), np.abs(d["dx"]).max(), np.abs(d["dw"]).max(), np.abs(d["db"]).max()))


def test_linear_case_list_reaches_its_branches():
    """The launch arithmetic of csrc/small_linear.hip replayed on the case list: tiles of 32 x 32, slices 64 deep; the forward
    reduces over ni, the dx tiles over no, the dW tiles over r; db comes from the dW tiles of column block 0, which run with zero
    columns when the weight is frozen."""
    cases = hc.LIN_CASES
    assert len(cases) <= 30 and len(set(cases)) == len(cases)
    base = hc.LIN_BASE
    assert {c.r for c in cases if (c.ni, c.no) == (base.ni, base.no)} == set(hc.LIN_R)
    assert {c.ni for c in cases if (c.r, c.no) == (base.r, base.no)} == set(hc.LIN_NI)
    assert {c.no for c in cases if (c.r, c.ni) == (base.r, base.ni)} == set(hc.LIN_NO)
    assert {hc.Lin(1, 1, 1), hc.Lin(160, 128, 128), hc.Lin(160, 128, 384), hc.Lin(1024, 129, 33)} <= set(cases)
    g = hc.lin_launch(*base)
    assert (g["fwd_tiles"], g["dx_tiles"], g["dw_tiles"], g["db_tiles"]) == (4, 6, 6, 2) and g["edge"] == (1, 1, 1)
    tiles = lambda n: hc.divup(n, hc.SL_T)  # noqa: E731
    assert [tiles(r) for r in hc.LIN_R] == [1, 1, 1, 2, 3, 5, 32]                      # row blocks: ragged, full, one row over
    assert [tiles(n) for n in hc.LIN_NI] == [1, 2, 2, 3, 4, 5] and [tiles(n) for n in hc.LIN_NO] == [1, 1, 1, 2, 5, 12]
    by_ni = {c.ni: hc.lin_launch(*c) for c in cases if (c.r, c.no) == (base.r, base.no)}
    assert [(by_ni[n]["fwd_slices"], by_ni[n]["fwd_last"]) for n in hc.LIN_NI] == [(1, 1), (1, 63), (1, 64), (2, 1), (2, 64), (3, 1)]
    by_no = {c.no: hc.lin_launch(*c) for c in cases if (c.r, c.ni) == (base.r, base.ni)}
    assert [by_no[n]["dx_slices"] for n in hc.LIN_NO] == [1, 1, 1, 1, 3, 6]
    by_r = {c.r: hc.lin_launch(*c) for c in cases if (c.ni, c.no) == (base.ni, base.no)}
    assert [by_r[r]["dw_slices"] for r in hc.LIN_R] == [1, 1, 1, 1, 2, 3, 16]
    assert hc.lin_launch(1, 1, 1)["fwd_tiles"] == 1 and hc.lin_launch(1024, 129, 33)["dx_tiles"] == 32 * 5
    # the gradient subsets: a frozen weight keeps the dW tiles (zero columns, db only); no parameter gradient drops them
    frozen, none = hc.lin_launch(*base, dx=True, dw=False, db=True), hc.lin_launch(*base, dx=True, dw=False, db=False)
    assert frozen["zero_columns"] and frozen["dw_tiles"] == 6 and none["dw_tiles"] == 0 and not none["zero_columns"]
    assert hc.lin_launch(*base, dx=False)["dx_tiles"] == 0
    assert len(hc.LIN_SUBSET_CASES) == 3 and len(hc.LIN_PACKED_CASES) == 2 and len(SUBSETS) == 7
    assert set(hc.LIN_PACKED_CASES) <= set(cases) and {c.r for c in hc.LIN_SUBSET_CASES} == {1, 33}


def _left_out(c, d):
    """The conditions of head_cases.att_make by another route: torch float64, the key or query really left out and the tensor
    recomputed.  -> {condition: smallest movement in gates}."""
    t = lambda a: torch.from_numpy(a).double().view(c.B, -1, c.H, c.D).transpose(1, 2)  # noqa: E731
    qh, kh, vh, doh = t(d["q"]), t(d["k"]), t(d["v"]), t(d["do"])
    scale, gates, flat = hc.att_scale(c.D), d["gates"], torch.from_numpy(hc.flat_rows(c.Lq))
    s = scale * (qh @ kh.transpose(2, 3))
    P = s.softmax(-1)
    dP = doh @ vh.transpose(2, 3)
    dS = P * (dP - (P * dP).sum(-1, keepdim=True))
    m = {}
    if c.Lk > 1:
        hole = torch.zeros(c.Lk, c.Lk, dtype=torch.float64)
        hole.fill_diagonal_(float("-inf"))
        without = (s[:, :, 0, None, :] + hole).softmax(-1) @ vh                          # (B, H, n left out, D)
        m["fwd"] = float((without - (P[:, :, 0:1] @ vh)).abs().amax(-1).min() / gates["out flat"][0])
    dv, dk, dq = P.transpose(2, 3) @ doh, scale * dS.transpose(2, 3) @ qh, scale * dS @ kh
    keep = lambda n, i: (torch.arange(n) != i).double()  # noqa: E731
    m["dv_cover"] = min(float(((P * keep(c.Lq, i)[:, None]).transpose(2, 3) @ doh - dv).abs().amax((2, 3)).min())
                        for i in range(c.Lq)) / gates["dv"][0]
    if c.Lk > 1:
        m["dk_cover"] = min(float((scale * (dS * keep(c.Lq, i)[:, None]).transpose(2, 3) @ qh - dk).abs().amax((2, 3)).min())
                            for i in range(c.Lq)) / gates["dk"][0]
        m["dq_cover"] = min(float(((scale * (dS * keep(c.Lk, i)) @ kh - dq)[:, :, flat]).abs().amax((2, 3)).min())
                            for i in range(c.Lk)) / gates["dq flat"][0]
    return m


@pytest.mark.parametrize("c", hc.ATT_CASES + [hc.OVER_CASE], ids=ATT_IDS + [hc.att_id(hc.OVER_CASE)])
def test_attention_case_is_decided(c):
    """att_make's assertions, and its measured conditions against the literal ones (a key or a query really left out)."""
    d = hc.att_make(c)
    flat = hc.flat_rows(c.Lq)
    for key, bound in (("k", 1), ("v", 2), ("q", 4)):
        assert bool((d[key] * 4 == np.rint(d[key] * 4)).all()) and float(np.abs(d[key]).max()) <= bound
    assert float(np.abs(d["q"][:, flat]).max()) <= 1 and flat[0] and int(flat.sum()) == (c.Lq + 2) // 3
    mine = {key: d[key] for key in ("fwd", "dv_cover", "dk_cover", "dq_cover") if key in d}
    print("%-30s %s" % (hc.att_id(c), "  ".join("%s %.3g" % kv for kv in mine.items())))
    print("%-30s %s" % ("", "  ".join("%s %.2e (torch32 %.2e)" % (k, g, e) for k, (g, e) in d["gates"].items())))
    assert set(mine) == ({"dv_cover"} if c.Lk == 1 else {"fwd", "dv_cover", "dk_cover", "dq_cover"})
    for key, v in mine.items():
        assert v >= hc.COVER or (key == "dq_cover" and c.Lq < 10), (key, v)
    if c.Lq * c.Lk <= 20000 and c.Lk <= 300:
        for key, v in _left_out(c, d).items():
            assert abs(v - mine[key]) <= 1e-6 * mine[key], (key, v, mine[key])


def test_attention_case_list_reaches_its_branches():
    """The launch arithmetic of csrc/attention.hip replayed on the case list.  Forward: one wavefront per (sample, head, query),
    four per workgroup, lane l takes keys l, l + 64, ...  Backward: one workgroup of 256 per (sample, head), a thread per key with
    stride 256, dsum with stride 256 over the queries, the lq * D loops with stride 256, dQ four keys at a time with a tail; LDS
    4 * (2 lq D + round4(lq) + lq lk) bytes, at most 64 KiB."""
    cases = hc.ATT_CASES
    assert len(cases) <= 40 and len(set(cases)) == len(cases)
    assert set(hc.ATT_LK) <= {c.Lk for c in cases} and set(hc.ATT_LQ) <= {c.Lq for c in cases}
    assert {c.D for c in cases} == {16, 32} and {c.H for c in cases} == {1, 2, 8} and {c.B for c in cases} == {1, 3}
    assert {(c.layout, c.D) for c in cases} == {(lay, D) for lay in hc.LAYOUTS for D in (16, 32)}
    fwd = {c: hc.att_fwd_launch(c.B, c.H, c.Lq, c.Lk) for c in cases}
    bwd = {c: hc.att_bwd_launch(c.B, c.H, c.D, c.Lq, c.Lk) for c in cases}
    assert any(g["items"] == 1 and g["idle_waves"] == 3 for g in fwd.values())
    assert {g["idle_waves"] for g in fwd.values()} == {0, 1, 2, 3}
    by_lk = {c.Lk: g for c, g in fwd.items()}
    assert [by_lk[n]["idle_lanes"] for n in (1, 2, 3, 4, 5, 63, 64, 65)] == [63, 62, 61, 60, 59, 1, 0, 0]
    assert [by_lk[n]["steps"] for n in (63, 64, 65, 127, 128, 129, 255, 256, 257, 991, 1500)] == [1, 1, 2, 2, 2, 3, 4, 4, 5, 16, 24]
    assert [by_lk[n]["ragged"] for n in (64, 65, 128, 129, 256, 257)] == [False, True, False, True, False, True]
    assert by_lk[65]["share"][:2] == [2, 1] and by_lk[991]["share"][30:32] == [16, 15] and by_lk[1500]["share"][27:29] == [24, 23]
    by_lk = {c.Lk: g for c, g in bwd.items()}
    assert [(by_lk[n]["key_passes"], by_lk[n]["key_last"]) for n in (255, 256, 257, 991, 1500)] == \
        [(1, 255), (1, 256), (2, 1), (4, 223), (6, 220)]
    assert [(by_lk[n]["quads"], by_lk[n]["tail"]) for n in (1, 2, 3, 4, 5, 63, 64, 65)] == \
        [(0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (15, 3), (16, 0), (16, 1)]
    assert {g["tail"] for g in bwd.values()} == {0, 1, 2, 3}
    assert {g["dsum_passes"] for c, g in bwd.items() if c.Lq == 257} == {2} and {g["dsum_passes"] for c, g in bwd.items() if c.Lq < 257} == {1}
    for D, below, at, above in ((16, 9, 16, 17), (32, 5, 8, 9)):                              # lq * D straddles 256
        ld = {c.Lq: (g["ld_passes"], g["ld_tail"]) for c, g in bwd.items() if c.D == D}
        assert ld[below][0] == 1 and ld[below][1] and ld[at] == (1, 0) and ld[above][0] == 2 and ld[above][1] in (16, 32)
    assert all(g["lds"] <= hc.AT_LDS for g in bwd.values())
    assert hc.LIMIT_CASE in cases and bwd[hc.LIMIT_CASE]["lds"] == hc.AT_LDS == 65536
    assert hc.att_lds(hc.OVER_CASE.Lq, hc.OVER_CASE.Lk, hc.OVER_CASE.D) > hc.AT_LDS and hc.OVER_CASE not in cases
    assert any((c.Lq, c.Lk, c.D) == (10, 1500, 16) for c in cases)
    assert hc.gate_admits(*hc.GATE_LIMIT) and not hc.gate_admits(16, 991, 16)
    # the contract cases: one cross, one self, B = 3, lk no multiple of 64, two heads to tell apart
    assert [c.layout for c in hc.CONTRACT_CASES] == ["cross", "self"] and set(hc.CONTRACT_CASES) <= set(cases)
    assert all(c.B == 3 and c.Lk % 64 and c.H == 2 for c in hc.CONTRACT_CASES)
    # what the suite can afford: no shape beyond those listed
    assert all(c.B * c.H * c.Lq * c.Lk <= 8 * 10 * 1500 and c.Lq <= 257 and c.Lk <= 1500 for c in cases)


def test_python_gate_never_admits_a_refused_backward(monkeypatch):
    """fused.attention_core_available over lq in 1..300, lk in 1..2000 at both head widths against attn_bwd_lds: whatever the gate
    admits fits the workgroup's 64 KiB; the gate's own LDS clause is the one written out in head_cases.gate_admits."""
    import ogc_amd  # noqa: F401
    from ogc_amd import fused, pointnet2_cuda
    from ogc_amd.pointnet2 import pointnet2 as api
    monkeypatch.setattr(api, "_native", pointnet2_cuda)             # (an earlier test of the process may have left the CPU oracle there)
    gate = fused.attention_core_available.__wrapped__               # (the function under its miss counter: nothing is counted)
    lks = np.arange(1, 2001)
    admitted = 0
    for d in (16, 32):
        for lq in range(1, 301):
            fits = hc.att_lds(lq, lks, d) <= hc.AT_LDS
            got = np.array([bool(gate(2 * d, 2, lq, lk)) for lk in range(1, 2001)])
            assert not (got & ~fits).any(), (lq, d, int(lks[got & ~fits][0]))
            assert np.array_equal(got, hc.gate_admits(lq, lks, d)), (lq, d)
            admitted += int(got.sum())
    assert 0 < admitted < 600 * 2000
    assert gate(16, 1, *hc.GATE_LIMIT[:2]) and not gate(16, 1, 16, 991) and not gate(64, 8, 5, 5) and U == hc.U


# ---- GPU helpers ------------------------------------------------------------------------------------------------------------------
def guarded(shape, pad=PAD):
    """-> (a contiguous NaN-filled tensor that is the head of a larger allocation, the sentinel-filled tail)."""
    n = int(np.prod(shape))
    big = torch.full((n + pad,), SENT, device=DEV)
    big[:n] = NAN
    return big[:n].view(shape), big[n:]


def survived(tab, what, tail):
    tab.same(what + " sentinel", tail, torch.full_like(tail, SENT))


# ---- A. small_linear ------------------------------------------------------------------------------------------------------------------
SUBSETS = [(dx, dw, db) for dx in (1, 0) for dw in (1, 0) for db in (1, 0) if dx or dw or db]


def _lin_forward(nat, tab, d, x, w, b, label):
    want = torch.from_numpy(d["y"] if b is not None else d["y0"])
    y, tail = guarded(want.shape)
    nat.small_linear_fwd_wrapper(x, w, b, y)
    torch.cuda.synchronize()
    tab.same(label, y.cpu(), want)
    survived(tab, label, tail)


def _lin_backward(nat, tab, c, d, x, w, dy, subset, label):
    outs = [guarded(s) if on else (None, None) for on, s in zip(subset, ((c.r, c.ni), (c.no, c.ni), (c.no,)))]
    nat.small_linear_bwd_wrapper(x, w, dy, outs[0][0], outs[1][0], outs[2][0])
    torch.cuda.synchronize()
    for name, (got, tail) in zip(("dx", "dw", "db"), outs):
        if got is not None:
            tab.same("%s %s" % (label, name), got.cpu(), torch.from_numpy(d[name]))
            survived(tab, "%s %s" % (label, name), tail)


@gpu
@pytest.mark.parametrize("c", hc.LIN_CASES, ids=LIN_IDS)
def test_small_linear_exact(nat, c):
    """ogc_small_linear_fwd / _bwd equal float64 bit for bit: with and without a bias, with a frozen weight (db from the zero-column
    tiles), every subset of the gradients on three cases; outputs are NaN-prefilled heads of larger allocations."""
    d, tab = hc.lin_make(c), Table(hc.lin_id(c))
    x, w, b, dy = (_dev(d[k]) for k in ("x", "w", "b", "dy"))
    _lin_forward(nat, tab, d, x, w, b, "y")
    _lin_forward(nat, tab, d, x, w, None, "y no bias")
    for subset in (SUBSETS if c in hc.LIN_SUBSET_CASES else [(1, 1, 1), (1, 1, 0), (1, 0, 1)]):
        _lin_backward(nat, tab, c, d, x, w, dy, subset, "bwd" + "".join(map(str, subset)))
    tab.done()


@gpu
@pytest.mark.parametrize("c", hc.LIN_PACKED_CASES, ids=[hc.lin_id(c) for c in hc.LIN_PACKED_CASES])
def test_small_linear_packed_parameters(nat, c):
    """What _CrossProjections does: W[:no] of a (3 no, ni) parameter, gradients into gw[:no] and gb[:no] of packed buffers.  The
    other projections' rows keep their sentinel; their weights (1e3) would show in y and dx."""
    d, tab = hc.lin_make(c), Table(hc.lin_id(c) + " packed")
    x, dy = _dev(d["x"]), _dev(d["dy"])
    w3 = torch.full((3 * c.no, c.ni), 1e3, device=DEV)
    b3 = torch.full((3 * c.no,), 1e3, device=DEV)
    w3[:c.no], b3[:c.no] = _dev(d["w"]), _dev(d["b"])
    _lin_forward(nat, tab, d, x, w3[:c.no], b3[:c.no], "y")
    gw3, gb3 = torch.full((3 * c.no, c.ni), SENT, device=DEV), torch.full((3 * c.no,), SENT, device=DEV)
    gw3[:c.no], gb3[:c.no] = NAN, NAN
    dx, tail = guarded((c.r, c.ni))
    nat.small_linear_bwd_wrapper(x, w3[:c.no], dy, dx, gw3[:c.no], gb3[:c.no])
    torch.cuda.synchronize()
    tab.same("dx", dx.cpu(), torch.from_numpy(d["dx"])), survived(tab, "dx", tail)
    tab.same("dw", gw3[:c.no].cpu(), torch.from_numpy(d["dw"])), survived(tab, "other rows of gw", gw3[c.no:])
    tab.same("db", gb3[:c.no].cpu(), torch.from_numpy(d["db"])), survived(tab, "other rows of gb", gb3[c.no:])
    tab.done()


@gpu
def test_small_linear_no_rows(nat):
    """rows = 0: the parameter gradients are zero (and nothing behind them is touched); the forward has nothing to write."""
    ni, no, tab = 65, 33, Table("lin-0x65x33")
    x, dy, w = torch.empty(0, ni, device=DEV), torch.empty(0, no, device=DEV), _dev(hc.lin_make(hc.LIN_BASE)["w"])
    (gw, gw_tail), (gb, gb_tail), (y, y_tail) = guarded((no, ni)), guarded((no,)), guarded((0, no))
    nat.small_linear_fwd_wrapper(x, w, None, y)
    nat.small_linear_bwd_wrapper(x, w, dy, None, gw, gb)
    torch.cuda.synchronize()
    tab.same("dw", gw, torch.zeros_like(gw)), tab.same("db", gb, torch.zeros_like(gb))
    survived(tab, "dw", gw_tail), survived(tab, "db", gb_tail), survived(tab, "y", y_tail)
    tab.done()


def _node_names(t):
    """Class names of every autograd node below t."""
    names, seen, stack = set(), set(), [t.grad_fn]
    while stack:
        f = stack.pop()
        if f is not None and f not in seen:
            seen.add(f)
            names.add(type(f).__name__)
            stack += [g for g, _ in f.next_functions]
    return names


def _leaf(a):
    return _dev(a).requires_grad_(True)


@gpu
def test_linear_routes_exact(nat):
    """small_linear (the kernels up to 1024 rows, the library beyond), _CrossProjections and many_rows_linear through autograd on
    lattice inputs: every output and gradient equals float64 (the library's fp32 sums are exact on these inputs too), and each
    route is the one its node classes name."""
    from ogc_amd.fused import _CrossProjections, many_rows_linear, small_linear
    tab = Table("linear routes")

    def run(fn, c, shape, route, bias=True):
        d = hc.lin_make(c)
        x, w, b = _leaf(d["x"].reshape(shape + (c.ni,))), _leaf(d["w"]), _leaf(d["b"]) if bias else None
        y = fn(x, w, b)
        assert type(y.grad_fn).__name__ == route or (route is None and "_SmallLinearBackward" not in _node_names(y)), y.grad_fn
        y.backward(_dev(d["dy"].reshape(shape + (c.no,))))
        name = "%s %s" % (hc.lin_id(c), route or "library")
        tab.same(name + " y", y.detach().cpu().reshape(c.r, c.no), torch.from_numpy(d["y"] if bias else d["y0"]))
        tab.same(name + " dx", x.grad.cpu().reshape(c.r, c.ni), torch.from_numpy(d["dx"]))
        tab.same(name + " dw", w.grad.cpu(), torch.from_numpy(d["dw"]))
        if bias:
            tab.same(name + " db", b.grad.cpu(), torch.from_numpy(d["db"]))

    run(small_linear, hc.Lin(160, 128, 128), (16, 10), "_SmallLinearBackward")
    run(small_linear, hc.Lin(160, 128, 384), (16, 10), "_SmallLinearBackward", bias=False)
    run(small_linear, hc.Lin(1024, 129, 33), (1024,), "_SmallLinearBackward")              # the last row count of the kernels
    run(small_linear, hc.Lin(1025, 8, 8), (1025,), None)                                     # one more: the library
    run(many_rows_linear, hc.Lin(4096, 8, 16), (2, 2048), "_ManyRowsLinearBackward")       # B = 2, B * L = 4096
    run(many_rows_linear, hc.Lin(160, 128, 128), (16, 10), "_SmallLinearBackward")         # few rows: on to small_linear
    # _CrossProjections: E = 32, 15 query rows, 3 x 70 memory rows, one packed (96, 32) parameter
    E, cq, ck = 32, hc.Lin(15, 32, 32), hc.Lin(210, 32, 64)
    dq, dk = hc.lin_make(cq), hc.lin_make(ck)
    query, memory = _leaf(dq["x"].reshape(3, 5, E)), _leaf(dk["x"].reshape(3, 70, E))
    W, b = _leaf(np.concatenate([dq["w"], dk["w"]])), _leaf(np.concatenate([dq["b"], dk["b"]]))
    q, kv = _CrossProjections.apply(query, memory, W, b)
    assert type(q.grad_fn).__name__ == type(kv.grad_fn).__name__ == "_CrossProjectionsBackward"
    torch.autograd.backward([q, kv], [_dev(dq["dy"].reshape(3, 5, E)), _dev(dk["dy"].reshape(3, 70, 2 * E))])
    for name, got, want in (("q", q.detach().reshape(15, E), dq["y"]), ("kv", kv.detach().reshape(210, 2 * E), dk["y"]),
                            ("dquery", query.grad.reshape(15, E), dq["dx"]), ("dmemory", memory.grad.reshape(210, E), dk["dx"]),
                            ("dW", W.grad, np.concatenate([dq["dw"], dk["dw"]])), ("db", b.grad, np.concatenate([dq["db"], dk["db"]]))):
        tab.same("_CrossProjections " + name, got.cpu(), torch.from_numpy(want))
    tab.done()


# ---- B. the attention core --------------------------------------------------------------------------------------------------------------
def layout_spec(c, packed_dq=False):
    """{operand: (buffer, width of the buffer's rows, first column)} for the operands and, with packed_dq, a dq that is the first
    third of a packed (B, Lq, 3E) gradient whose other thirds nothing may touch."""
    E = c.H * c.D
    if c.layout == "cross":
        return {"q": ("q", 3 * E if packed_dq else E, 0), "k": ("kv", 2 * E, 0), "v": ("kv", 2 * E, E)}
    if c.layout == "self":
        return {"q": ("qkv", 3 * E, 0), "k": ("qkv", 3 * E, E), "v": ("qkv", 3 * E, 2 * E)}
    return {"q": ("q", E + 8, 4), "k": ("k", E + 8, 4), "v": ("v", E + 8, 4)}


class Operands:
    """q, k, v of a case in its layout on the device (spare columns NaN, `pad` guard rows behind every buffer) and dq, dk, dv as
    NaN-filled slices of the same kind of sentinel-filled buffers."""

    def __init__(self, c, d, pad=0, packed_dq=False):
        E = c.H * c.D
        self.c, self.view, self.grad, self.bufs, self.gbufs, self.live, self.tails = c, {}, {}, {}, {}, {}, {}
        for (name, (buf, width, off)), (_, (gbuf, gwidth, goff)) in zip(layout_spec(c).items(), layout_spec(c, packed_dq).items()):
            L = c.Lq if name == "q" else c.Lk
            n = c.B * L
            if buf not in self.bufs:
                self.bufs[buf] = torch.full((n + pad, width), NAN, device=DEV)
                self.gbufs[gbuf] = torch.full((n + pad, gwidth), SENT, device=DEV)
                self.live[gbuf] = torch.zeros(n + pad, gwidth, dtype=torch.bool, device=DEV)
            self.view[name] = self.bufs[buf][:n].view(c.B, L, width)[:, :, off:off + E]
            self.view[name].copy_(torch.from_numpy(d[name]))
            self.tails[name] = self.bufs[buf][n:, off:off + E]
            self.grad[name] = self.gbufs[gbuf][:n].view(c.B, L, gwidth)[:, :, goff:goff + E]
            self.grad[name].fill_(NAN)
            self.live[gbuf][:n, goff:goff + E] = True

    def untouched(self, tab):
        """Everything of the gradient buffers outside dq, dk, dv: spare columns, other thirds, guard rows."""
        for name, buf in self.gbufs.items():
            rest = buf[~self.live[name]]
            tab.same("around d" + name, rest, torch.full_like(rest, SENT))


def run_attention(nat, c, d, pad=0, packed_dq=False, backward=True, tails=None):
    """ogc_attention_fwd and _bwd through the wrappers -> ({tensor: device result}, the Operands, [(name, sentinel tail)])."""
    ops = Operands(c, d, pad, packed_dq)
    for name, value in (tails or {}).items():
        ops.tails[name].copy_(value)
    E, scale = c.H * c.D, hc.att_scale(c.D)
    (out, out_tail), (prob, prob_tail), (do, _) = guarded((c.B, c.Lq, E), pad), guarded((c.B, c.H, c.Lq, c.Lk), pad), \
        guarded((c.B, c.Lq, E), pad)
    do.copy_(torch.from_numpy(d["do"]))
    q, k, v = ops.view["q"], ops.view["k"], ops.view["v"]
    nat.attention_fwd_wrapper(c.H, scale, q, k, v, out, prob)
    res = dict(out=out, prob=prob)
    if backward:
        nat.attention_bwd_wrapper(c.H, scale, q, k, v, out, prob, do, ops.grad["q"], ops.grad["k"], ops.grad["v"])
        res.update(dq=ops.grad["q"], dk=ops.grad["k"], dv=ops.grad["v"])
    torch.cuda.synchronize()
    return res, ops, [("out", out_tail), ("prob", prob_tail)]


def check_truth(tab, c, d, res, names=hc.TENSORS):
    for name in names:
        got = res[name].cpu()
        assert got.shape == d["truth"][name].shape
        for (label, g), (_, t), (_, y) in zip(hc.att_parts(c, name, got), hc.att_parts(c, name, d["truth"][name]),
                                              hc.att_parts(c, name, d["yard"][name])):
            tab.check(label, g, t, y)


@gpu
@pytest.mark.parametrize("c", hc.ATT_CASES, ids=ATT_IDS)
def test_attention_truth(nat, c):
    """ogc_attention_fwd / _bwd in the case's layout against the float64 truth: out, prob, dq per row class, dk, dv; every output
    starts as NaN; what surrounds dq, dk, dv in their buffers keeps its sentinel."""
    d, tab = hc.att_make(c), Table(hc.att_id(c))
    res, ops, tails = run_attention(nat, c, d, pad=PAD)
    check_truth(tab, c, d, res)
    if c.Lk == 1:                                                    # identically zero, and the kernel's arithmetic gives exact zeros
        tab.same("dq = 0", res["dq"], torch.zeros_like(res["dq"])), tab.same("dk = 0", res["dk"], torch.zeros_like(res["dk"]))
    ops.untouched(tab)
    for name, tail in tails:
        survived(tab, name, tail)
    tab.done()


# ---- C. memory contract and isolation ---------------------------------------------------------------------------------------------------
CONTRACT_IDS = [hc.att_id(c) for c in hc.CONTRACT_CASES]


@gpu
@pytest.mark.parametrize("c", hc.CONTRACT_CASES, ids=CONTRACT_IDS)
def test_attention_guard_bands(nat, c):
    """Every operand is the head of a larger allocation.  Behind k lie rows 64 * q of the last query, which would dominate its
    softmax, behind v rows of 1e3; behind every output a sentinel; the cross case's dq is the first third of a packed gradient.
    The results equal the plain run bit for bit and meet the truth; nothing around the outputs changes."""
    d, tab = hc.att_make(c), Table(hc.att_id(c) + " guard")
    plain, _, _ = run_attention(nat, c, d)
    last_q = torch.from_numpy(d["q"][-1, -1]).to(DEV)
    loud = {"k": (64 * last_q).expand(PAD, -1), "v": torch.full((PAD, c.H * c.D), 1e3, device=DEV),
            "q": torch.full((PAD, c.H * c.D), 7.0, device=DEV)}
    res, ops, tails = run_attention(nat, c, d, pad=PAD, packed_dq=c.layout == "cross", tails=loud)
    check_truth(tab, c, d, res)
    for name in hc.TENSORS:
        tab.same(name + " = plain", res[name], plain[name])
    ops.untouched(tab)
    for name, tail in tails:
        survived(tab, name, tail)
    tab.done()


@gpu
@pytest.mark.parametrize("c", hc.CONTRACT_CASES, ids=CONTRACT_IDS)
def test_attention_batch_independence(nat, c):
    """Each sample alone equals its slice of the batched call, bit for bit."""
    d = hc.att_make(c)
    together, _, _ = run_attention(nat, c, d)
    for i in range(c.B):
        alone, _, _ = run_attention(nat, c._replace(B=1), {key: np.ascontiguousarray(d[key][i:i + 1]) for key in ("q", "k", "v", "do")})
        for name in hc.TENSORS:
            assert torch.equal(alone[name][0], together[name][i]), (i, name)


@gpu
@pytest.mark.parametrize("c", hc.CONTRACT_CASES, ids=CONTRACT_IDS)
def test_attention_sample_isolation(nat, c):
    """NaN in sample 1's k, then in sample 1's dout: exactly sample 1's outputs (of the pass that reads it) are NaN; samples 0 and
    2 are bit-identical to the clean run."""
    d, tab = hc.att_make(c), Table(hc.att_id(c) + " sample")
    clean, _, _ = run_attention(nat, c, d)
    for key, hit in (("k", hc.TENSORS), ("do", ("dq", "dk", "dv"))):
        bad = {name: d[name].copy() for name in ("q", "k", "v", "do")}
        bad[key][1] = np.nan
        res, _, _ = run_attention(nat, c, bad)
        for name in hc.TENSORS:
            if name in hit:
                tab.nan("NaN %s: %s[1]" % (key, name), res[name][1])
                tab.same("NaN %s: %s[0, 2]" % (key, name), res[name][0::2], clean[name][0::2])
            else:
                tab.same("NaN %s: %s" % (key, name), res[name], clean[name])
    tab.done()


@gpu
@pytest.mark.parametrize("c", hc.CONTRACT_CASES, ids=CONTRACT_IDS)
def test_attention_head_isolation(nat, c):
    """NaN in the columns of head 1 of k, then of v, then of dout: of out, dq, dk, dv exactly head 1's columns, and of prob its
    rows, change — those that read the operand at all (prob and dv do not read v; the forward does not read dout) — and the rest is
    bit-identical to the clean run."""
    d, tab, h = hc.att_make(c), Table(hc.att_id(c) + " head"), 1
    cols = slice(h * c.D, (h + 1) * c.D)
    other = [i for i in range(c.H * c.D) if not cols.start <= i < cols.stop]
    clean, _, _ = run_attention(nat, c, d)
    for key, hit in (("k", hc.TENSORS), ("v", ("out", "dq", "dk")), ("do", ("dq", "dk", "dv"))):
        bad = {name: d[name].copy() for name in ("q", "k", "v", "do")}
        bad[key][:, :, cols] = np.nan
        res, _, _ = run_attention(nat, c, bad)
        for name in hc.TENSORS:
            what = "NaN %s: %s" % (key, name)
            if name not in hit:
                tab.same(what, res[name], clean[name])
            elif name == "prob":
                tab.nan(what + " head 1", res[name][:, h])
                tab.same(what + " head 0", res[name][:, :h], clean[name][:, :h])
            else:
                tab.nan(what + " head 1", res[name][:, :, cols])
                tab.same(what + " head 0", res[name][:, :, other], clean[name][:, :, other])
    tab.done()


# ---- D. refusals ------------------------------------------------------------------------------------------------------------------------
def _sliced(B, L, width, off, E):
    return torch.ones(B, L, width, device=DEV)[:, :, off:off + E]


REFUSALS = {
    # name: (H, E, q, k / v, dk / dv as (width, first column), message forward, message backward)
    "head width 8": (2, 16, (16, 0), (16, 0), (16, 0), "head width 8", "head width 8"),
    "stride no multiple of 4": (2, 32, (32, 0), (34, 0), (32, 0), "multiples of 4 floats", "multiples of 4 floats"),
    "q stride no multiple of 4": (2, 32, (34, 0), (32, 0), (32, 0), "multiples of 4 floats", "multiples of 4 floats"),
    "stride below H * D": (2, 32, (32, 0), (16, 0), (32, 0), "row strides must cover all heads", "row strides must cover all heads"),
    "slice from column 1": (2, 32, (32, 0), (36, 1), (32, 0), "16-byte aligned", "16-byte aligned"),
    "dk stride no multiple of 4": (2, 32, (32, 0), (32, 0), (34, 0), None, "gradient row strides"),
    "dk slice from column 1": (2, 32, (32, 0), (32, 0), (36, 1), None, "16-byte aligned"),
}


@gpu
@pytest.mark.parametrize("name", list(REFUSALS))
def test_attention_refusals(nat, name):
    """Each of these the ABI refuses before any launch: the call raises with the ABI's message and the NaN-prefilled outputs are
    untouched."""
    from ogc_amd._lib import OgcOpsError
    H, E, (qw, qo), (kw, ko), (gw, go), msg_fwd, msg_bwd = REFUSALS[name]
    B, Lq, Lk = 2, 3, 5
    kE = min(E, kw)                                                # ("below H * D": k and v narrower than the heads need)
    q, k, v = _sliced(B, Lq, qw, qo, E), _sliced(B, Lk, kw, ko, kE), _sliced(B, Lk, kw, ko, kE)
    out, prob = torch.full((B, Lq, E), NAN, device=DEV), torch.full((B, H, Lq, Lk), NAN, device=DEV)
    if msg_fwd is not None:
        with pytest.raises(OgcOpsError, match=msg_fwd):
            nat.attention_fwd_wrapper(H, 0.25, q, k, v, out, prob)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()) and bool(torch.isnan(prob).all())
    dq = torch.full((B, Lq, E), NAN, device=DEV)
    dk, dv = (torch.full((B, Lk, gw), NAN, device=DEV) for _ in range(2))
    with pytest.raises(OgcOpsError, match=msg_bwd):
        nat.attention_bwd_wrapper(H, 0.25, q, k, v, torch.ones(B, Lq, E, device=DEV), torch.ones(B, H, Lq, Lk, device=DEV),
                                  torch.ones(B, Lq, E, device=DEV), dq, dk[:, :, go:go + kE], dv[:, :, go:go + kE])
    torch.cuda.synchronize()
    assert bool(torch.isnan(dq).all()) and bool(torch.isnan(dk).all()) and bool(torch.isnan(dv).all())


@gpu
def test_attention_backward_over_the_lds_limit(nat):
    """(lq, lk, D) = (16, 992, 16) needs 65600 bytes of LDS: the backward is refused before any launch; the forward of that shape
    runs and meets the truth."""
    from ogc_amd._lib import OgcOpsError
    c = hc.OVER_CASE
    d, tab = hc.att_make(c), Table(hc.att_id(c))
    res, ops, tails = run_attention(nat, c, d, pad=PAD, backward=False)
    check_truth(tab, c, d, res, ("out", "prob"))
    for name, tail in tails:
        survived(tab, name, tail)
    with pytest.raises(OgcOpsError, match="does not fit"):
        nat.attention_bwd_wrapper(c.H, hc.att_scale(c.D), ops.view["q"], ops.view["k"], ops.view["v"], res["out"], res["prob"],
                                  _dev(d["do"]), ops.grad["q"], ops.grad["k"], ops.grad["v"])
    torch.cuda.synchronize()
    for name in ("q", "k", "v"):
        tab.nan("d" + name + " after the refusal", ops.grad[name])
    ops.untouched(tab)
    tab.done()


# ---- E. the module routes ---------------------------------------------------------------------------------------------------------------
CORE = "_CrossAttentionCoreBackward"
ROUTES = {
    # name: (B, Lq, Lk or None for self-attention, node classes that must be there, node classes that must not)
    "self": (3, 10, None, {"_SelfAttentionCoreBackward", "_SmallLinearBackward"}, {CORE, "_CrossProjectionsBackward"}),
    "cross": (3, 10, 70, {CORE, "_CrossProjectionsBackward", "_SmallLinearBackward"}, {"_ManyRowsLinearBackward"}),
    "cross-4096-keys": (4, 8, 1024, {CORE, "_CrossProjectionsBackward", "_SmallLinearBackward"}, {"_ManyRowsLinearBackward"}),
    # more than 1024 query rows: F.linear for the queries and the output projection; the keys by their own row count.  Here 645
    # key rows go through ogc_small_linear_bwd: its db, once ONE running fp32 sum over the rows, missed in_proj_bias's gate (the
    # same sum replayed on the host: 3.3e-5 off at |db| = 48, against 4.7e-6 summed slice by slice, as the kernel does now)
    "cross-1032-queries": (129, 8, 5, {CORE, "_SmallLinearBackward"}, {"_CrossProjectionsBackward", "_ManyRowsLinearBackward"}),
    "cross-1032-queries-4128-keys": (129, 8, 32, {CORE, "_ManyRowsLinearBackward"}, {"_CrossProjectionsBackward", "_SmallLinearBackward"}),
}
GRADS = ("in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias")


def _module(E, H, seed):
    torch.manual_seed(seed)
    mha = torch.nn.MultiheadAttention(E, H, batch_first=True)
    with torch.no_grad():
        mha.in_proj_bias.normal_(0, 0.2)
        mha.out_proj.bias.normal_(0, 0.2)
    return mha


def _module_inputs(E, B, Lq, Lk, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, Lq, E, generator=g)
    k = None if Lk is None else torch.randn(B, Lk, E, generator=g)
    return q, k, torch.randn(B, Lq, E, generator=g)


def _module_run(mha, q, k, w, dtype, device, fused, grad=True):
    """-> ({"out", "query", "key", parameter gradients}, the output's autograd node names)."""
    from ogc_amd.fused import multihead_attention
    m = copy.deepcopy(mha).to(device=device, dtype=dtype)
    q = q.detach().clone().to(device=device, dtype=dtype).requires_grad_(grad)
    k = q if k is None else k.detach().clone().to(device=device, dtype=dtype).requires_grad_(grad)
    with torch.set_grad_enabled(grad):
        out = multihead_attention(m, q, k, k) if fused else m(q, k, k, need_weights=False)[0]
    res, nodes = {"out": out.detach().cpu()}, _node_names(out)
    if grad:
        (out * w.to(device=device, dtype=dtype)).sum().backward()
        res["query"] = q.grad.cpu()
        if k is not q:
            res["key"] = k.grad.cpu()
        params = dict(m.named_parameters())
        res.update({name: params[name].grad.cpu() for name in GRADS})
    return res, nodes


def _module_check(tab, mha, q, k, w, grad=True):
    truth, _ = _module_run(mha, q, k, w, torch.float64, "cpu", False, grad)
    yard, _ = _module_run(mha, q, k, w, torch.float32, "cpu", False, grad)
    got, nodes = _module_run(mha, q, k, w, torch.float32, DEV, True, grad)
    assert set(got) == set(truth)
    for name in truth:                                              # (in_proj_bias as one tensor: its key third is zero in exact arithmetic)
        tab.check(name, got[name], truth[name], yard[name])
    return nodes


@gpu
@pytest.mark.parametrize("E,H", [(32, 2), (64, 2)])
@pytest.mark.parametrize("route", list(ROUTES))
def test_module_routes_truth(nat, route, E, H):
    """multihead_attention(mha, q, k, k) against the same nn.MultiheadAttention in float64 on the host, the output and every
    gradient under Table's gate (yardstick: the module in fp32 on the host); the route by its autograd node classes."""
    B, Lq, Lk, there, absent = ROUTES[route]
    from ogc_amd.fused import attention_core_available
    assert attention_core_available(E, H, Lq, Lq if Lk is None else Lk)
    tab = Table("%s E%d H%d" % (route, E, H))
    nodes = _module_check(tab, _module(E, H, 7), *_module_inputs(E, B, Lq, Lk, E + B))
    assert there <= nodes and not (absent & nodes), sorted(nodes)
    tab.done()


@gpu
@pytest.mark.parametrize("E,H", [(32, 2), (64, 2)])
def test_module_forward_only(nat, E, H):
    """Under no_grad (cross-attention then projects through small_linear on both sides): the output against float64."""
    tab = Table("no_grad E%d H%d" % (E, H))
    for Lk in (70, None):
        nodes = _module_check(tab, _module(E, H, 8), *_module_inputs(E, 3, 10, Lk, E), grad=False)
        assert not nodes
    tab.done()


@gpu
def test_module_at_the_gate_limit(nat):
    """(lq, lk, D) = (16, 990, 16), the largest lk the Python gate admits at lq = 16, through multihead_attention and its backward;
    one key more is not admitted (the wrappers take it: LIMIT_CASE of test_attention_truth)."""
    from ogc_amd.fused import attention_core_available
    lq, lk, D = hc.GATE_LIMIT
    q, k, w = _module_inputs(D, 1, lq, lk, 3)
    assert attention_core_available(D, 1, lq, lk, q.to(DEV), k.to(DEV)) and hc.att_lds(lq, lk + 1, D) == hc.AT_LDS
    tab = Table("gate limit 16x990")
    nodes = _module_check(tab, _module(D, 1, 9), q, k, w)
    assert {CORE, "_CrossProjectionsBackward"} <= nodes
    tab.done()
    assert not attention_core_available(D, 1, lq, lk + 1, q.to(DEV), k.to(DEV))


@gpu
def test_module_fallback_equals_the_module(nat):
    """Heads of 8 columns are not offered: multihead_attention runs the module itself, and its result equals the module's."""
    from ogc_amd.fused import attention_core_available, multihead_attention
    mha = _module(32, 4, 5).to(DEV)
    q, k, _ = _module_inputs(32, 3, 10, 70, 6)
    q, k = q.to(DEV), k.to(DEV)
    assert not attention_core_available(32, 4, 10, 70, q, k)
    for key in (k, q):
        got, want = multihead_attention(mha, q, key, key), mha(q, key, key, need_weights=False)[0]
        assert torch.equal(got, want) and not ({CORE, "_SelfAttentionCoreBackward", "_SmallLinearBackward"} & _node_names(got))

"""The soft-correspondence kernels — ogc_soft_nn_target (csrc/soft_nn.hip: the lane-per-query form and the matrix-core form) and
ogc_soft_carry (csrc/soft_carry.hip) — against a float64 reference on DECIDED inputs (tests/soft_corr_cases.py): squared distances
and consistency products exact in fp32 in any order, a power-of-two temperature, no row near the 1e-10 clamp unless it is meant
to be, every candidate of weight to some row.  Rounding is then negligible and EVERY row of every output is held to float64
tightly enough that structure shows: a dropped last candidate of a wavefront's share, a mis-merged lane group, a wrong row in the
tail query tile, a mask slot read from the next row, padding that leaks into Z.  The scene-scale tests
(test_fused_loss_gpu.test_soft_nn_target, test_soft_carry_gpu.test_kernel_against_the_op_sequence) keep the other half: no worse
than torch's fp32 where the distance formula is ill-conditioned.

Tolerance, per output tensor AND row class (test_group_norm_truth_gpu.Table).  The yardstick is the op sequence of the original
in torch fp32 on the host, measured against the same float64 truth:
    err_kernel <= max(4 * err_torch32, 8 * 2**-24 * max|truth|)
for the max-abs error, and for the 2-norm of the error with the floor taken per element.  The soft-NN clamp rows (every eleventh
query from the fifth: m1 = 2^-40 onehot, output (V / Z) * 1e10 ~ 1e-2, in which Z does not cancel) and the other rows
(|output| ~ 8) are gated SEPARATELY: their magnitudes differ by 1e3 and one class must not hide the other.  The ones column of
soft-carry must also satisfy |out - 1| <= 8 * 2**-24.  Both errors are printed per case and class; nothing measured from the
kernels is written into this file.
Error model of the matrix-core forms, should a row miss: d2 is exact, v_sqrt_f32 and v_exp_f32 are 1 ulp each, and log2(e) / tau
is folded into one fp32 scale, so a weight carries a relative error of about (2 + |y|) * 2**-24 with |y| = log2(e) d / tau <= 16
on these clouds — but the weights fall off as 2**-|y|, so the weighted mean of |y| is of order 1: a few 2**-24 relative per
weight, the same order as the yardstick's library exp.  The sums add one rounding per step: a lane walks at most 6 tiles, the
butterfly adds 4 steps and the wavefront merge 8 (soft-NN); 5 tiles of 4 MFMAs and 4 wavefronts (soft-carry).

The shapes (soft_corr_cases.NN_* / CARRY_*) are the smallest that reach each branch; each line there names its branch, and
test_case_list_reaches_its_branches re-derives them from the launch arithmetic.  The lane-per-query form beyond one staged tile
per wavefront (n2 >= 256) is reachable only with OGC_SOFT_NN_MFMA=0, read once per process: the matrix-core sizes go through it
in ONE child process, against the same truth and gate.

Memory contract of ogc_soft_nn_target, both forms (test_soft_carry_gpu has soft-carry's): guard bands, batch independence, and
reuse of the stream's workspace after a larger call — all bit for bit.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import soft_corr_cases as sc
from test_group_norm_truth_gpu import Table as _Table, _dev

gpu = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRA_CASES = sc.CONTRACT_CASES


@pytest.fixture(scope="module")
def nat():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    import ogc_amd  # noqa: F401  (fails loudly if libogc_ops.so is missing)
    from ogc_amd import pointnet2_cuda
    return pointnet2_cuda


# ---- the generator's guarantees (CPU) --------------------------------------------------------------------------------------------
def _conditions(c, d):
    """What soft_corr_cases.make measured, by another route: torch float64, weights normalised by softmax (Z = 1)."""
    t = lambda a: torch.from_numpy(a).double()  # noqa: E731
    p1, p2 = t(d["p1"]), t(d["p2"])
    truth, yard = sc.reference(c, d, torch.float64), sc.reference(c, d, torch.float32)
    clamp = torch.zeros(c.n1, dtype=torch.bool)
    if c.op == "nn":
        clamp[5::11] = True
    gate_row, gates = torch.zeros(c.n1, dtype=torch.float64), {}
    for name, rows in (("rows", ~clamp), ("clamp", clamp)):
        if bool(rows.any()):
            err = float((yard[:, rows].double() - truth[:, rows]).abs().max())
            gates[name] = max(4 * err, 8 * sc.U * float(truth[:, rows].abs().max()))
            gate_row[rows] = gates[name]
    m = {"gates": gates}
    e = (-torch.cdist(p1, p2) / sc.TAU).softmax(-1)                                     # (B, n1, n2), rows sum to 1
    pads = sc.padding_slots(c) * torch.exp(-p1.norm(dim=-1) / sc.TAU) / \
        torch.exp(-torch.cdist(p1, p2) / sc.TAU).sum(-1)                                # the padding's weight in the same units
    if c.op == "nn":
        W = e * torch.einsum("bmk,bnk->bmn", t(d["m1"]), t(d["m2"]))
        A, V = W.sum(-1), W @ p2
        out = V / A.clamp(1e-10).unsqueeze(-1)
        rest = 1 - e                                                                     # Z with candidate j left out
        left = ((V.unsqueeze(2) - W.unsqueeze(-1) * p2.unsqueeze(1)) / rest.unsqueeze(-1)) / \
            ((A.unsqueeze(-1) - W) / rest).clamp(1e-10).unsqueeze(-1)
        m["az_rows"] = float(A[:, ~clamp].min())
        if bool(clamp.any()):
            m["az_clamp"] = float(A[:, clamp].max())
            doubled = (V / 2) / (A / 2).clamp(1e-10).unsqueeze(-1)
            m["z2"] = float(((doubled - out).abs().amax(-1) / gate_row)[:, clamp].min())
        padded = (V / (1 + pads).unsqueeze(-1)) / (A / (1 + pads)).clamp(1e-10).unsqueeze(-1)
        share = W / A.unsqueeze(-1)
    else:
        x = t(d["x"])
        out = e @ x
        rest = 1 - e
        left = (out.unsqueeze(2) - e.unsqueeze(-1) * x.unsqueeze(1)) / rest.unsqueeze(-1)
        padded = out / (1 + pads).unsqueeze(-1)
        share = e
    assert float((out - truth).abs().max()) <= 1e-12 * float(truth.abs().max())
    move = (left - out.unsqueeze(2)).abs().amax(-1)
    move[~(rest > 0)] = float("inf")
    if c.n1 >= c.n2 and not (c.op == "carry" and c.k == 1):
        m["cover"] = float((move / gate_row[None, :, None]).amax(1).min())
    if c.n1 < c.n2:
        m["share"] = float(share.topk(2, dim=-1)[0][..., 1].min())
    if c.off == 0 and sc.padding_slots(c):
        ratio = (padded - out).abs().amax(-1) / gate_row
        m["pad"] = float((ratio[:, clamp] if c.op == "nn" else ratio).max())
    return m


@pytest.mark.parametrize("c", sc.ALL_CASES + EXTRA_CASES, ids=[sc.case_id(c) for c in sc.ALL_CASES + EXTRA_CASES])
def test_case_is_decided(c):
    """Re-checks what soft_corr_cases.make asserts: the lattices, d2 exact in fp32, coverage of every candidate (or two strong
    candidates per row below n2 queries), the clamp margins of every row, and that padding at the origin would show."""
    d = sc.make(c)
    h = sc.half_width(c.n2)
    q1, q2 = (torch.from_numpy(d["p1"]).double() - c.off) * 16, (torch.from_numpy(d["p2"]).double() - c.off) * 16
    assert bool((q1 == q1.round()).all() and (q2 == q2.round()).all()) and float(q2.abs().max()) <= h
    assert float((q1 - q2[:, torch.arange(c.n1) % c.n2]).abs().max()) <= 1                 # one lattice step or none per axis
    a, b = torch.from_numpy(d["p1"]), torch.from_numpy(d["p2"])
    assert a.dtype == torch.float32 and b.dtype == torch.float32
    d2 = torch.baddbmm((a * a).sum(-1, keepdim=True) + (b * b).sum(-1).unsqueeze(1), a * -2, b.transpose(1, 2))   # fp32, mm first
    assert torch.equal(d2.double(), ((a.double().unsqueeze(2) - b.double().unsqueeze(1)) ** 2).sum(-1))
    if c.op == "nn":
        m1, m2 = torch.from_numpy(d["m1"]), torch.from_numpy(d["m2"])
        clamp = torch.zeros(c.n1, dtype=torch.bool)
        clamp[5::11] = True
        assert bool(((m2 * 4) == (m2 * 4).round()).all()) and torch.equal(m2.sum(-1), torch.ones(c.B, c.n2))
        assert bool(((m1[:, ~clamp] * 4) == (m1[:, ~clamp] * 4).round()).all())
        assert torch.equal(m1[:, ~clamp].sum(-1), torch.ones(c.B, int((~clamp).sum())))
        assert torch.equal(m1[:, clamp].sum(-1), torch.full((c.B, int(clamp.sum())), sc.CLAMP_SCALE))
        assert torch.equal((m1[:, clamp] > 0).sum(-1), torch.ones(c.B, int(clamp.sum()), dtype=torch.long))
        cons32, cons64 = torch.einsum("bmk,bnk->bmn", m1, m2), torch.einsum("bmk,bnk->bmn", m1.double(), m2.double())
        assert torch.equal(cons32.double(), cons64)                                          # the consistency is exact in fp32
        if c.n2 >= 16 * c.k:
            assert bool((m2[..., 0] > 0).any() and (m2[..., -1] > 0).any())                  # both end slots are populated
    else:
        x = torch.from_numpy(d["x"]).double() * 64
        assert bool((x == x.round()).all() and (x >= 0).all() and (x[..., -1] == 64).all())
        assert c.k == 1 or bool((x[..., :-1].sum(-1) == 64).all())
    if c.B > 1:
        assert not np.array_equal(d["p2"][0], d["p2"][1])                                    # samples are drawn independently
    m = _conditions(c, d)
    print("%-28s %s" % (sc.case_id(c), "  ".join("%s %.3g" % (k, v) for k, v in m.items() if k != "gates")),
          "  gates", "  ".join("%s %.2e" % kv for kv in m["gates"].items()))
    if c.op == "nn":
        assert m["az_rows"] >= 1e-3
        assert c.n1 <= 5 or (m["az_clamp"] <= 1e-11 and m["z2"] >= sc.COVER)
    if c.n1 >= c.n2 and not (c.op == "carry" and c.k == 1):
        assert m["cover"] >= sc.COVER, m["cover"]
    if c.n1 < c.n2:
        assert m["share"] >= sc.MIN_SHARE, m["share"]
    if c.off == 0:
        assert m["pad"] >= sc.COVER, m["pad"]
    for key, val in m.items():                                                               # and make() measured the same
        if key == "gates":
            assert {k: v[1] for k, v in d["gates"].items()} == val
        else:
            assert d[key] == val or abs(d[key] - val) <= 1e-6 * abs(val), (key, d[key], val)


# the launch arithmetic of csrc/soft_nn.hip and csrc/soft_carry.hip, written out
def nn_form(n2):
    return "mfma" if n2 >= 256 else "lane"


def nn_lane_launch(n1, n2, k):
    kmax = 8 if k <= 8 else 16 if k <= 16 else 32
    tile = 32 if kmax > 16 else 64
    per = -(-n2 // 8)
    shares = [max(0, min(n2, (w + 1) * per) - w * per) for w in range(8)]
    return dict(kmax=kmax, tile=tile, per=per, shares=shares, empty=shares.count(0), staged=max(-(-s // tile) for s in shares),
                ragged=any(s % 8 for s in shares), pad=sum(-(-s // 8) * 8 - s for s in shares), qblocks=-(-n1 // 64))


def nn_mfma_launch(n1, n2, k):
    nm = 2 if k <= 8 else 3 if k <= 12 else 4 if k <= 16 else 8
    tiles = -(-n2 // 16)
    tiles_pad = -(-tiles // 16) * 16
    per = tiles_pad // 8
    return dict(nm=nm, tiles=tiles, tiles_pad=tiles_pad, per=per, pad=tiles_pad * 16 - n2,
                all_pad=sum(1 for w in range(8) if w * per * 16 >= n2), qblocks=-(-n1 // 32))


def carry_launch(n1, n2, c):
    """One entry per call of the kernel (the wrapper splits x in blocks of 64 columns)."""
    tiles = -(-n2 // 16)
    tiles_pad = -(-tiles // 4) * 4
    calls = []
    for c0 in range(0, c, 64):
        cols = min(64, c - c0)
        qt = 4 if cols <= 32 else 2
        calls.append(dict(cols=cols, nt=-(-cols // 16), qt=qt, qblocks=-(-n1 // (qt * 16)), tiles_pad=tiles_pad, per=tiles_pad // 4,
                          pad=tiles_pad * 16 - n2, all_pad=sum(1 for w in range(4) if w * (tiles_pad // 4) * 16 >= n2)))
    return calls


def test_case_list_reaches_its_branches():
    """The launch arithmetic of both kernels, replayed on the case lists: every branch the issue of this suite names is there."""
    lane = {c: nn_lane_launch(c.n1, c.n2, c.k) for c in sc.NN_CASES if nn_form(c.n2) == "lane"}
    mfma = {c: nn_mfma_launch(c.n1, c.n2, c.k) for c in sc.NN_CASES if nn_form(c.n2) == "mfma"}
    assert nn_form(255) == "lane" and nn_form(256) == "mfma" and {255, 256, 257} <= {c.n2 for c in sc.NN_CASES}
    assert all(c in lane for c in sc.NN_LANE_CASES) and all(c in mfma for c in sc.NN_MFMA_CASES)
    # lane-per-query form
    by_n2 = {c.n2: g for c, g in lane.items()}
    assert [by_n2[n]["empty"] for n in (1, 7, 8, 9)] == [7, 1, 0, 3] and by_n2[9]["shares"][4] == 1
    assert by_n2[100]["shares"] == [13] * 7 + [9] and by_n2[100]["ragged"] and by_n2[100]["pad"] == 28
    assert by_n2[255]["shares"] == [32] * 7 + [31]
    kmax = {}
    for c, g in lane.items():
        kmax.setdefault(c.k, set()).add((g["kmax"], g["tile"]))
    assert [kmax[k] for k in (1, 8, 9, 16, 17, 32)] == [{(8, 64)}, {(8, 64)}, {(16, 64)}, {(16, 64)}, {(32, 32)}, {(32, 32)}]
    assert any(g["kmax"] == 32 and g["shares"][0] == g["tile"] for g in lane.values())       # a share that fills SN_TILE exactly
    assert all(g["staged"] == 1 for g in lane.values())                                      # one staged tile below n2 = 256 ...
    large = [nn_lane_launch(c.n1, c.n2, c.k) for c in sc.NN_LANE_LARGE]                      # ... more only through the switch
    assert {(g["tile"], g["staged"]) for g in large} >= {(64, 1), (64, 2), (32, 2)}
    assert all(nn_form(c.n2) == "mfma" for c in sc.NN_LANE_LARGE) and set(sc.NN_LANE_LARGE) <= set(sc.NN_CASES)
    # matrix-core form
    by_n2 = {c.n2: g for c, g in mfma.items()}
    assert by_n2[256]["pad"] == 0 and by_n2[512]["pad"] == 0 and by_n2[511]["pad"] == 1
    assert (by_n2[257]["pad"], by_n2[257]["all_pad"], by_n2[257]["tiles"], by_n2[257]["per"]) == (255, 3, 17, 4)
    assert [by_n2[n]["per"] for n in (256, 511, 512, 513)] == [2, 4, 4, 6]
    nm = {}
    for c, g in mfma.items():
        nm.setdefault(c.k, set()).add(g["nm"])
    assert [nm[k] for k in (1, 8, 9, 10, 12, 13, 16, 17, 32)] == [{2}, {2}, {3}, {3}, {3}, {4}, {4}, {8}, {8}]
    # n1 around the query blocks of both forms, B = 1 and 3 in both
    for n2, form in ((64, lane), (256, mfma)):
        assert {c.n1 for c in sc.NN_EDGE_CASES if c.n2 == n2} == set(sc.N1_EDGES) and all(c in form for c in sc.NN_EDGE_CASES if c.n2 == n2)
    assert {c.B for c in lane} == {1, 3} and {c.B for c in mfma} == {1, 3}
    assert any(g["qblocks"] > 1 and c.n1 % 64 for c, g in lane.items()) and any(g["qblocks"] > 1 and c.n1 % 32 for c, g in mfma.items())
    # soft-carry
    calls = {c: carry_launch(c.n1, c.n2, c.k) for c in sc.CARRY_ALL}
    assert {1, 16, 17, 32, 33, 48, 49, 64, 65, 100} <= {c.k for c in sc.CARRY_CASES}
    assert {c.k: (g[0]["nt"], g[0]["qt"]) for c, g in calls.items() if c.k in (1, 16, 17, 32, 33, 48, 49, 64)} == \
        {1: (1, 4), 16: (1, 4), 17: (2, 4), 32: (2, 4), 33: (3, 2), 48: (3, 2), 49: (4, 2), 64: (4, 2)}
    assert [[g["cols"] for g in calls[c]] for c in sc.CARRY_CASES if c.k > 64] == [[64, 1], [64, 36]]
    assert {1, 15, 16, 17, 63, 64, 65, 257} <= {c.n2 for c in sc.CARRY_CASES}
    assert {c.n2: g[0]["tiles_pad"] for c, g in calls.items() if c in sc.CARRY_CASES and c.n2 in (1, 16, 17, 64, 65, 257)} == \
        {1: 4, 16: 4, 17: 4, 64: 4, 65: 8, 257: 20}
    for qt in (4, 2):
        assert {c.n1 for c in sc.CARRY_EDGE_CASES if calls[c][0]["qt"] == qt} == set(sc.N1_EDGES)
    assert {c.B for c in sc.CARRY_ALL} == {1, 3}
    # padding at the origin, once per op, where there is padding to count
    assert [(c.op, sc.padding_slots(c)) for c in sc.ALL_CASES if c.off == 0] == [("nn", 28), ("nn", 255), ("carry", 63)]
    assert sc.nn_lane_padding(100) == nn_lane_launch(1, 100, 1)["pad"] and sc.nn_mfma_padding(257) == nn_mfma_launch(1, 257, 1)["pad"]
    assert sc.carry_padding(65) == carry_launch(1, 65, 1)[0]["pad"]
    # the contract cases: one per form; the reuse pair shrinks the packed table
    assert [nn_form(c.n2) for c in sc.CONTRACT_CASES] == ["lane", "mfma"] and [c.n2 for c in sc.CONTRACT_CASES] == [149, 300]
    assert (sc.REUSE_BIG.n2, sc.REUSE_SMALL.n2) == (513, 257) and sc.REUSE_BIG.k == sc.REUSE_SMALL.k
    assert sc.REUSE_BIG in sc.NN_CASES and sc.REUSE_SMALL in sc.NN_CASES and sc.REUSE_SMALL.off == 0
    # what the suite can afford
    assert 50 <= len(sc.ALL_CASES) <= 70 and all(c.n1 * c.n2 <= 513 * 513 and c.k <= (32 if c.op == "nn" else 100) for c in sc.ALL_CASES)


# ---- GPU helpers ------------------------------------------------------------------------------------------------------------------
class Table(_Table):
    def __init__(self, c, mode=""):
        self.name, self.bad = sc.case_id(c) + mode, []


def run_nn(nat, c, d):
    """ogc_soft_nn_target on fresh device copies, the output pre-filled with NaN."""
    out = torch.full((c.B, c.n1, 3), float("nan"), device=DEV)
    nat.soft_nn_target_wrapper(c.B, c.n1, c.n2, c.k, sc.TAU, _dev(d["p1"]), _dev(d["p2"]), _dev(d["m1"]), _dev(d["m2"]), out)
    return out


def run_carry(nat, c, d):
    out = torch.full((c.B, c.n1, c.k), float("nan"), device=DEV)
    nat.soft_carry_wrapper(c.B, c.n1, c.n2, c.k, sc.TAU, _dev(d["p1"]), _dev(d["p2"]), _dev(d["x"]), out)
    return out


def check_classes(tab, c, d, out):
    """Every row of `out` against the truth, each row class against its own gate."""
    out = out.cpu()
    assert out.shape == d["truth"].shape
    for name, (rows, _, _) in d["gates"].items():
        tab.check(name, out[:, rows], d["truth"][:, rows], d["yard"][:, rows])


# ---- soft nearest neighbour ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("c", sc.NN_CASES, ids=[sc.case_id(c) for c in sc.NN_CASES])
def test_soft_nn_truth(nat, c):
    """ogc_soft_nn_target, the form its size selects, against the float64 truth: every row, clamp rows and the others apart."""
    d = sc.make(c)
    tab = Table(c, " " + nn_form(c.n2))
    check_classes(tab, c, d, run_nn(nat, c, d))
    tab.done()


CHILD = """
import sys, torch, ogc_amd
from ogc_amd import pointnet2_cuda as nat
import soft_corr_cases as sc
outs = {}
for c in sc.NN_LANE_LARGE:
    d = sc.inputs(c)
    t = [torch.from_numpy(d[key]).cuda() for key in ("p1", "p2", "m1", "m2")]
    out = torch.full((c.B, c.n1, 3), float("nan"), device="cuda")
    nat.soft_nn_target_wrapper(c.B, c.n1, c.n2, c.k, sc.TAU, *t, out)
    outs[sc.case_id(c)] = out.cpu()
torch.save(outs, sys.argv[1])
"""


@gpu
def test_soft_nn_lane_form_at_matrix_core_sizes(nat, tmp_path):
    """The lane-per-query kernel where a wavefront stages more than one tile of candidates (n2 >= 256): the matrix-core cases
    through OGC_SOFT_NN_MFMA=0 in one fresh child process, against the same truth and gate."""
    path = str(tmp_path / "lane.pt")
    env = dict(os.environ, OGC_SOFT_NN_MFMA="0", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    r = subprocess.run([sys.executable, "-c", CHILD, path], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-1500:]
    outs = torch.load(path)
    bad, differs = [], 0
    for c in sc.NN_LANE_LARGE:
        d = sc.make(c)
        tab = Table(c, " lane")
        check_classes(tab, c, d, outs[sc.case_id(c)])
        bad += [(tab.name, b) for b in tab.bad]
        differs += int(not torch.equal(outs[sc.case_id(c)], run_nn(nat, c, d).cpu()))
    assert not bad, bad
    assert differs, "the child's results equal this process's bit for bit: the switch did not select the other kernel"


# ---- soft carry ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("c", sc.CARRY_ALL, ids=[sc.case_id(c) for c in sc.CARRY_ALL])
def test_soft_carry_truth(nat, c):
    """ogc_soft_carry (through the wrapper's column split beyond 64 columns) against the float64 truth, every row; the ones
    column within 8 * 2**-24 of 1."""
    d = sc.make(c)
    tab = Table(c)
    out = run_carry(nat, c, d)
    check_classes(tab, c, d, out)
    ones = float((out[..., -1].double() - 1).abs().max())
    print("%-34s ones column off by %.3e (bound %.3e)" % (tab.name, ones, 8 * sc.U))
    if not ones <= 8 * sc.U:
        tab.bad.append("ones column")
    tab.done()


# ---- the memory contract of ogc_soft_nn_target ----------------------------------------------------------------------------------------
CONTRACT_IDS = [sc.case_id(c) for c in sc.CONTRACT_CASES]


@gpu
@pytest.mark.parametrize("c", sc.CONTRACT_CASES, ids=CONTRACT_IDS)
def test_soft_nn_guard_bands(nat, c):
    """The last sample's buffers end inside larger allocations: behind p2 lie points that coincide with queries, behind the masks
    1e6, behind target a sentinel; target itself starts as NaN.  A read or write past the end changes the result or the
    sentinel."""
    d = sc.make(c)
    B, n1, n2, k, PAD = c.B, c.n1, c.n2, c.k, 97
    want = run_nn(nat, c, d)
    p1, p2 = torch.from_numpy(d["p1"]).to(DEV), torch.from_numpy(d["p2"]).to(DEV)
    big_p1 = torch.full((B * n1 + PAD, 3), 7.0, device=DEV)
    big_p2 = torch.empty(B * n2 + PAD, 3, device=DEV)
    big_m1 = torch.full((B * n1 + PAD, k), 1e6, device=DEV)
    big_m2 = torch.full((B * n2 + PAD, k), 1e6, device=DEV)
    big_out = torch.full((B * n1 + PAD, 3), -12345.0, device=DEV)
    big_p1[:B * n1] = p1.reshape(-1, 3)
    big_p2[:B * n2] = p2.reshape(-1, 3)
    big_p2[B * n2:] = p1[-1, -PAD:]                      # candidates that would win if they were read
    big_m1[:B * n1] = torch.from_numpy(d["m1"]).to(DEV).reshape(-1, k)
    big_m2[:B * n2] = torch.from_numpy(d["m2"]).to(DEV).reshape(-1, k)
    big_out[:B * n1] = float("nan")
    nat.soft_nn_target_wrapper(B, n1, n2, k, sc.TAU, big_p1[:B * n1].view(B, n1, 3), big_p2[:B * n2].view(B, n2, 3),
                               big_m1[:B * n1].view(B, n1, k), big_m2[:B * n2].view(B, n2, k), big_out[:B * n1].view(B, n1, 3))
    torch.cuda.synchronize()
    tab = Table(c, " guard")
    check_classes(tab, c, d, want)
    tab.same("target", big_out[:B * n1].view(B, n1, 3), want)
    tab.same("sentinel", big_out[B * n1:], torch.full((PAD, 3), -12345.0, device=DEV))
    tab.done()


@gpu
@pytest.mark.parametrize("c", sc.CONTRACT_CASES, ids=CONTRACT_IDS)
def test_soft_nn_batch_independence(nat, c):
    """Each sample alone equals its slice of the batched call, bit for bit."""
    d = sc.make(c)
    together = run_nn(nat, c, d)
    one = c._replace(B=1)
    for i in range(c.B):
        alone = run_nn(nat, one, {key: np.ascontiguousarray(d[key][i:i + 1]) for key in ("p1", "p2", "m1", "m2")})
        assert torch.equal(alone[0], together[i]), i


@gpu
def test_soft_nn_workspace_reuse(nat):
    """A call at n2 = 513 and then one at n2 = 257 on the same stream: the smaller call's result is what it was before the larger
    one, bit for bit, and meets the truth.  The larger call leaves in the packed table candidates that sit on the smaller call's
    queries with masks of 1e3 — where the smaller call's 255 padding slots and its coordinate array will lie — and the smaller
    cloud is centred on the origin, so stale weight would show in Z (the clamp rows) and anywhere else."""
    small, big = sc.REUSE_SMALL, sc.REUSE_BIG
    d, dbig = sc.make(small), sc.make(big)
    first = run_nn(nat, small, d)
    reps = -(-big.n2 // small.n1)
    poison = dict(p1=dbig["p1"], p2=np.tile(d["p1"], (1, reps, 1))[:, :big.n2].copy(), m1=dbig["m1"],
                  m2=np.full((1, big.n2, big.k), 1e3, np.float32))
    loud = run_nn(nat, big, poison)
    assert bool(torch.isfinite(loud).all())
    again = run_nn(nat, small, d)
    tab = Table(small, " after n2=513")
    check_classes(tab, small, d, again)
    tab.same("target", again, first)
    tab.done()

"""The dynamic and invariance terms of the unsupervised loss (csrc/seg_loss.hip: ogc_rigid_moments / _translation / _blend,
ogc_mask_iou, ogc_matched_distance; ogc_kabsch_rotation and ogc_lsap_maximize between them) against a float64 reference on
DECIDED inputs (tests/seg_loss_cases.py), called through the native wrappers directly.  The twin of
test_batch_norm_truth_gpu.py and test_soft_corr_truth_gpu.py.

Tolerance.  Float tensors go through test_group_norm_truth_gpu.Table: the yardstick is the reference's op sequence in torch
float32 ON THE HOST, measured against the same sequence in float64,
    err_kernel <= max(4 * err_torch32, 8 * 2**-24 * max|truth|)
for the max-abs error and for the 2-norm.  Everything else is exact equality, and no allowance of an ulp is made anywhere:
  * mom: the 16 moments are exact in float64 in any order (integers below 2^53 in units of 2^-14), in the default mode (fp64
    atomics) and in the deterministic mode (one slab per chunk);
  * S, means: rigid_finalize_kernel's float64 operations replayed in numpy in its order (IEEE division, no contraction);
  * the special slots: weight 0 -> invalid, R = I, t = 0; one live point -> S = 0, valid, R = I, t = fp32(q) - fp32(p);
  * zero rows (all-zero mask row, pc2 at the origin; N = 1): residual 0, both gradient rows 0;
  * counts, iou (numpy float32 in the kernel's order, one IEEE division), the assignments (scipy);
  * ogc_matched_distance with p = 1, forward and backward: every difference and partial sum is exact in fp32;
  * equal rows: d12 = 0 and a zero p = 2 gradient row.
The blend is run twice: on the kernels' own R, t (the chain fused.rigid_residual composes, and that function itself, same bits)
and on the fp32-rounded float64 R, t, which isolates it; p = 0 with pc2 = pc is the blended flow of oa_icp.py.

The shapes are the smallest that reach each launch-geometry branch; each line of the case lists names its branch and
test_case_list_reaches_its_branches replays the launch arithmetic.  Outputs are pre-filled with NaN (-7 for integers), so a row
that is not written shows.
"""
import numpy as np
import pytest
import torch

import seg_loss_cases as sc
from test_group_norm_truth_gpu import Table as _Table, _dev

gpu = pytest.mark.gpu
DEV = "cuda"
DYN_IDS = [sc.case_id(c) for c in sc.DYN_CASES]
INV_IDS = [sc.case_id(c) for c in sc.INV_CASES]


@pytest.fixture(scope="module")
def nat():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    import ogc_amd  # noqa: F401  (fails loudly if libogc_ops.so is missing)
    from ogc_amd import pointnet2_cuda
    return pointnet2_cuda


class Table(_Table):
    def __init__(self, name):
        self.name, self.bad = name, []

    def same_nan(self, what, got, want):
        """Equal, with NaN where — and only where — `want` has it."""
        self.same(what + " NaNs", torch.isnan(got), torch.isnan(want))
        self.same(what, torch.nan_to_num(got, nan=-77.0), torch.nan_to_num(want, nan=-77.0))

    def zero(self, what, got):
        self.same(what, got, torch.zeros_like(got))


# ---- the generator's guarantees (CPU) --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", sc.DYN_CASES, ids=DYN_IDS)
def test_dynamic_case_is_decided(c):
    """Re-derives, from integer moments and the closed form S = M - (sum wp)(sum wq)^T / W in torch float64, what
    seg_loss_cases.make_dyn asserts through the reference's op sequence: the lattices, the exact moments, the special slots, the
    conditioning of every fitted slot, the residual of every row outside the zero rows, the coverage of every slot."""
    d = sc.make_dyn(c)
    VB, N, K = c.VB, c.N, c.K
    pc, pc2, mask = (torch.from_numpy(d[n]).double() for n in ("pc", "pc2", "mask"))
    ip, iq, iw = (pc * 16).long(), (pc2 * 16).long(), (mask * 4).long()
    assert torch.equal(ip.double() / 16, pc) and torch.equal(iq.double() / 16, pc2) and torch.equal(iw.double() / 4, mask)
    assert int(ip.abs().max()) <= 48 and int(iq.abs().max()) < 1024 and set(iw.unique().tolist()) <= {0, 1, 3, 4}
    g16 = torch.from_numpy(d["grad"]).double() * 16
    assert torch.equal(g16, g16.round()) and 1 <= float(g16.abs().min()) and float(g16.abs().max()) <= 32 and \
        (N == 1 or len(g16.unique()) > 2)
    # the moments in integers: units 2^-2, 2^-6, 2^-10
    W = iw.sum(dim=1)
    wp, wq = torch.einsum("bnk,bni->bki", iw, ip), torch.einsum("bnk,bni->bki", iw, iq)
    wpq = torch.einsum("bnk,bni,bnj->bkij", iw, ip, iq)
    assert int(wpq.abs().max()) < 2 ** 53
    mom = torch.cat([W.unsqueeze(2).double() / 4, wp.double() / 64, wq.double() / 64, wpq.reshape(VB, K, 9).double() / 1024], dim=2)
    assert torch.equal(mom, torch.from_numpy(d["mom"]))
    live = (iw > 0).sum(dim=1)
    assert torch.equal(live, torch.from_numpy(d["live"])) and int(iw[iw > 0].min()) >= 1     # leaving a point out moves W by >= 1/4
    zero_rows = (iw == 0).all(dim=2)
    assert torch.equal(zero_rows | (N == 1), torch.from_numpy(d["zero_rows"]))
    assert int(zero_rows.sum()) == (2 * VB if N >= 63 else 0) and not bool(iq[zero_rows].any())
    # the special slots are there
    roles = sc.slot_roles(c)
    if c.special:
        assert not bool(live[:, roles["zero"]].any()) and bool((live[:, roles["single"]] == 1).all())
    if N > 1:
        assert bool((live[:, roles["plain"]] >= 4).all())
    # the fit, closed form
    Wd = mom[..., :1]
    pm, qm = mom[..., 1:4] / Wd, mom[..., 4:7] / Wd
    S = mom[..., 7:].reshape(VB, K, 3, 3) - mom[..., 1:4].unsqueeze(3) * qm.unsqueeze(2)
    fitted = (live >= 2).reshape(-1)
    assert torch.equal(fitted, d["fitted"])
    R = torch.eye(3, dtype=torch.float64).repeat(VB * K, 1, 1)
    t = torch.zeros(VB * K, 3, dtype=torch.float64)
    ratio = float("inf")
    if fitted.any():
        Sf = S.reshape(-1, 3, 3)[fitted]
        u, s, vh = torch.linalg.svd(Sf)
        sign = torch.sign(torch.det(Sf))
        ratio = float(((s[:, 1] + sign * s[:, 2]) / s[:, 0]).min())
        flip = torch.ones_like(s)
        flip[:, 2] = torch.where(torch.det(vh.transpose(1, 2) @ u.transpose(1, 2)) < 0, -1.0, 1.0)
        R[fitted] = vh.transpose(1, 2) @ (flip.unsqueeze(2) * u.transpose(1, 2))
    one = (live == 1).reshape(-1) | fitted
    t[one] = qm.reshape(-1, 3)[one] - (R[one] @ pm.reshape(-1, 3)[one].unsqueeze(2)).squeeze(2)
    if c.special == "all":
        det = torch.det(S)
        assert bool((det[:, roles["mirror"]] < 0).all()) and bool((det[:, roles["plain"]] > 0).all())
        on_plane = iw[:, :, roles["planar"]] > 0
        assert bool((ip[..., 2][on_plane] == 3).all()) and int(on_plane.sum(dim=1).min()) >= 8
        assert float(torch.linalg.svdvals(S[:, roles["planar"]])[:, 2].max()) <= 1e-12
        Rm = R.reshape(VB, K, 3, 3)[:, roles["mirror"]]
        assert float((torch.det(Rm) - 1).abs().max()) <= 1e-12
    truth = d["truth"]
    assert float((R - truth["R"]).abs().max()) <= 1e-9 and float((t - truth["t"]).abs().max()) <= 1e-9
    # residuals, slot by slot
    blend = torch.zeros(VB, N, 3, dtype=torch.float64)
    moved = []
    for k in range(K):
        Rk, tk = R.reshape(VB, K, 3, 3)[:, k], t.reshape(VB, K, 3)[:, k]
        moved.append(pc @ Rk.transpose(1, 2) + tk.unsqueeze(1))
        blend += mask[:, :, k:k + 1] * moved[k]
    diff = blend - pc2
    rows = ~torch.from_numpy(d["zero_rows"])
    residual = float(diff[rows].abs().min()) if rows.any() else float("inf")
    assert float((diff - truth["diff"]).abs().max()) <= 1e-9
    gates, cover = {}, float("inf")
    for name in ("R", "t", "out1", "out2", "g1", "g2", "flow"):
        gates[name] = sc.gate(truth[name], d["yard"][name])
    for p in (1, 2):
        out = diff.norm(p=p, dim=-1)
        for k in range(K):
            moves = (diff - mask[:, :, k:k + 1] * (moved[k] - pc)).norm(p=p, dim=-1) - out
            for b in range(VB):
                if live[b, k] and rows.any():
                    cover = min(cover, float(moves[b].abs().max()) / gates["out%d" % p][0])
    print("%-22s ratio %.3f  min |residual| %.3e  cover %.0f gates  torch32 error: %s"
          % (sc.case_id(c), ratio, residual, cover, "  ".join("%s %.1e" % (n, gates[n][1]) for n in gates)))
    assert ratio >= sc.MIN_RATIO and residual >= sc.MIN_RESIDUAL and cover >= sc.COVER
    for mine, theirs in ((ratio, d["ratio"]), (residual, d["residual"]), (cover, d["cover"])):
        assert mine == theirs or abs(mine - theirs) <= 1e-6 * abs(theirs)
    # zero rows are zero in the reference too, gradients included
    for name in ("out1", "out2", "g1", "g2"):
        assert not bool(truth[name][~rows].any()) and not bool(d["yard"][name][~rows].any())


@pytest.mark.parametrize("c", sc.INV_CASES, ids=INV_IDS)
def test_invariance_case_is_decided(c):
    """Re-checks make_inv with torch: the lattice, the top-2 gap, the tie rows (torch.argmax takes the first maximum), the counts
    and the IoU by the reference's own route (one-hot tensors, einsum, clamp), the unused slots, the equal rows, and that the p = 1
    truth is exact in fp32."""
    d = sc.make_inv(c)
    PB, N, K = c.PB, c.N, c.K
    m1, m2 = torch.from_numpy(d["mask1"]), torch.from_numpy(d["mask2"])
    gap, ties = float("inf"), [0, 0]
    for which, m in ((0, m1), (1, m2)):
        v = m.double() * 64
        assert torch.equal(v, v.round()) and float(v.min()) >= 0 and float(v.max()) < 64
        arg = m.argmax(-1)
        assert torch.equal(arg, torch.from_numpy(d["arg%d" % (which + 1)]))
        if K == 1:
            continue
        top = v.topk(2, dim=2)[0]
        tie = torch.from_numpy(sc.tie_rows(N, which))
        assert bool((top[:, tie, 0] == top[:, tie, 1]).all())
        ties[which] = int(tie.sum())
        if tie.any():
            second = torch.where(v == top[..., :1], torch.arange(K), -1).max(dim=2)[0]     # the LAST maximum
            assert bool((second[:, tie] > arg[:, tie]).all())
        if (~tie).any():
            gap = min(gap, float((top[:, ~tie, 0] - top[:, ~tie, 1]).min()))
    eye = torch.eye(K, dtype=torch.float32)
    s1, s2 = eye[m1.argmax(-1)], eye[m2.argmax(-1)]
    inter = torch.einsum("bng,bnp->bgp", s1, s2)
    union = s1.sum(dim=1).unsqueeze(-1) + s2.sum(dim=1, keepdim=True) - inter
    iou = inter / union.clamp(1e-10)
    assert torch.equal(inter.long(), torch.from_numpy(d["counts"])) and bool((inter.sum(dim=(1, 2)) == N).all())
    assert torch.equal(iou, torch.from_numpy(d["iou"]))
    unused = int((iou.sum(dim=2) == 0).sum(dim=1).min())
    if K >= 4 and N > 1:
        assert unused >= K // 4
    col12 = torch.from_numpy(d["col12"]).long()
    assert bool((col12.sort(dim=1)[0] == torch.arange(K)).all())
    eq = torch.from_numpy(sc.equal_rows(N))
    target = torch.gather(m2, 2, col12.unsqueeze(1).expand(-1, N, K))
    assert torch.equal(target[:, eq], m1[:, eq]) and (N < 14 or bool(eq.any()))
    moved = float((col12 != torch.arange(K)).float().mean())
    if K > 1:
        assert gap >= 1 and moved > 0
    for x in d["truth"][1]:
        assert torch.equal(x.float().double(), x)
    errs = "  ".join("%s %.1e" % (n, sc.gate(t, y)[1]) for n, t, y in zip(("d12", "d21", "g1", "g2"), d["truth"][2], d["yard"][2]))
    print("%-18s top-2 gap %.0f/64  ties %d + %d  equal rows %d  unused slots %d  slots moved by the matching %.0f %%  "
          "torch32 error (p = 2): %s" % (sc.case_id(c), gap, ties[0], ties[1], int(eq.sum()), unused, 100 * moved, errs))


def test_case_list_reaches_its_branches():
    """The launch arithmetic of csrc/seg_loss.hip, replayed on the case lists."""
    dyn = {(c.VB, c.N, c.K): sc.sl_chunks(c.N, c.VB * c.K) for c in sc.DYN_CASES}
    assert dyn[(5, 6657, 32)] == (27, 14) and dyn[(32, 1025, 32)] == (5, 3) and dyn[(128, 600, 32)] == (3, 1)
    assert all(dyn[(2, n, k)] == (1, 1) for n in sc.N_EDGES[:-1] for k in (1, 2, 3)) and dyn[(2, 257, 1)] == (2, 2)
    assert {c.N for c in sc.DYN_EDGE_CASES} == {1, 63, 64, 65, 70, 255, 256, 257} and {c.K for c in sc.DYN_EDGE_CASES} == {1, 2, 3}
    fills = {c.K: -(-c.K * 12 // sc.THREADS) for c in sc.DYN_CASES}                # passes of the R | t fill
    assert fills[21] == 1 and fills[22] == 2 and fills[31] == 2 and fills[32] == 2 and 21 * 12 == 252
    assert any(c.VB == 3 and c.special == "all" for c in sc.DYN_CASES)
    assert len(_det_cases()) >= 8 and all(c in _det_cases() for c in sc.DYN_CHUNK_CASES[:2])
    inv = {(c.PB, c.N, c.K): sc.sl_chunks(c.N, c.PB) for c in sc.INV_CASES}
    assert inv[(64, 16641, 2)] == (66, 33) and inv[(2048, 600, 2)] == (3, 2)
    assert {(c.N, c.K) for c in sc.INV_EDGE_CASES} == {(n, k) for n in (1, 255, 256, 257) for k in (1, 2, 16, 17, 31, 32)}
    assert 16 * 16 == sc.THREADS < 17 * 17 and any(c.PB == 3 for c in sc.INV_CASES)
    assert max(c.K for c in sc.DYN_CASES + sc.INV_CASES) == sc.KMAX


def _det_cases():
    """The dynamic cases whose moments take more than one chunk: they also run in the deterministic mode."""
    return [c for c in sc.DYN_CASES if sc.sl_chunks(c.N, c.VB * c.K)[1] > 1]


# ---- GPU helpers ------------------------------------------------------------------------------------------------------------------
def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _ints(*shape):
    return torch.full(shape, -7, dtype=torch.int32, device=DEV)


def run_moments(nat, c, x):
    VB, N, K = c.VB, c.N, c.K
    mom = torch.full((VB * K * 16,), 7.0, dtype=torch.float64, device=DEV)
    S, means = _nan(VB * K, 9), _nan(VB * K, 6)
    nat.rigid_moments_wrapper(VB, N, K, x["pc"], x["pc2"], x["mask"], mom, S, means)
    return mom.cpu(), S.cpu(), means.cpu()


def run_fit(nat, c, S, means):
    VB, K = c.VB, c.K
    R, valid, t = _nan(VB * K, 9), _ints(VB * K), _nan(VB * K, 3)
    nat.kabsch_rotation_wrapper(VB * K, S, R, valid)
    nat.rigid_translation_wrapper(VB * K, means, valid, R, t)
    return R, t, valid


def run_blend(nat, c, x, R, t, p, backward, pc2=None):
    VB, N, K = c.VB, c.N, c.K
    out = _nan(VB, N, K) if backward else (_nan(VB, N, 3) if p == 0 else _nan(VB, N))
    nat.rigid_blend_wrapper(VB, N, K, p, backward, x["pc"], x["pc"] if pc2 is None else pc2, x["mask"], R, t,
                            x["grad"] if backward else None, out)
    return out.cpu()


def _moment_checks(tab, d, got, mode):
    mom, S, means = got
    VB, K = d["mom"].shape[:2]
    tab.same("mom" + mode, mom.view(VB, K, 16), torch.from_numpy(d["mom"]))
    tab.same_nan("S" + mode, S.view(VB, K, 9), torch.from_numpy(d["S32"]))
    tab.same_nan("means" + mode, means.view(VB, K, 6), torch.from_numpy(d["means32"]))


def _orth(R):
    R = R.double().view(-1, 3, 3)
    return R @ R.transpose(1, 2) - torch.eye(3, dtype=torch.float64)


# ---- the dynamic term -----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("c", sc.DYN_CASES, ids=DYN_IDS)
def test_dynamic_truth(nat, c):
    """ogc_rigid_moments (both modes where there is more than one chunk), ogc_kabsch_rotation + ogc_rigid_translation and
    ogc_rigid_blend (p = 0, 1, 2, forward and backward, on the kernels' own fit and on the truth's) on one case."""
    from ogc_amd import _lib, fused
    d = sc.make_dyn(c)
    VB, N, K = c.VB, c.N, c.K
    truth, yard, tab = d["truth"], d["yard"], Table(sc.case_id(c))
    x = {n: _dev(d[n]) for n in ("pc", "pc2", "mask", "grad")}
    before = _lib.DETERMINISTIC
    try:
        _lib.set_deterministic(False)
        got = run_moments(nat, c, x)
        _moment_checks(tab, d, got, "")
        if c in _det_cases():
            _lib.set_deterministic(True)
            assert _lib.load().ogc_get_deterministic() == 1
            _moment_checks(tab, d, run_moments(nat, c, x), " det")
    finally:
        _lib.set_deterministic(before)

    # the fit: the special slots exactly, the fitted ones against the truth
    R, t, valid = run_fit(nat, c, got[1].to(DEV), got[2].to(DEV))
    Rc, tc, live = R.cpu().view(-1, 3, 3), t.cpu(), torch.from_numpy(d["live"]).reshape(-1)
    tab.same("valid", valid.cpu(), (live >= 1).int())
    eye = torch.eye(3).expand(int((live <= 1).sum()), 3, 3)
    tab.same("R = I (no fit)", Rc[live <= 1], eye)
    tab.zero("t = 0 (no weight)", tc[live == 0])
    tab.zero("S = 0 (one point)", got[1][live == 1])
    for i in torch.nonzero(live == 1).reshape(-1).tolist():
        b, k = divmod(i, K)
        n = int(np.flatnonzero(d["mask"][b, :, k])[0])
        tab.same("t = q - p (one point)", tc[i], torch.from_numpy(d["pc2"][b, n] - d["pc"][b, n]))
    fit = d["fitted"]
    if fit.any():
        tab.check("R", Rc[fit], truth["R"][fit], yard["R"][fit])
        tab.check("t", tc[fit], truth["t"][fit], yard["t"][fit])
        tab.check("RR^T - I", _orth(Rc[fit]), _orth(truth["R"][fit]), _orth(yard["R"][fit]))
        tab.check("det R", torch.det(Rc[fit].double()), torch.det(truth["R"][fit]), torch.det(yard["R"][fit].double()))

    # the blend
    zero = torch.from_numpy(d["zero_rows"])
    own = {}
    for feed, Rf, tf in (("own", R, t), ("truth", truth["R"].float().reshape(-1, 9).to(DEV), truth["t"].float().to(DEV))):
        for p in (1, 2):
            out, g = run_blend(nat, c, x, Rf, tf, p, 0, x["pc2"]), run_blend(nat, c, x, Rf, tf, p, 1, x["pc2"])
            tab.check("out%d %s" % (p, feed), out, truth["out%d" % p], yard["out%d" % p])
            tab.check("g%d %s" % (p, feed), g, truth["g%d" % p], yard["g%d" % p])
            tab.zero("out%d %s zero rows" % (p, feed), out[zero])
            tab.zero("g%d %s zero rows" % (p, feed), g[zero])
            own[p, feed] = (out, g)
        tab.check("flow " + feed, run_blend(nat, c, x, Rf, tf, 0, 0), truth["flow"], yard["flow"])
        tab.check("diff " + feed, run_blend(nat, c, x, Rf, tf, 0, 0, x["pc2"]), truth["diff"], yard["diff"])

    # fused.rigid_residual composes the same five launches
    for p in (1, 2):
        assert fused.rigid_residual_available(x["mask"], p)
        mask = x["mask"].clone().requires_grad_(True)
        res = fused.rigid_residual(x["pc"], x["pc2"], mask, p)
        g, = torch.autograd.grad((res * x["grad"]).sum(), [mask])
        tab.same("rigid_residual p=%d" % p, res.detach().cpu(), own[p, "own"][0])
        tab.same("rigid_residual grad p=%d" % p, g.cpu(), own[p, "own"][1])
    tab.done()


# ---- the invariance term --------------------------------------------------------------------------------------------------------------
def run_distance(nat, c, x, col12, col21, p, backward):
    PB, N, K = c.PB, c.N, c.K
    o1, o2 = (_nan(PB, N, K), _nan(PB, N, K)) if backward else (_nan(PB, N), _nan(PB, N))
    nat.matched_distance_wrapper(PB, N, K, p, backward, x["mask1"], x["mask2"], col12, col21, x["g12"] if backward else None,
                                 x["g21"] if backward else None, o1, o2)
    return o1.cpu(), o2.cpu()


@gpu
@pytest.mark.parametrize("c", sc.INV_CASES, ids=INV_IDS)
def test_invariance_truth(nat, c):
    """ogc_mask_iou, ogc_lsap_maximize on its IoUs in both directions, ogc_matched_distance (p = 1 exactly, p = 2 through the
    table) and fused.matched_distances, which chains them."""
    from ogc_amd import fused
    d = sc.make_inv(c)
    PB, N, K = c.PB, c.N, c.K
    tab = Table(sc.case_id(c))
    x = {n: _dev(d[n]) for n in ("mask1", "mask2", "g12", "g21")}
    counts, iou = _ints(PB, K, K), _nan(PB, K, K)
    nat.mask_iou_wrapper(PB, N, K, x["mask1"], x["mask2"], counts, iou)
    tab.same("counts", counts.cpu().long(), torch.from_numpy(d["counts"]))
    tab.same("counts add up", counts.cpu().long().sum(dim=(1, 2)), torch.full((PB,), N))
    tab.same("iou", iou.cpu(), torch.from_numpy(d["iou"]))
    cols = _ints(2 * PB, K)
    nat.lsap_maximize_wrapper(2 * PB, K, torch.stack([iou, iou.transpose(1, 2)]).contiguous(), cols)
    tab.same("col12", cols[:PB].cpu(), torch.from_numpy(d["col12"]))
    tab.same("col21", cols[PB:].cpu(), torch.from_numpy(d["col21"]))
    col12, col21 = _dev(d["col12"]), _dev(d["col21"])
    eq = torch.from_numpy(sc.equal_rows(N))
    names = ("d12", "d21", "grad1", "grad2")
    direct = {}
    for p in (1, 2):
        got = run_distance(nat, c, x, col12, col21, p, 0) + run_distance(nat, c, x, col12, col21, p, 1)
        direct[p] = got
        for name, g, t, y in zip(names, got, d["truth"][p], d["yard"][p]):
            if p == 1:
                tab.same("%s p=1" % name, g, t.float())
            else:
                tab.check("%s p=2" % name, g, t, y)
        tab.zero("d12 p=%d equal rows" % p, got[0][:, eq])
        tab.zero("grad1 p=%d equal rows" % p, got[2][:, eq])
    for p in (1, 2):
        assert fused.matched_distance_available(x["mask1"], p, False)
        a, b = x["mask1"].clone().requires_grad_(True), x["mask2"].clone().requires_grad_(True)
        d12, d21 = fused.matched_distances(a, b, p)
        ga, gb = torch.autograd.grad((d12 * x["g12"]).sum() + (d21 * x["g21"]).sum(), [a, b])
        for name, g, want in zip(names, (d12.detach(), d21.detach(), ga, gb), direct[p]):
            tab.same("matched_distances %s p=%d" % (name, p), g.cpu(), want)
    tab.done()


# ---- the edges of the contract --------------------------------------------------------------------------------------------------------
@gpu
def test_more_than_32_slots_is_refused(nat):
    """K = 33: ogc_rigid_blend, ogc_mask_iou and ogc_matched_distance answer OGC_ERR_UNSUPPORTED (-3) and leave their outputs as
    they were; the availability gates of fused.py answer False for such a mask (and True at 32)."""
    from ogc_amd import _lib, fused
    VB, N, K = 2, 70, 33
    g = torch.Generator().manual_seed(33)
    pc, mask = torch.rand(VB, N, 3, generator=g).to(DEV), torch.rand(VB, N, K, generator=g).to(DEV)
    R, t = torch.eye(3, device=DEV).reshape(1, 9).repeat(VB * K, 1), torch.zeros(VB * K, 3, device=DEV)
    grad, cols = torch.ones(VB, N, device=DEV), torch.arange(K, dtype=torch.int32, device=DEV).repeat(VB, 1)
    outs = [_nan(VB, N, K), _nan(VB, N, K)]
    counts, iou = _ints(VB, K, K), _nan(VB, K, K)
    calls = [lambda p, bw: nat.rigid_blend_wrapper(VB, N, K, p, bw, pc, pc, mask, R, t, grad, outs[0]),
             lambda p, bw: nat.mask_iou_wrapper(VB, N, K, mask, mask, counts, iou),
             lambda p, bw: nat.matched_distance_wrapper(VB, N, K, p, bw, mask, mask, cols, cols, grad, grad, outs[0], outs[1])]
    for call in calls:
        for p, bw in ((1, 0), (2, 1)):
            with pytest.raises(_lib.OgcOpsError, match=r"status -3\).*more than 32 slots"):
                call(p, bw)
    torch.cuda.synchronize()
    assert bool(torch.isnan(outs[0]).all()) and bool(torch.isnan(outs[1]).all()) and bool(torch.isnan(iou).all())
    assert bool((counts == -7).all())
    misses = dict(fused.GATE_MISSES)
    try:
        for p in (1, 2):
            assert not fused.rigid_residual_available(mask, p) and fused.rigid_residual_available(mask[..., :32], p)
            assert not fused.matched_distance_available(mask, p, False) and fused.matched_distance_available(mask[..., :32], p, False)
    finally:
        fused.GATE_MISSES.clear()
        fused.GATE_MISSES.update(misses)


@gpu
def test_empty_shapes(nat):
    """VB = 0 or N = 0: the calls succeed and write what include/ogc_ops.h promises and nothing else.  ogc_rigid_moments with
    N = 0: zero moments, NaN S and means, and after ogc_kabsch_rotation / ogc_rigid_translation invalid, R = I, t = 0.
    ogc_mask_iou with N = 0: zero counts, zero IoUs (0 / 1e-10)."""
    K = 3
    buf = torch.zeros(64, device=DEV)
    ibuf = torch.zeros(64, dtype=torch.int32, device=DEV)
    e3 = ek = e1 = buf        # the wrappers take the sizes as arguments: an empty tensor has no pointer to give
    # N = 0
    mom = torch.full((2 * K * 16,), 7.0, dtype=torch.float64, device=DEV)
    S, means = torch.zeros(2 * K, 9, device=DEV), torch.zeros(2 * K, 6, device=DEV)
    nat.rigid_moments_wrapper(2, 0, K, e3, e3, ek, mom, S, means)
    assert not bool(mom.any()) and bool(torch.isnan(S).all()) and bool(torch.isnan(means).all())
    R, valid, t = _nan(2 * K, 9), _ints(2 * K), _nan(2 * K, 3)
    nat.kabsch_rotation_wrapper(2 * K, S, R, valid)
    nat.rigid_translation_wrapper(2 * K, means, valid, R, t)
    assert not bool(valid.any()) and not bool(t.any()) and torch.equal(R, torch.eye(3, device=DEV).reshape(1, 9).repeat(2 * K, 1))
    guard = _nan(16)
    for p, bw in ((0, 0), (1, 0), (2, 1)):
        nat.rigid_blend_wrapper(2, 0, K, p, bw, e3, e3, ek, R, t, e1, guard)
    counts, iou = _ints(2, K, K), _nan(2, K, K)
    nat.mask_iou_wrapper(2, 0, K, ek, ek, counts, iou)
    assert not bool(counts.any()) and not bool(iou.any())
    cols = ibuf[:2 * K].view(2, K)
    for p, bw in ((1, 0), (2, 1)):
        nat.matched_distance_wrapper(2, 0, K, p, bw, ek, ek, cols, cols, e1, e1, guard, guard)
    # VB = 0: nothing is touched
    z3 = zk = z1 = buf
    mom = torch.full((16,), 7.0, dtype=torch.float64, device=DEV)
    S, means = _nan(1, 9), _nan(1, 6)
    nat.rigid_moments_wrapper(0, 5, K, z3, z3, zk, mom, S, means)
    R, valid, t = _nan(1, 9), _ints(1), _nan(1, 3)
    nat.kabsch_rotation_wrapper(0, S, R, valid)
    nat.rigid_translation_wrapper(0, means, valid, R, t)
    for p, bw in ((0, 0), (1, 0), (2, 1)):
        nat.rigid_blend_wrapper(0, 5, K, p, bw, z3, z3, zk, R, t, z1, guard)
    counts, iou = _ints(1, K, K), _nan(1, K, K)
    nat.mask_iou_wrapper(0, 5, K, zk, zk, counts, iou)
    for p, bw in ((1, 0), (2, 1)):
        nat.matched_distance_wrapper(0, 5, K, p, bw, zk, zk, cols, cols, z1, z1, guard, guard)
    torch.cuda.synchronize()
    assert bool((mom == 7).all()) and bool((valid == -7).all()) and bool((counts == -7).all()) and bool(torch.isnan(guard).all())
    for x in (S, means, R, t, iou):
        assert bool(torch.isnan(x).all())

"""The FORWARD of a first level's chain (first pair -> pooled tail) over the live steps of its neighbour lists only
(ogc_live_steps_fwd and the two *_live kernels of csrc/conv1x1.hip, fused.LIVE_FORWARD): the tile-aligned list against a numpy
restatement of its rule; each list form against its dense form on NaN-filled outputs — values at live positions, statistics,
GroupNorm coefficients, extremes and pooled outputs bit for bit; one SA level with the switch on and off; preconditions.

The statistics bound.  Both forms add the SAME fp32 partial sums (one per 64-position tile, 16-row block and row quad) in fp64,
in an order that atomics decide.  Any order of n additions of values p_i in a format of unit roundoff u = 2^-53 ends within
(n - 1) u sum|p_i| (1 + O(n u)) of the exact sum, so two orders differ by at most 2 (n - 1) u sum|p_i|; sum|p_i| is bounded by the
sum of |y| (of y^2) over the group, taken in float64 from the dense output, times (1 + 2^-20) for the roundings inside a partial."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GROUPS = 4
EPS = 1e-5
B, P, NPTS, C0, C1, C2 = 2, 12, 200, 6, 32, 32
FILLS = (1, 1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)   # tests/test_live_steps_gpu.py's (the first 1: an all-zero row)
# the same fills in an order that makes the packing meet its hard cases (asserted in test_main_pattern_holds_the_hard_cases)
MAIN = (64, 48, 1, 63, 31, 17, 15, 33, 32, 49, 16, 1, 47, 2)
PATTERNS = {"main": MAIN, "ones": (1,), "full": (64,)}
CASES = [(64, 32), (64, 64), (32, 64)]
SHIFT = 28
MASK = (1 << SHIFT) - 1
PAD = -1


def _idx(S, fills, seed=5):
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
    """numpy restatement of the backward list: per sample the ascending packed entries."""
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


def _groups(entries):
    """the entries of one sample split into groups: runs with the same (entry & MASK) >> 2 — one dense 64-position tile each"""
    out = []
    for e in entries:
        if out and ((out[-1][0] & MASK) >> 2) == ((e & MASK) >> 2):
            out[-1].append(e)
        else:
            out.append([e])
    return out


def _fwd_rule(entries):
    """numpy restatement of the forward list: greedy pack, no group across a boundary between tiles of four, pads = -1."""
    out = []
    for g in _groups(entries):
        used = len(out) % 4
        if used + len(g) > 4:
            out += [PAD] * (4 - used)
        out += g
    return out


def _native():
    import ogc_amd  # noqa: F401
    from ogc_amd.pointnet2 import pointnet2 as api
    return api._native


def test_main_pattern_holds_the_hard_cases():
    """numpy only: the main pattern has a multi-entry group that would straddle a tile boundary in the unpadded list, a tile that
    mixes groups of different sizes, and a partial last tile.  (At S = 32 a group is a pair of centres with two to four entries,
    so only two groups of two can share a tile: no mixed tile exists there, and the S = 64 cases carry that one.)"""
    for S in (64, 32):
        straddle = mixed = partial = False
        for entries in _rule(_idx(S, MAIN)):
            at = 0
            for g in _groups(entries):
                straddle |= len(g) > 1 and at // 4 != (at + len(g) - 1) // 4
                at += len(g)
            fwd = _fwd_rule(entries)
            partial |= len(fwd) % 4 != 0
            for t0 in range(0, len(fwd), 4):
                sizes = {len(g) for g in _groups([e for e in fwd[t0:t0 + 4] if e != PAD])}
                mixed |= len(sizes) > 1
        assert straddle and partial, (S, straddle, partial)
        assert mixed or S == 32, S


@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("S", [64, 32])
def test_forward_list_equals_its_rule(S, pattern):
    """Every live entry once, ascending; no group across a tile boundary; pads marked; the count; `live` / `n_live` unchanged."""
    nat = _native()
    idx = _idx(S, PATTERNS[pattern])
    dev_idx = torch.from_numpy(idx).cuda()
    live, n_live, fwd, n_fwd = nat.live_steps_fwd_wrapper(dev_idx)
    live0, n_live0 = nat.live_steps_wrapper(dev_idx)
    want = _rule(idx)
    assert fwd.shape == live.shape == (B, P * S // 16)
    assert n_live.tolist() == n_live0.tolist() == [len(w) for w in want]
    for b in range(B):
        assert live[b, :len(want[b])].tolist() == live0[b, :len(want[b])].tolist() == want[b]
        got = fwd[b, :int(n_fwd[b])].tolist()
        assert got == _fwd_rule(want[b])
        assert [e for e in got if e != PAD] == want[b]                      # the same entries, ascending
        for t0 in range(0, len(got), 4):                                    # no group in two tiles
            for e in got[t0:t0 + 4]:
                if e != PAD:
                    assert all(((o & MASK) >> 2) != ((e & MASK) >> 2) for o in got[:t0] + got[t0 + 4:] if o != PAD)
    if pattern == "full":   # nothing skipped: every tile is one whole group
        assert n_fwd.tolist() == [P * S // 16] * B and not (fwd == PAD).any()


def _coeffs(nat, c, hw, gamma, beta, stats, slots):
    f32 = dict(dtype=torch.float32, device=stats.device)
    mean, rstd, a, bb = torch.empty(B * GROUPS, **f32), torch.empty(B * GROUPS, **f32), torch.empty(B * c, **f32), torch.empty(B * c, **f32)
    nat.group_norm_coeffs_wrapper(B, c, hw, GROUPS, EPS, None, gamma, beta, stats, slots, None, mean, rstd, a, bb)
    return mean, rstd, a, bb


def _check_stats(name, st_list, st_dense, y_dense, c, hw, slots):
    """fp64 statistics summed over the slots: within the bound for two orders of the same fp32 partial sums (module docstring)."""
    got = st_list.view(slots, B, GROUPS, 2).sum(0)
    want = st_dense.view(slots, B, GROUPS, 2).sum(0)
    y = y_dense.double().view(B, GROUPS, -1)
    n = (hw // 64) * (c // GROUPS // 4)          # partial sums per (sample, group)
    u = 2.0 ** -53
    for k, absum in ((0, y.abs().sum(-1)), (1, (y * y).sum(-1))):
        bound = 2.0 * (n - 1) * u * absum * (1.0 + 2.0 ** -20)
        err = (got[..., k] - want[..., k]).abs()
        print("%-10s stat %d  max err %.3e  min bound %.3e  partials %d" % (name, k, err.max().item(), bound.min().item(), n))
        assert (err <= bound).all(), (name, k, err.max().item(), bound.min().item())


_CACHE = {}


def _dense_chain(S, c3, pattern):
    """The chain's dense forward, kernel by kernel (computed once per case, never modified)."""
    key = (S, c3, pattern)
    if key in _CACHE:
        return _CACHE[key]
    nat = _native()
    idx_np = _idx(S, PATTERNS[pattern])
    g = torch.Generator().manual_seed(100 * S + c3)
    idx = torch.from_numpy(idx_np).cuda()
    pts = torch.randn(B, C0, NPTS, generator=g).cuda()
    x0 = torch.gather(pts.unsqueeze(2).expand(B, C0, P, NPTS), 3, idx.long().unsqueeze(1).expand(B, C0, P, S)).contiguous()
    w1 = (torch.randn(C1, C0, generator=g) / C0 ** 0.5).cuda()
    w2 = (torch.randn(C2, C1, generator=g) / C1 ** 0.5).cuda()
    w3 = (torch.randn(c3, C2, generator=g) / C2 ** 0.5).cuda()
    gam = [(1.0 + 0.25 * torch.randn(c, generator=g)).cuda() for c in (C1, C2, c3)]
    gam[2][::3] = -gam[2][::3]                     # both signs of the pooled norm's scale: largest and smallest extremes
    bet = [(0.25 * torch.randn(c, generator=g)).cuda() for c in (C1, C2, c3)]
    hw, dev = P * S, x0.device
    f32 = dict(dtype=torch.float32, device=dev)
    slots = nat.conv1x1_gn_slots()
    zst = lambda: torch.zeros(slots * B * GROUPS * 2, dtype=torch.float64, device=dev)
    st1 = zst()
    nat.first_conv_stats_wrapper(B, C1, C0, hw, GROUPS, x0, w1, st1)
    _, _, a1, bb1 = _coeffs(nat, C1, hw, gam[0], bet[0], st1, slots)
    y2, st2 = torch.empty(B, C2, P, S, **f32), zst()
    nat.conv1x1_gemm_affine_first_wrapper(B, C2, C1, hw, True, GROUPS, C0, w2, x0, w1, a1, bb1, y2, st2)
    co2 = _coeffs(nat, C2, hw, gam[1], bet[1], st2, slots)
    y3, st3 = torch.empty(B, c3, P, S, **f32), zst()
    yext, aext = torch.empty(B, c3, P, **f32), torch.empty(B, c3, P, dtype=torch.int32, device=dev)
    nat.conv1x1_gemm_affine_pool_wrapper(B, c3, C2, hw, True, GROUPS, S, w3, y2, co2[2], co2[3], gam[2], y3, st3, yext, aext)
    co3 = _coeffs(nat, c3, hw, gam[2], bet[2], st3, slots)
    keep = torch.zeros(B, hw, dtype=torch.bool)
    for b, entries in enumerate(_rule(idx_np)):
        for e in entries:
            keep[b, 16 * (e & MASK):16 * (e & MASK) + 16] = True
    k = dict(idx=idx, x0=x0, w1=w1, w2=w2, w3=w3, gam=gam, bet=bet, a1=a1, bb1=bb1, y2=y2, st2=st2, co2=co2, y3=y3, st3=st3,
             yext=yext, aext=aext, co3=co3, keep=keep.cuda(), hw=hw, slots=slots)
    _CACHE[key] = k
    return k


def _pool(nat, k, c3, S, yext, aext, st3):
    f32 = dict(dtype=torch.float32, device=yext.device)
    out, arg = torch.empty(B, c3, P, **f32), torch.empty(B, c3, P, dtype=torch.int32, device=yext.device)
    nat.group_norm_pool_extremes_wrapper(B, c3, P, S, GROUPS, EPS, True, yext, aext, k["gam"][2], k["bet"][2], out, arg,
                                         torch.empty(B * GROUPS, **f32), torch.empty(B * GROUPS, **f32), st3, k["slots"])
    return out, arg


@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("S,c3", CASES)
def test_list_forms_against_dense_forms(S, c3, pattern):
    nat = _native()
    k = _dense_chain(S, c3, pattern)
    hw, slots, dev = k["hw"], k["slots"], k["x0"].device
    f32 = dict(dtype=torch.float32, device=dev)
    nan = float("nan")
    _, _, fwd, n_fwd = nat.live_steps_fwd_wrapper(k["idx"])
    if pattern == "full":
        assert k["keep"].all()

    # ---- first pair: y2 at live positions, its statistics, the coefficients they give
    y2_l = torch.full((B, C2, P, S), nan, **f32)
    st2_l = torch.full_like(k["st2"], 3.0)          # (the entry point zeroes it)
    nat.conv1x1_gemm_affine_first_live_wrapper(B, C2, C1, hw, True, GROUPS, C0, S, k["w2"], k["x0"], k["w1"], k["a1"], k["bb1"], fwd,
                                               n_fwd, y2_l, st2_l)
    keep2 = k["keep"].unsqueeze(1).expand(B, C2, hw)
    assert torch.equal(y2_l.view(B, C2, hw)[keep2], k["y2"].view(B, C2, hw)[keep2])
    assert torch.isnan(y2_l.view(B, C2, hw)[~keep2]).all()
    _check_stats("pair", st2_l, k["st2"], k["y2"], C2, hw, slots)
    co2_l = _coeffs(nat, C2, hw, k["gam"][1], k["bet"][1], st2_l, slots)
    for name, got, want in zip(("mean", "rstd", "a", "bb"), co2_l, k["co2"]):
        assert torch.equal(got, want), "pair " + name

    # ---- pooled tail, fed the NaN-filled y2 the pair's list form wrote
    y3_l = torch.full((B, c3, P, S), nan, **f32)
    st3_l = torch.full_like(k["st3"], 3.0)
    yext_l, aext_l = torch.full((B, c3, P), nan, **f32), torch.full((B, c3, P), -7, dtype=torch.int32, device=dev)
    nat.conv1x1_gemm_affine_pool_live_wrapper(B, c3, C2, hw, True, GROUPS, S, k["w3"], y2_l, k["co2"][2], k["co2"][3], k["gam"][2],
                                              fwd, n_fwd, y3_l, st3_l, yext_l, aext_l)
    keep3 = k["keep"].unsqueeze(1).expand(B, c3, hw)
    assert torch.equal(y3_l.view(B, c3, hw)[keep3], k["y3"].view(B, c3, hw)[keep3])
    assert torch.isnan(y3_l.view(B, c3, hw)[~keep3]).all()
    _check_stats("tail", st3_l, k["st3"], k["y3"], c3, hw, slots)
    co3_l = _coeffs(nat, c3, hw, k["gam"][2], k["bet"][2], st3_l, slots)
    for name, got, want in zip(("mean", "rstd", "a", "bb"), co3_l, k["co3"]):
        assert torch.equal(got, want), "tail " + name
    assert torch.equal(aext_l, k["aext"])
    assert (yext_l == k["yext"]).all()
    out_d, arg_d = _pool(nat, k, c3, S, k["yext"], k["aext"], k["st3"])
    out_l, arg_l = _pool(nat, k, c3, S, yext_l, aext_l, st3_l)
    assert torch.equal(out_l, out_d) and torch.equal(arg_l, arg_d)

    # ---- the tail's list form on a DENSE y2 (the tail-only combination) gives the same
    y3_t = torch.full((B, c3, P, S), nan, **f32)
    st3_t, yext_t, aext_t = torch.zeros_like(k["st3"]), torch.full((B, c3, P), nan, **f32), torch.zeros_like(aext_l)
    nat.conv1x1_gemm_affine_pool_live_wrapper(B, c3, C2, hw, True, GROUPS, S, k["w3"], k["y2"], k["co2"][2], k["co2"][3],
                                              k["gam"][2], fwd, n_fwd, y3_t, st3_t, yext_t, aext_t)
    assert torch.equal(y3_t.view(B, c3, hw)[keep3], y3_l.view(B, c3, hw)[keep3])
    assert torch.equal(aext_t, aext_l) and (yext_t == yext_l).all()


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


FORWARD_WRAPPERS = ("conv1x1_gemm_affine_first_live_wrapper", "conv1x1_gemm_affine_pool_live_wrapper")


def test_sa_level_with_and_without_the_forward_list(monkeypatch):
    """The first level of segnet_kitti at N = 512, B = 2 (tests/test_live_steps_gpu.py): outputs bit-identical, parameter gradients
    at the golden gradient tolerance of the segnets; with the switch on both scales run both forward list forms, with it off none —
    and none when a condition of the chain fails (the one-node pooled tail switched off), with the output still right."""
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
    counting = _Counting(api._native, FORWARD_WRAPPERS)
    monkeypatch.setattr(api, "_native", counting)
    runs = {}
    for name, on, sparse_pool in (("on", True, True), ("off", False, True), ("broken", True, False)):
        monkeypatch.setattr(fused, "LIVE_FORWARD", on)
        monkeypatch.setattr(fused, "SPARSE_POOL_BACKWARD", sparse_pool)
        for n in counting.calls:
            counting.calls[n] = 0
        sa.zero_grad()
        out = sa(xyz, feats)[1]
        (out * probe).sum().backward()
        runs[name] = (out.detach().clone(), {n: p.grad.clone() for n, p in sa.named_parameters()}, dict(counting.calls))
    assert runs["on"][2] == {n: 2 for n in FORWARD_WRAPPERS}
    assert runs["off"][2] == {n: 0 for n in FORWARD_WRAPPERS} and runs["broken"][2] == {n: 0 for n in FORWARD_WRAPPERS}
    assert torch.equal(runs["on"][0], runs["off"][0]) and torch.equal(runs["broken"][0], runs["off"][0])
    grad_rtol = 1e-3   # tests/golden_cases.py: run_segnet
    for n, g_off in runs["off"][1].items():
        g_on = runs["on"][1][n]
        err, scale = (g_on - g_off).abs().max().item(), g_off.abs().max().item()
        print("%-40s err %.3e  scale %.3e" % (n, err, scale))
        assert torch.isfinite(g_on).all() and err <= grad_rtol * scale + 1e-8, n


def test_preconditions_are_reported():
    """Null list, bad nsample, a list without room for the worst case: an error status each, and no kernel (nor the memset in
    front of it) has run — the outputs keep their fill."""
    from ogc_amd import _lib
    nat = _native()
    S, c3 = 64, 32
    hw = P * S
    f32 = dict(dtype=torch.float32, device="cuda")
    idx = torch.from_numpy(_idx(S, MAIN)).cuda()
    _, _, fwd, n_fwd = nat.live_steps_fwd_wrapper(idx)
    short = fwd[:, :hw // 16 - 1].contiguous()
    x0, w1, w2, w3 = torch.randn(B, C0, P, S, **f32), torch.randn(C1, C0, **f32), torch.randn(C2, C1, **f32), torch.randn(c3, C2, **f32)
    y2_in = torch.randn(B, C2, P, S, **f32)
    a1, bb1, a2, bb2 = torch.randn(B * C1, **f32), torch.randn(B * C1, **f32), torch.randn(B * C2, **f32), torch.randn(B * C2, **f32)
    gamma3 = torch.randn(c3, **f32)
    slots = nat.conv1x1_gn_slots()
    for lv, nl, ns in ((None, None, S), (fwd, None, S), (fwd, n_fwd, 16), (fwd, n_fwd, 48), (short, n_fwd, S)):
        y2, y3 = torch.full((B, C2, P, S), 7.0, **f32), torch.full((B, c3, P, S), 7.0, **f32)
        st2 = torch.full((slots * B * GROUPS * 2,), 7.0, dtype=torch.float64, device="cuda")
        st3 = st2.clone()
        yext, aext = torch.full((B, c3, P), 7.0, **f32), torch.full((B, c3, P), 7, dtype=torch.int32, device="cuda")
        with pytest.raises(_lib.OgcOpsError):
            nat.conv1x1_gemm_affine_first_live_wrapper(B, C2, C1, hw, True, GROUPS, C0, ns, w2, x0, w1, a1, bb1, lv, nl, y2, st2)
        with pytest.raises(_lib.OgcOpsError):
            nat.conv1x1_gemm_affine_pool_live_wrapper(B, c3, C2, hw, True, GROUPS, ns, w3, y2_in, a2, bb2, gamma3, lv, nl, y3, st3,
                                                      yext, aext)
        for t in (y2, y3, st2, st3, yext, aext):
            assert t.eq(7).all()
    with pytest.raises(_lib.OgcOpsError):   # the forward list needs nsample 32 or 64
        nat.live_steps_fwd_wrapper(torch.zeros(B, P, 16, dtype=torch.int32, device="cuda"))

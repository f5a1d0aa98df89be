"""The GroupNorm-adjoint backward kernels of csrc/gn_fused_bwd.hip (and the adjoint form of csrc/conv1x1_h.hip) on inputs where no
rounding can happen, so that no tolerance is needed — in the manner of test_wgrad_exact_gpu.py.

Every input is a small integer: y_prev and y / grad_y in [-4, 4], the folded norm pa in {-2, -1, 1, 2} and pb in [-3, 3], the
pooled GroupNorm's coef2 = (c2 in [-2, 2], c3 in [-3, 3]) and inj = (ag in [-8, 8], arg as int bits), the weights in [-2, 2], the
adjoint's coef = (alpha, c2, c3) in [-2, 2]^3, and for the first-layer forms x0 and w1 in [-2, 2] (the recomputed y1 = w1 x0 is
then an exact integer, |y1| <= 32).  Every operand is an integer below 256, which bf16 holds, and every partial sum stays below
2^24 (asserted on the host for every case), where fp32 holds every integer.  So every result has to EQUAL the integer evaluation
in every kernel and every summation order.  The expected values are products of integers formed in float64 on the device (exact:
every sum is asserted below 2^53) and held as int64.

Moment matrices (ogc_conv1x1_wgrad_moments*):   H[b, m, k] = sum_p g[b, m, p] mask[b, k, p],   H2 = sum_p g mask y_prev,   with
mask = [pa y_prev + pb > 0] (all ones at relu = 0) and, in the pooled forms, g = c2 y + c3 + [p % S == arg] ag.
Geometries (b, hw), from moments_launch — at these sizes a wave takes 8 steps (16 positions in fp32, 32 in bf16), a workgroup 32:
    one step                    (1, 16) / (1, 32)       waves 1 .. 3 have none
    nine steps                  (3, 144) / (3, 288)     wave 1 has a single, odd step; waves 2 and 3 none
    36 steps                    (1 and 3, 576 / 1152)   a second chunk per sample with one live wave: blockIdx.x -> (sample, chunk)
The first-layer forms need hw % 64 == 0: 64 (four steps), 192 (twelve: wave 1 half full) and 576.
Channel pairs: one per rung of the tile ladder, then ragged and wide.

Input gradient (ogc_conv1x1_dgrad_adjoint*):   alpha mask (sum_k w[k, m] g[b, k, p]) + c2 y_prev + c3, rounded to bf16 by torch
for the 16-bit forms; for the first-layer forms the weight gradient dW1[m, c] = sum_{b, p} g_prev[b, m, p] x0[b, c, p] of it.
cout: one per KQ rung (32, 64, 100, 132, 160) and a ragged one (30); cin: 16, 64, 67 (a ragged row tile), 131 (three row tiles);
hw: 64 and 320 (one and two workgroups per sample, the second with one live wave); b: 1 and 3.  The pooled forms run at every
nsample; where the entry point's LDS check (dgrad_adjoint_impl) refuses the width, and only there, the case is skipped.

List forms: neighbour lists with per-centre fills 1, 15, 16, 17, S - 1, S; the lists come from live_steps_wrapper; the inputs are
per-point integers gathered through idx (repeats carry equal values, as in the product), every arg lies below its centre's fill,
and the inputs are NaN at the positions of skipped steps, which a list form may not read.  Expected: the dense integers."""
import functools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
F32 = torch.float32
NSAMPLES = (16, 32, 64)

CHANNELS = [(16, 16), (16, 32), (32, 32), (16, 64), (32, 64), (64, 32), (64, 64),   # one per rung of the ladder
            (3, 17), (35, 67), (100, 160)]                                          # ragged, wide
GEOM = {F32: [(1, 16), (3, 144), (1, 576), (3, 576)], BF: [(1, 32), (3, 288), (1, 1152), (3, 1152)]}
GEOM_FIRST = [(1, 64), (3, 192), (1, 576), (3, 576)]
D_COUT, D_CIN, D_HW, D_B = (32, 64, 100, 132, 160, 30), (16, 64, 67, 131), (64, 320), (1, 3)


@pytest.fixture()
def nat():
    import ogc_amd  # noqa: F401
    from ogc_amd.pointnet2 import pointnet2 as api
    n = api._native
    precision = n.get_matmul_precision()
    try:
        yield n
    finally:
        n.set_matmul_precision(precision)


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g, dtype=torch.int64)


def _prod(eq, *ops):
    """An integer product, exact: float64 on the device with every sum below 2^53, returned as int64."""
    bound = 1
    for o in ops:
        bound *= max(int(o.abs().max()), 1)
    assert bound * max(max(o.shape) for o in ops) < 2 ** 53
    return torch.einsum(eq, *[o.to(DEV).double() for o in ops]).round().long()


def _inj(ag, arg):
    inj = torch.empty(*ag.shape, 2)
    inj[..., 0] = ag.float()
    inj[..., 1] = arg.int().view(F32)   # the index travels as int bits (test_act16_gpu._sparse)
    return inj.to(DEV)


def _rebuild(y, c2, c3, ag, arg, s):
    """g = c2 y + c3 + [p % S == arg] ag"""
    b, c, hw = y.shape
    g = (c2[:, :, None] * y + c3[:, :, None]).view(b, c, hw // s, s)
    return g.scatter_add(3, arg.unsqueeze(-1), ag.unsqueeze(-1)).view(b, c, hw)


def _common(g, b, cin, cout):
    """What every case draws besides its tensors."""
    return {"pa": torch.tensor([-2, -1, 1, 2])[_ints(g, 0, 3, b, cin)], "pb": _ints(g, -3, 3, b, cin),
            "c2": _ints(g, -2, 2, b, cout), "c3": _ints(g, -3, 3, b, cout),
            "w": _ints(g, -2, 2, cout, cin), "coef": _ints(g, -2, 2, b, cin, 3)}


def _dev(c):
    """The device copies every entry point takes."""
    for k in ("pa", "pb"):
        c[k, "dev"] = c[k].float().reshape(-1).to(DEV)
    c["coef2"] = torch.stack((c["c2"], c["c3"]), dim=-1).float().contiguous().to(DEV)
    c["w", "dev"] = c["w"].float().to(DEV)
    c["coef", "dev"] = c["coef"].float().contiguous().to(DEV)
    return c


@functools.lru_cache(maxsize=None)
def _inputs(cin, cout, b, hw):
    """The integer inputs of one dense / pooled case (int64, host) and their device copies in both storage types."""
    g = torch.Generator().manual_seed(1000003 * cin + 10007 * cout + 101 * b + hw)
    c = _common(g, b, cin, cout)
    c["yp"], c["y"] = _ints(g, -4, 4, b, cin, hw), _ints(g, -4, 4, b, cout, hw)
    for s in NSAMPLES:
        if hw % s == 0:
            c["ag", s], c["arg", s] = _ints(g, -8, 8, b, cout, hw // s), _ints(g, 0, s - 1, b, cout, hw // s)
            c["inj", s] = _inj(c["ag", s], c["arg", s])
    for k in ("yp", "y"):
        c[k, F32], c[k, BF] = c[k].float().to(DEV), c[k].to(BF).to(DEV)
    return _dev(c)


def _mask(c, relu):
    m = c["pa"][:, :, None] * c["yp"] + c["pb"][:, :, None] > 0 if relu else torch.ones_like(c["yp"], dtype=torch.bool)
    return m.long()


def _gy(c, s):
    return _rebuild(c["y"], c["c2"], c["c3"], c["ag", s], c["arg", s], s) if s else c["y"]


def _want_moments(c, relu, s):
    """(b, 2, cout, cin): H, H2 as integers, on the device as fp32."""
    gy, mask = _gy(c, s), _mask(c, relu)
    hw = gy.shape[2]
    # sum_p |g| |mask y_prev| <= max |g| max |y_prev| hw: below 2^24 every fp32 partial sum is an exact integer
    assert int(gy.abs().max()) * max(int(c["yp"].abs().max()), 1) * hw < 2 ** 24
    h = torch.stack((_prod("bmp,bkp->bmk", gy, mask), _prod("bmp,bkp->bmk", gy, mask * c["yp"])), dim=1)
    return h.float()


def _want_dgrad(c, relu, s):
    """(b, cin, hw) int64 on the device: alpha mask (w^T g) + c2 y_prev + c3."""
    gy, mask = _gy(c, s), _mask(c, relu)
    gz = _prod("km,bkp->bmp", c["w"], gy)
    co = c["coef"].to(DEV)
    out = co[:, :, 0:1] * mask.to(DEV) * gz + co[:, :, 1:2] * c["yp"].to(DEV) + co[:, :, 2:3]
    assert int(gz.abs().max()) * 2 + 2 * int(c["yp"].abs().max()) + 2 < 2 ** 24 and int(out.abs().max()) < 2 ** 24
    return out


def _nan_moments(b, cin, cout):
    return torch.full((b, 2, cout, cin), float("nan"), device=DEV)   # (the entry points zero the matrices themselves)


# ---- moment matrices, dense and pooled -----------------------------------------------------------------------------------------

def _run_moments(nat, dt, pooled, relu):
    nat.set_matmul_precision("bf16" if dt is BF else "fp32")
    launched, bad = 0, []
    for cin, cout in CHANNELS:
        for b, hw in GEOM[dt]:
            c = _inputs(cin, cout, b, hw)
            for s in (NSAMPLES if pooled else (0,)):
                if s and hw % s:
                    continue
                hm = _nan_moments(b, cin, cout)
                if s:
                    nat.conv1x1_wgrad_moments_pooled_wrapper(b, cin, cout, hw, relu, s, c["yp", dt], c["pa", "dev"], c["pb", "dev"],
                                                             c["y", dt], c["coef2"], c["inj", s], hm)
                else:
                    nat.conv1x1_wgrad_moments_wrapper(b, cin, cout, hw, relu, c["yp", dt], c["pa", "dev"], c["pb", "dev"], c["y", dt], hm)
                launched += 1
                if not torch.equal(hm, _want_moments(c, relu, s)):
                    bad.append((cin, cout, b, hw, s))
    assert launched >= len(CHANNELS) * len(GEOM[dt])
    assert not bad, "H / H2 differ from the integers at (cin, cout, b, hw, nsample) %s" % bad


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("dt", [F32, BF], ids=["fp32", "h"])
def test_moments_dense_exact(nat, dt, relu):
    _run_moments(nat, dt, False, relu)


@pytest.mark.parametrize("dt", [F32, BF], ids=["fp32", "h"])
def test_moments_pooled_exact(nat, dt):
    """Every nsample of 16, 32, 64 that divides hw, with the ReLU of the folded norm on."""
    _run_moments(nat, dt, True, 1)


# ---- first-layer forms ---------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _first_inputs(c0, cin, cout, b, hw):
    g = torch.Generator().manual_seed(7 + 1000003 * cin + 10007 * cout + 101 * b + hw + 13 * c0)
    c = _common(g, b, cin, cout)
    c["x0"], c["w1"], c["y"] = _ints(g, -2, 2, b, c0, hw), _ints(g, -2, 2, cin, c0), _ints(g, -4, 4, b, cout, hw)
    c["yp"] = torch.einsum("mc,bcp->bmp", c["w1"], c["x0"])   # y1, never stored by the kernels
    c["x0", "dev"], c["w1", "dev"], c["y", F32] = c["x0"].float().to(DEV), c["w1"].float().to(DEV), c["y"].float().to(DEV)
    return _dev(c)


@pytest.mark.parametrize("c0", [3, 6, 8])
def test_moments_first_exact(nat, c0):
    nat.set_matmul_precision("fp32")
    bad = []
    for cin, cout in [p for p in CHANNELS if p[0] <= 64]:
        for b, hw in GEOM_FIRST:
            c = _first_inputs(c0, cin, cout, b, hw)
            hm = _nan_moments(b, cin, cout)
            nat.conv1x1_wgrad_moments_first_wrapper(b, cin, cout, hw, 1, c0, c["x0", "dev"], c["w1", "dev"], c["pa", "dev"],
                                                    c["pb", "dev"], c["y", F32], hm)
            if not torch.equal(hm, _want_moments(c, 1, 0)):
                bad.append((cin, cout, b, hw))
    assert not bad, "H / H2 differ from the integers at (cin, cout, b, hw) %s" % bad


def _want_dw1(c, g_prev):
    dw1 = _prod("bmp,bcp->mc", g_prev, c["x0"])
    assert int(g_prev.abs().max()) * int(c["x0"].abs().max()) * g_prev.shape[0] * g_prev.shape[2] < 2 ** 24
    return dw1.float()


@pytest.mark.parametrize("c0", [3, 6, 8])
def test_dgrad_first_exact(nat, c0):
    """cout <= 64 (the entry point's limit): both KQ rungs and the ragged width."""
    nat.set_matmul_precision("fp32")
    bad = []
    for cout in (32, 64, 30):
        for cin in (16, 64, 35):
            for hw in D_HW:
                for b in D_B:
                    c = _first_inputs(c0, cin, cout, b, hw)
                    dw1 = torch.full((cin, c0), float("nan"), device=DEV)
                    nat.conv1x1_dgrad_adjoint_first_wrapper(b, cin, cout, hw, 1, c0, c["w", "dev"], c["y", F32], c["x0", "dev"],
                                                            c["w1", "dev"], c["pa", "dev"], c["pb", "dev"], c["coef", "dev"], dw1)
                    if not torch.equal(dw1, _want_dw1(c, _want_dgrad(c, 1, 0))):
                        bad.append((cin, cout, b, hw))
    assert not bad, "dW1 differs from the integers at (cin, cout, b, hw) %s" % bad


# ---- input gradient, dense and pooled ------------------------------------------------------------------------------------------

def _lds_refused(cout, s):
    """dgrad_adjoint_impl: the weight tile, the 64 x 5 coefficients and the pooled table (4 waves x cout x 64 / nsample float4)
    against 64 KiB."""
    kq = (cout + 3) // 4
    return (64 * 4 * (kq | 1) + 64 * 5) * 4 + 4 * cout * (64 // s) * 16 > 64 * 1024


def _run_dgrad(nat, dt, pooled, relu):
    from ogc_amd._lib import OgcOpsError
    nat.set_matmul_precision("bf16" if dt is BF else "fp32")
    ran, bad = set(), []
    for cout in D_COUT:
        for cin in D_CIN:
            for hw in D_HW:
                for b in D_B:
                    c = _inputs(cin, cout, b, hw)
                    for s in (NSAMPLES if pooled else (0,)):
                        out = torch.full((b, cin, hw), float("nan"), device=DEV, dtype=dt)
                        args = (c["yp", dt], c["pa", "dev"], c["pb", "dev"], c["coef", "dev"], out)
                        if not s:
                            nat.conv1x1_dgrad_adjoint_wrapper(b, cin, cout, hw, relu, c["w", "dev"], c["y", dt], *args)
                        elif _lds_refused(cout, s):
                            with pytest.raises(OgcOpsError, match="LDS"):
                                nat.conv1x1_dgrad_adjoint_pooled_wrapper(b, cin, cout, hw, relu, s, c["w", "dev"], c["y", dt], c["coef2"],
                                                                         c["inj", s], *args)
                            continue
                        else:
                            nat.conv1x1_dgrad_adjoint_pooled_wrapper(b, cin, cout, hw, relu, s, c["w", "dev"], c["y", dt], c["coef2"],
                                                                     c["inj", s], *args)
                        ran.add((cout, s))
                        if not torch.equal(out, _want_dgrad(c, relu, s).float().to(dt)):
                            bad.append((cin, cout, b, hw, s))
    assert all((cout, s) in ran for cout in (30, 32, 64) for s in (NSAMPLES if pooled else (0,)))   # at least the widths up to 64
    assert not bad, "grad_prev differs from the integers at (cin, cout, b, hw, nsample) %s" % bad


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("dt", [F32, BF], ids=["fp32", "h"])
def test_dgrad_dense_exact(nat, dt, relu):
    _run_dgrad(nat, dt, False, relu)


@pytest.mark.parametrize("dt", [F32, BF], ids=["fp32", "h"])
def test_dgrad_pooled_exact(nat, dt):
    _run_dgrad(nat, dt, True, 1)


@pytest.mark.parametrize("ch", [16, 64])
def test_dgrad_persistent_exact(nat, ch):
    """b * hw / 64 = 8192 position tiles: the dense 16-bit form goes to the persistent kernel of conv1x1_h.hip
    (ogc_gemm16_adjoint_launch), and with OGC_GEMM16=0 to dgrad_adjoint_kernel.  Both hold the shared adjoint expression; both
    equal the integers."""
    nat.set_matmul_precision("bf16")
    b, hw = 2, 64 * 4096
    c = _inputs(ch, ch, b, hw)
    want = _want_dgrad(c, 1, 0).float().to(BF)
    try:
        for mode in (None, "0"):
            if mode is None:
                os.environ.pop("OGC_GEMM16", None)
            else:
                os.environ["OGC_GEMM16"] = mode
            out = torch.full((b, ch, hw), float("nan"), device=DEV, dtype=BF)
            nat.conv1x1_dgrad_adjoint_wrapper(b, ch, ch, hw, 1, c["w", "dev"], c["y", BF], c["yp", BF], c["pa", "dev"], c["pb", "dev"],
                                              c["coef", "dev"], out)
            assert torch.equal(out, want), "OGC_GEMM16=%s" % mode
    finally:
        os.environ.pop("OGC_GEMM16", None)
        _inputs.cache_clear()   # (two tensors of 64 MiB)


# ---- list forms ----------------------------------------------------------------------------------------------------------------

LB, LNPTS = 2, 50


def _fills(S):
    return (1, 15, 16, 17, S - 1, S)


@functools.lru_cache(maxsize=None)
def _list_inputs(S, P, cin, cout, c0):
    """idx (LB, P, S) with the fills of _fills(S) in turn; per-point integers gathered through it; the lists of live_steps_wrapper;
    the mask of positions in live steps."""
    import ogc_amd  # noqa: F401
    from ogc_amd.pointnet2 import pointnet2 as api
    g = torch.Generator().manual_seed(31 * S + P + 1009 * cin + 17 * cout + c0)
    fills = torch.tensor([_fills(S)[r % 6] for r in range(LB * P)]).view(LB, P)
    idx = _ints(g, 1, LNPTS - 1, LB, P, S)
    first = idx[:, :, :1].clone()
    col = torch.arange(S).view(1, 1, S)
    last = (first + 1 + _ints(g, 0, LNPTS - 3, LB, P, 1)) % LNPTS                        # != first
    idx = torch.where(col == fills.unsqueeze(-1) - 1, last, idx)                         # the last live column differs from column 0
    idx = torch.where((col >= fills.unsqueeze(-1)) | (col == 0), first, idx)             # trailing columns repeat column 0
    hw = P * S
    c = _common(g, LB, cin, cout)

    def gather(ch, lo, hi):
        pts = _ints(g, lo, hi, LB, ch, LNPTS)
        return torch.gather(pts.unsqueeze(2).expand(LB, ch, P, LNPTS), 3, idx.unsqueeze(1).expand(LB, ch, P, S)).reshape(LB, ch, hw)
    c["y"] = gather(cout, -4, 4)
    if c0:
        c["x0"], c["w1"] = gather(c0, -2, 2), _ints(g, -2, 2, cin, c0)
        c["yp"] = torch.einsum("mc,bcp->bmp", c["w1"], c["x0"])
    else:
        c["yp"] = gather(cin, -4, 4)
    c["ag", S] = _ints(g, -8, 8, LB, cout, P)
    c["arg", S] = (_ints(g, 0, S - 1, LB, cout, P) % fills.unsqueeze(1))                 # below the centre's fill
    c["inj", S] = _inj(c["ag", S], c["arg", S])
    c["live"], c["n_live"] = api._native.live_steps_wrapper(idx.int().to(DEV))
    s_star = torch.minimum(fills // 16, torch.tensor(S // 16 - 1))                       # live steps 0 .. s* of every centre
    c["live_pos"] = (col // 16 <= s_star.unsqueeze(-1)).reshape(LB, 1, hw).to(DEV)
    nan = torch.tensor(float("nan"), device=DEV)
    for k in ("y", "yp") + (("x0",) if c0 else ()):                                      # NaN where a list form may not read
        c[k, "nan"] = torch.where(c["live_pos"], c[k].float().to(DEV), nan)
    if c0:
        c["w1", "dev"] = c["w1"].float().to(DEV)
    return _dev(c)


LIST_CASES = [(S, P, cin, cout) for S in (32, 64) for P in (6, 18) for cin, cout in ((16, 16), (35, 67), (64, 64))]


def test_moments_list_forms_exact(nat):
    """_pooled_live, _live and _first_live: the dense integers from inputs that are NaN at every skipped step."""
    nat.set_matmul_precision("fp32")
    bad = []
    for S, P, cin, cout in LIST_CASES:
        hw = P * S
        c = _list_inputs(S, P, cin, cout, 0)
        com = (c["yp", "nan"], c["pa", "dev"], c["pb", "dev"], c["y", "nan"])
        hm = _nan_moments(LB, cin, cout)
        nat.conv1x1_wgrad_moments_pooled_live_wrapper(LB, cin, cout, hw, 1, S, *com, c["coef2"], c["inj", S], c["live"], c["n_live"], hm)
        if not torch.equal(hm, _want_moments(c, 1, S)):
            bad.append(("pooled_live", S, P, cin, cout))
        hm = _nan_moments(LB, cin, cout)
        nat.conv1x1_wgrad_moments_live_wrapper(LB, cin, cout, hw, 1, S, *com, c["live"], c["n_live"], hm)
        if not torch.equal(hm, _want_moments(c, 1, 0)):
            bad.append(("live", S, P, cin, cout))
        f = _list_inputs(S, P, cin, cout, 6)
        hm = _nan_moments(LB, cin, cout)
        nat.conv1x1_wgrad_moments_first_live_wrapper(LB, cin, cout, hw, 1, 6, S, f["x0", "nan"], f["w1", "dev"], f["pa", "dev"],
                                                     f["pb", "dev"], f["y", "nan"], f["live"], f["n_live"], hm)
        if not torch.equal(hm, _want_moments(f, 1, 0)):
            bad.append(("first_live", S, P, cin, cout))
    assert not bad, "H / H2 differ from the dense integers at (form, S, P, cin, cout) %s" % bad


def test_dgrad_list_forms_exact(nat):
    """_live_fill equals the dense integers at every position; _pooled_live at the positions of live steps, and the NaN the output
    was filled with survives everywhere else; _first_live gives the dense dW1."""
    nat.set_matmul_precision("fp32")
    bad = []
    for S, P, cin, cout in LIST_CASES:
        hw = P * S
        c = _list_inputs(S, P, cin, cout, 0)
        tail = (c["yp", "nan"], c["pa", "dev"], c["pb", "dev"], c["coef", "dev"], c["live"], c["n_live"])
        out = torch.full((LB, cin, hw), float("nan"), device=DEV)
        nat.conv1x1_dgrad_adjoint_live_fill_wrapper(LB, cin, cout, hw, 1, S, c["w", "dev"], c["y", "nan"], *tail, out)
        if not torch.equal(out, _want_dgrad(c, 1, 0).float()):
            bad.append(("live_fill", S, P, cin, cout))
        out = torch.full((LB, cin, hw), float("nan"), device=DEV)
        nat.conv1x1_dgrad_adjoint_pooled_live_wrapper(LB, cin, cout, hw, 1, S, c["w", "dev"], c["y", "nan"], c["coef2"], c["inj", S],
                                                      *tail, out)
        want = torch.where(c["live_pos"], _want_dgrad(c, 1, S).float(), torch.tensor(float("nan"), device=DEV))
        if not torch.equal(torch.isnan(out), torch.isnan(want)) or not torch.equal(out.nan_to_num(0.0), want.nan_to_num(0.0)):
            bad.append(("pooled_live", S, P, cin, cout))
        cout = cout if cout <= 64 else 30                                                # (the first-layer forms' limit)
        f = _list_inputs(S, P, cin, cout, 6)
        dw1 = torch.full((cin, 6), float("nan"), device=DEV)
        nat.conv1x1_dgrad_adjoint_first_live_wrapper(LB, cin, cout, hw, 1, 6, S, f["w", "dev"], f["y", "nan"], f["x0", "nan"],
                                                     f["w1", "dev"], f["pa", "dev"], f["pb", "dev"], f["coef", "dev"], f["live"],
                                                     f["n_live"], dw1)
        if not torch.equal(dw1, _want_dw1(f, _want_dgrad(f, 1, 0))):
            bad.append(("first_live", S, P, cin, cout))
    assert not bad, "the list forms differ from the dense integers at (form, S, P, cin, cout) %s" % bad

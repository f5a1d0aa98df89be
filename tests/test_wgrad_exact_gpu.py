"""The weight-gradient kernels of csrc/conv1x1_wgrad.hip on inputs where no rounding can happen, so that no tolerance is needed.

Every input is a small integer: x and dy / y in [-4, 4], the folded norm pa in {-2, -1, 1, 2} and pb in [-3, 3], the pooled
GroupNorm's coefficients c2 in [-2, 2], c3 in [-3, 3] and its injected value ag in [-8, 8] at a uniform neighbour index.  The
operands act(pa x + pb) (|.| <= 11) and c2 y + c3 + ag (|.| <= 19) are integers that bf16 holds exactly, and every partial sum
of their products stays below 2^24 (asserted on the host for every case), where fp32 holds every integer.  So dW has to EQUAL
the int64 product in every kernel and in every summation order: fp32 or bf16 operands, 16- or 32-position register tiles, the
shared 128 x 128 tile with fp32 or packed stages, atomics or the deterministic mode's slabs.

Geometries (b, hw) are the smallest that exercise the walks: one step; nine 16-position steps at eight per wave (wave 0 crosses
two image boundaries, wave 1 has a single odd step, waves 2 and 3 none); 8 + 2 and 8 + 1 steps of 32 positions; one and nine
stages of the shared tiles.  Which kernel serves a case follows from the entry point, the channel counts and hw, as in
wgrad_impl: every form runs at every geometry and every channel pair, plus 131 -> 128 at hw = 48 (register tiles at wide
widths)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16

GEOMETRIES = [(1, 16), (3, 48), (5, 64), (3, 96), (1, 32), (1, 64), (3, 192)]
CHANNELS = [(16, 16), (16, 32), (32, 32), (16, 64), (32, 64), (64, 32), (64, 64),   # one per register tile
            (3, 17), (35, 67),                                                      # ragged
            (128, 128), (131, 129)]                                                 # wide
CASES = [(cin, cout, b, hw) for cin, cout in CHANNELS for b, hw in GEOMETRIES] + [(131, 128, 3, 48)]
NSAMPLES = (16, 32, 64)


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g, dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def _inputs(cin, cout, b, hw):
    """The integer inputs of one case (int64, host) and their device copies in both storage types."""
    g = torch.Generator().manual_seed(1000003 * cin + 10007 * cout + 101 * b + hw)
    c = {"x": _ints(g, -4, 4, b, cin, hw), "y": _ints(g, -4, 4, b, cout, hw),
         "pa": torch.tensor([-2, -1, 1, 2])[_ints(g, 0, 3, b, cin)], "pb": _ints(g, -3, 3, b, cin),
         "c2": _ints(g, -2, 2, b, cout), "c3": _ints(g, -3, 3, b, cout)}
    for s in NSAMPLES:
        if hw % s == 0:
            c["ag", s] = _ints(g, -8, 8, b, cout, hw // s)
            c["arg", s] = _ints(g, 0, s - 1, b, cout, hw // s)
            inj = torch.empty(b, cout, hw // s, 2)
            inj[..., 0] = c["ag", s].float()
            inj[..., 1] = c["arg", s].int().view(torch.float32)   # the index travels as int bits (test_act16_gpu._sparse)
            c["inj", s] = inj.to(DEV)
    for k in ("x", "y"):
        c[k, torch.float32] = c[k].float().to(DEV)
        c[k, BF] = c[k].to(BF).to(DEV)
    for k in ("pa", "pb"):
        c[k, "dev"] = c[k].float().reshape(-1).to(DEV)
    c["coef2"] = torch.stack((c["c2"], c["c3"]), dim=-1).float().contiguous().to(DEV)
    return c


@functools.lru_cache(maxsize=None)
def _want(cin, cout, b, hw, act, nsample):
    """dW of one case as int64 arithmetic gives it.  act: None (x itself), 0 (pa x + pb), 1 (relu of it); nsample: 0 (dy = y is
    the gradient) or the neighbourhood size of the pooled form (the gradient is rebuilt from y)."""
    c = _inputs(cin, cout, b, hw)
    a = c["x"]
    if act is not None:
        a = c["pa"][:, :, None] * a + c["pb"][:, :, None]
        if act:
            a = a.clamp_min(0)
    gy = c["y"]
    if nsample:
        gy = (c["c2"][:, :, None] * gy + c["c3"][:, :, None]).view(b, cout, hw // nsample, nsample)
        gy = gy.scatter_add(3, c["arg", nsample].unsqueeze(-1), c["ag", nsample].unsqueeze(-1)).view(b, cout, hw)
    # sum_p |g| |act| <= max |g| max |act| b hw for every element of dW: below 2^24 every fp32 partial sum is an exact integer
    assert int(gy.abs().max()) * int(a.abs().max()) * b * hw < 2 ** 24
    want = torch.einsum("bmp,bkp->mk", gy, a)
    assert want.dtype == torch.int64
    return want.float().to(DEV)


@pytest.fixture()
def nat():
    import ogc_amd  # noqa: F401
    from ogc_amd import _lib
    from ogc_amd.pointnet2 import pointnet2 as api
    n = api._native
    precision, det = n.get_matmul_precision(), _lib.DETERMINISTIC
    try:
        yield n
    finally:
        n.set_matmul_precision(precision)
        _lib.set_deterministic(det)


def _run(nat, form, precision, relu, det):
    """Every case of one form: dW equals the integer product."""
    from ogc_amd import _lib
    nat.set_matmul_precision(precision)
    _lib.set_deterministic(det)
    xt, yt = {"plain": (torch.float32, torch.float32), "affine": (torch.float32, torch.float32), "xf_h": (torch.float32, BF),
              "affine_h": (BF, BF), "pooled": (torch.float32, torch.float32), "pooled_h": (BF, BF)}[form]
    launched, bad = 0, []
    for cin, cout, b, hw in CASES:
        c = _inputs(cin, cout, b, hw)
        x, y, pa, pb = c["x", xt], c["y", yt], c["pa", "dev"], c["pb", "dev"]
        for s in (NSAMPLES if form.startswith("pooled") else (0,)):
            if s and hw % s:
                continue
            dw = torch.full((cout, cin), float("nan"), device=DEV)   # (the entry points zero dW themselves)
            if s:
                nat.conv1x1_wgrad_affine_pooled_wrapper(b, cin, cout, hw, relu, s, x, pa, pb, y, c["coef2"], c["inj", s], dw)
            elif form.startswith("affine"):
                nat.conv1x1_wgrad_affine_wrapper(b, cin, cout, hw, relu, x, pa, pb, y, dw)
            else:
                nat.conv1x1_wgrad_wrapper(b, cin, cout, hw, x, y, dw)
            launched += 1
            if not torch.equal(dw, _want(cin, cout, b, hw, None if form in ("plain", "xf_h") else relu, s)):
                bad.append((cin, cout, b, hw, s))
    assert launched >= len(CASES)
    assert not bad, "%s (%s operands, relu %d, deterministic %d): dW differs from the integer product at (cin, cout, b, hw, nsample) %s" % (
        form, precision, relu, det, bad)


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_plain_exact(nat, precision, det):
    _run(nat, "plain", precision, 0, det)


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_affine_exact(nat, precision, relu, det):
    _run(nat, "affine", precision, relu, det)


@pytest.mark.parametrize("det", [False, True])
def test_xf_h_exact(nat, det):
    _run(nat, "xf_h", "bf16", 0, det)


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("relu", [0, 1])
def test_affine_h_exact(nat, relu, det):
    _run(nat, "affine_h", "bf16", relu, det)


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("form,precision", [("pooled", "fp32"), ("pooled_h", "bf16")])
def test_pooled_exact(nat, form, precision, det):
    """Every nsample of 16, 32, 64 that divides hw, with the ReLU of the folded norm on."""
    _run(nat, form, precision, 1, det)

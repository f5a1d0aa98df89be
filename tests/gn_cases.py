"""Decided inputs and a float64 reference for the GroupNorm kernels (csrc/group_norm.hip), for
tests/test_group_norm_truth_gpu.py.  Host side: numpy for the inputs, torch float64 for the reference; no GPU needed, the
library is not imported.

Why "decided".  A ReLU gate or an arg-max computed in fp32 may legitimately differ from the float64 one when the value it
hangs on lies within rounding of the threshold; tests on randn inputs therefore leave such elements out.  Here the inputs are
chosen so that no element is in doubt, and everything is compared:

  * x lies on the lattice q / 8, |q| <= 255 (plus an optional common shift): exact in fp32 and in bf16 (8 significant bits);
  * in a pooled case (B, C, P, S) every neighbourhood row holds S DISTINCT lattice points, so the two largest values of
    a * x + bb differ by at least |a| / 8;
  * gamma is uniform in +-[0.5, 1.5] (fp32), negative on every fifth channel; beta[ch] is picked from a fixed grid in
    [-0.5, 0.5] AFTER the float64 statistics are known, as the candidate that maximises min |y64| over all samples and all
    lattice values present in the channel (beta does not enter the statistics; see _pick_beta for the pooled refinement);
  * with C >= 8: one channel with gamma == 0 exactly (and beta = +0.5, so that its gradient is not gated away), one with
    beta = -40 (every element gated under ReLU, every row an all-zero tie), one with beta = +40 (nothing gated);
  * `const`: one (sample, group) row holds the single value 1/8: var = 0, every neighbourhood an exact tie (arg = 0).  The
    value is a power of two so that mean * a is exact and the test is about ties, not about the cancellation in a * x + bb
    (that is the `shift` case's business).
  * grad (the incoming gradient) lies on the lattice k / 16, |k| <= 32, never zero.

make() asserts, and the unmarked tests re-check independently:
  relu cases    min |y64| >= GATE_MARGIN over ALL elements;
  pooled cases  top-1 minus top-2 of act(y64) >= GAP_MARGIN in every row that is not a tie by construction (gamma == 0,
                all-gated rows, the constant group).
A case that misses a threshold gets another seed or a finer candidate grid; the thresholds stay.
"""
import collections
import functools

import numpy as np
import torch

EPS = 1e-5
GATE_MARGIN = 5e-4
GAP_MARGIN = 2e-3
BETA_GRID = np.linspace(-0.5, 0.5, 401).astype(np.float32)
TABLE_ROWS = 1024

# kind "plain": dims = (HW,); kind "pooled": dims = (P, S).  data: "lattice" | "randn".  shift: added to every x.
# const: one (sample, group) row is the constant 1/8.  offset: the activation tensors start `offset` floats into their buffers.
Case = collections.namedtuple("Case", "kind B C dims groups relu seed data shift const offset")


def plain(B, C, HW, groups, relu, seed=0, data="lattice", shift=0.0, const=False, offset=0):
    return Case("plain", B, C, (HW,), groups, relu, seed, data, shift, const, offset)


def pooled(B, C, P, S, groups, relu, seed=0, const=False):
    return Case("pooled", B, C, (P, S), groups, relu, seed, "lattice", 0.0, const, 0)


def case_id(c):
    s = "%s-%dx%dx%s-g%d-r%d" % (c.kind, c.B, c.C, "x".join(map(str, c.dims)), c.groups, c.relu)
    return s + ("-randn" if c.data == "randn" else "") + ("-shift" if c.shift else "") + ("-const" if c.const else "") + \
        ("-off%d" % c.offset if c.offset else "")


PLAIN_CASES = [
    plain(1, 4, 7, 2, 0),                          # tiny
    plain(2, 8, 185, 4, 1),                        # hw % 4 != 0: every scalar path
    plain(2, 8, 1028, 4, 1),                       # vector path, one float4 past the first 256 threads
    plain(3, 6, 1024, 6, 1),                       # cg == 1
    plain(2, 6, 260, 1, 1),                        # one group
    plain(2, 8, 1024, 4, 1, offset=1),             # tensors 4 bytes into their buffers: scalar fallbacks at hw % 4 == 0
    plain(1, 2, 32772, 2, 1),                      # 2 statistics slots, chunk_len rounded to 16388 (vector); 8 backward slots
    plain(1, 2, 32770, 2, 1),                      # the same on the scalar statistics path
    plain(1, 4, 131072, 1, 0),                     # 32 statistics slots
    plain(1, 64, 65536, 1, 1),                     # cg * slots = 512: two rounds of the prologue's first loop
    plain(100, 4, 16384, 2, 0, data="randn"),      # nb * slots = 400: two rounds of its second loop
    plain(2, 8, 1028, 4, 1, shift=64.0),           # mean >> spread
    plain(2, 8, 260, 2, 0, const=True),            # var = 0 in one (sample, group)
    plain(2, 8, 64, 8, 1),                         # groups == C at C = 8, with the special channels
]

POOLED_CASES = [pooled(2, 8, P, S, 4, relu) for (P, S) in ((257, 4), (129, 8), (65, 16), (33, 32), (17, 64), (9, 128), (5, 256))
                for relu in (0, 1)]
POOLED_CASES += [
    pooled(2, 8, 1, 64, 2, 1), pooled(2, 8, 63, 16, 8, 1), pooled(2, 8, 1, 64, 1, 0), pooled(2, 8, 63, 16, 1, 0),
    pooled(2, 1024, 300, 4, 4, 1), pooled(64, 32, 300, 4, 4, 0),     # a strided row loop with a ragged tail
    pooled(2, 1024, 300, 16, 4, 1), pooled(64, 32, 300, 16, 4, 0),   # the same where bx is halved (5 -> 3)
    pooled(1, 8, 1025, 4, 4, 1),                                     # 2 backward slots
    pooled(1, 8, 8200, 4, 2, 1),                                     # 9 -> 8 slots, the sums kernel strides
    pooled(2, 512, 4100, 4, 4, 1),                                   # the sparse kernel's bx 5 -> 3
    pooled(2, 8, 33, 32, 4, 0, const=True),                          # all ties in one (sample, group)
]

STATS_SLOTS = (1, 3, 8, 9, 32)
STATS_PLAIN = plain(2, 8, 185, 4, 1)
STATS_POOLED = pooled(2, 8, 65, 16, 4, 1)

ALL_CASES = PLAIN_CASES + POOLED_CASES


def special_channels(C):
    """(gamma == 0, beta == -40, beta == +40) channels, or () below 8 channels; the last has a negative gamma."""
    return (1, 2, 4) if C >= 8 else ()


def const_row(c):
    """(sample, group) of the constant row."""
    return (c.B - 1, min(1, c.groups - 1))


def _x(c, rng):
    n = int(np.prod(c.dims))
    if c.data == "randn":
        return (rng.standard_normal((c.B, c.C, n)) * 2 + 0.7).astype(np.float32).reshape((c.B, c.C) + c.dims)
    if c.kind == "pooled":
        P, S = c.dims
        table = np.stack([rng.permutation(511)[:S] - 255 for _ in range(TABLE_ROWS)]).astype(np.int32)
        q = table[rng.integers(0, TABLE_ROWS, (c.B, c.C, P))]
    else:
        q = rng.integers(-255, 256, (c.B, c.C) + c.dims).astype(np.int32)
    x = q.astype(np.float32) / np.float32(8) + np.float32(c.shift)
    if c.const:
        b, g = const_row(c)
        cg = c.C // c.groups
        x[b, g * cg:(g + 1) * cg] = np.float32(0.125)
    return x


def _stats(c, x):
    """float64 mean, rstd (B, groups)."""
    r = x.astype(np.float64).reshape(c.B, c.groups, -1)
    mean = r.mean(axis=2)
    var = ((r - mean[:, :, None]) ** 2).mean(axis=2)
    return mean, 1.0 / np.sqrt(var + EPS)


def _presence(c, q):
    """(B, C, 511) bool: which lattice values occur among q (B, C, ...) (integers in [-255, 255])."""
    q = q.reshape(c.B * c.C, -1) + 255
    n = np.bincount((q + np.arange(c.B * c.C)[:, None] * 511).ravel(), minlength=c.B * c.C * 511)
    return n.reshape(c.B, c.C, 511) > 0


def _pick_beta(c, x, gamma, mean, rstd, rng):
    """beta[ch]: the grid candidate that maximises the smallest margin, in units of its threshold, over samples b and lattice
    values v present in (b, ch):  |a * (v - mean) + beta| / GATE_MARGIN — and, in a pooled ReLU case, / GAP_MARGIN for the
    values that are the extreme of some neighbourhood (its maximum where gamma >= 0, its minimum where gamma < 0): when every
    other element of the row is gated, the row's gap is that value itself.  The last of equally good candidates."""
    cg = c.C // c.groups
    if c.data == "randn" or not c.relu:      # nothing is gated: any beta will do
        return BETA_GRID[rng.integers(0, len(BETA_GRID), c.C)].copy()
    q = np.rint((x.astype(np.float64) - c.shift) * 8).astype(np.int64)
    weight = np.where(_presence(c, q), 1.0 / GATE_MARGIN, 0.0)
    if c.kind == "pooled" and c.relu:
        ext = np.where((gamma >= 0)[None, :, None], q.max(axis=3), q.min(axis=3))
        weight = np.where(_presence(c, ext), 1.0 / GAP_MARGIN, weight)
    values = (np.arange(511) - 255) / 8.0 + c.shift
    beta = np.empty(c.C, np.float32)
    cand = BETA_GRID.astype(np.float64)
    for ch in range(c.C):
        g = ch // cg
        y0 = (values[None, :] - mean[:, g, None]) * (rstd[:, g, None] * float(gamma[ch]))     # (B, 511)
        keep = weight[:, ch] > 0
        m = (np.abs(y0[keep][None, :] + cand[:, None]) * weight[:, ch][keep][None, :]).min(axis=1)
        beta[ch] = BETA_GRID[np.flatnonzero(m == m.max())[-1]]
    return beta


@functools.lru_cache(maxsize=2)
def make(c):
    """dict: x (B, C, *dims), gamma, beta (C), grad (B, C, HW) or (B, C, P) — fp32 numpy — and the margins
    gate (min |y64|) and gap (smallest top-1 minus top-2 of act(y64) outside the ties by construction; inf if not pooled)."""
    rng = np.random.default_rng([c.seed, c.B, c.C, c.groups, c.relu] + list(c.dims))
    x = _x(c, rng)
    gamma = rng.uniform(0.5, 1.5, c.C).astype(np.float32)
    gamma[4::5] *= np.float32(-1)
    sp = special_channels(c.C)
    if sp:
        gamma[sp[0]] = 0.0
    mean, rstd = _stats(c, x)
    beta = _pick_beta(c, x, gamma, mean, rstd, rng)
    if sp:
        beta[sp[1]], beta[sp[2]] = -40.0, 40.0
    gshape = (c.B, c.C) + (c.dims if c.kind == "plain" else c.dims[:1])
    k = rng.integers(1, 33, gshape) * rng.choice([-1, 1], gshape)
    grad = (k / 16.0).astype(np.float32)
    d = {"x": x, "gamma": gamma, "beta": beta, "grad": grad}
    d["gate"], d["gap"] = margins(c, d)
    if c.relu and c.data == "lattice":
        assert d["gate"] >= GATE_MARGIN, (case_id(c), d["gate"])
    if c.kind == "pooled":
        assert d["gap"] >= GAP_MARGIN, (case_id(c), d["gap"])
    return d


def tie_rows(c, d, y):
    """(B, C, P) bool: rows of a pooled case whose maximum is a tie by construction."""
    tie = np.zeros(y.shape[:3], bool)
    tie[:, d["gamma"] == 0] = True
    if c.relu:
        tie |= (y <= 0).all(axis=3)
    if c.const:
        b, g = const_row(c)
        cg = c.C // c.groups
        tie[b, g * cg:(g + 1) * cg] = True
    return tie


def margins(c, d):
    """(min |y64| over all elements, smallest top-1 minus top-2 of act(y64) over the rows that are no tie by construction)."""
    cg = c.C // c.groups
    mean, rstd = _stats(c, d["x"])
    a = np.repeat(rstd, cg, axis=1) * d["gamma"].astype(np.float64)[None, :]            # (B, C)
    ex = (slice(None), slice(None)) + (None,) * len(c.dims)
    y = (d["x"].astype(np.float64) - np.repeat(mean, cg, axis=1)[ex]) * a[ex] + d["beta"].astype(np.float64)[None, :][ex]
    gate = float(np.abs(y).min())
    if c.kind != "pooled":
        return gate, float("inf")
    tie = tie_rows(c, d, y)
    act = np.maximum(y, 0.0) if c.relu else y
    top = np.partition(act, act.shape[3] - 2, axis=3)[..., -2:]
    gaps = (top[..., 1] - top[..., 0])[~tie]
    return gate, float(gaps.min()) if gaps.size else float("inf")


def host_partials(c, x, slots):
    """float64 (sum, sum of squares) of `slots` slices of every (b, group) row of x, layout [slot][b * groups][2] — what a
    producing convolution hands to the *_stats entry points.  The slices are uneven on purpose."""
    r = x.astype(np.float64).reshape(c.B * c.groups, -1)
    n = r.shape[1]
    k = np.arange(1, slots)
    edges = np.unique(np.concatenate([[0, n], (k * n // slots + k % 3).clip(0, n)]))   # (a slot left over stays zero)
    out = np.zeros((slots, c.B * c.groups, 2))
    for s in range(len(edges) - 1):
        piece = r[:, edges[s]:edges[s + 1]]
        out[s, :, 0] = piece.sum(axis=1)
        out[s, :, 1] = (piece * piece).sum(axis=1)
    return out


def reference(c, d, device="cpu"):
    """The float64 truth, by torch on `device`:  y = (x - mean) * rstd * gamma + beta  (biased variance, EPS), optional ReLU;
    pooled: arg = first maximum of act(y) over the neighbourhood, out = act(y) at arg; gradients of sum(result * grad) by autograd
    through exactly that expression (a tie routes to the first index).  Also mean, rstd (B, groups), a = rstd * gamma,
    bb = beta - mean * a (B, C), and c2, c3 (B, groups) with  dx = a * dy' + c2 * x + c3  (dy' the gated — and, pooled,
    scattered — incoming gradient)."""
    B, C, G = c.B, c.C, c.groups
    cg = C // G
    x = torch.from_numpy(d["x"]).to(device).double().requires_grad_(True)
    gamma = torch.from_numpy(d["gamma"]).to(device).double().requires_grad_(True)
    beta = torch.from_numpy(d["beta"]).to(device).double().requires_grad_(True)
    grad = torch.from_numpy(d["grad"]).to(device).double()
    r = x.reshape(B, G, -1)
    mean = r.mean(dim=2, keepdim=True)
    var = ((r - mean) ** 2).mean(dim=2, keepdim=True)
    rstd = (var + EPS).rsqrt()
    xhat = ((r - mean) * rstd).reshape(B, C, -1)
    y = (xhat * gamma[None, :, None] + beta[None, :, None]).reshape(x.shape)
    act = torch.relu(y) if c.relu else y
    out = {}
    if c.kind == "pooled":
        top = act.detach().max(dim=3, keepdim=True)[0]           # the FIRST maximum, spelled out (torch.argmax semantics)
        pos = torch.arange(act.shape[3], device=act.device).expand_as(act)
        arg = torch.where(act.detach() == top, pos, act.shape[3]).min(dim=3)[0]
        res = act.gather(3, arg.unsqueeze(3)).squeeze(3)
        out["arg"] = arg.to(torch.int32)
    else:
        res = act
    gx, gg, gb = torch.autograd.grad((res * grad).sum(), [x, gamma, beta])
    mean, rstd = mean.detach().reshape(B, G), rstd.detach().reshape(B, G)
    a = rstd.repeat_interleave(cg, dim=1) * gamma.detach()[None, :]
    bb = beta.detach()[None, :] - mean.repeat_interleave(cg, dim=1) * a
    # c2, c3 from the sums, validated against the autograd gradient
    xd = x.detach()
    if c.kind == "pooled":
        gated = grad * (res.detach() > 0) if c.relu else grad
        dyp = torch.zeros_like(xd).scatter_(3, arg.unsqueeze(3), gated.unsqueeze(3))
    else:
        dyp = grad * (y.detach() > 0) if c.relu else grad
    gk = gamma.detach()[None, :, None]
    ds = (dyp * xd).reshape(B, C, -1).mul(gk).reshape(B, G, -1).sum(dim=2)
    db = dyp.reshape(B, C, -1).mul(gk).reshape(B, G, -1).sum(dim=2)
    n = cg * int(np.prod(c.dims))
    c2 = (db * mean - ds) * rstd ** 3 / n
    c3 = -c2 * mean - db * rstd / n
    ex = (slice(None), slice(None)) + (None,) * len(c.dims)
    rebuilt = a[ex] * dyp + c2.repeat_interleave(cg, dim=1)[ex] * xd + c3.repeat_interleave(cg, dim=1)[ex]
    assert float((rebuilt - gx).abs().max()) <= 1e-9 * max(1.0, float(gx.abs().max())), "c2 / c3 do not reproduce autograd"
    out.update(y=res.detach(), mean=mean, rstd=rstd, a=a, bb=bb, dx=gx, dgamma=gg, dbeta=gb, c2=c2, c3=c3, dyp=dyp)
    return out

"""Decided inputs and a float64 reference for the BatchNorm kernels (csrc/batch_norm.hip), for
tests/test_batch_norm_truth_gpu.py.  Host side: numpy for the inputs, torch float64 for the reference; no GPU needed, the
library is not imported.  The twin of tests/gn_cases.py (read its docstring for why "decided"), with the statistics taken per
channel over (B, HW):

  * x lies on the lattice q / 8, |q| <= 255 (plus an optional common shift of 64): exact in fp32, and so are the sums of x and
    x * x in fp32 groups of four and in fp64, in any order;
  * in a pooled case (B, C, P, S) every neighbourhood row holds S DISTINCT lattice points;
  * gamma is uniform in +-[0.5, 1.5] (fp32), negative on every fifth channel; beta[ch] is picked from a fixed grid in
    [-0.5, 0.5] AFTER the float64 statistics are known, as the candidate that maximises min |y64| over the lattice values
    present in the channel — in training mode and, for a case that is also run in evaluation mode (`ev`), under the running
    statistics as well;
  * with C >= 8: one channel with gamma == 0 exactly (its beta comes out as +0.5: not gated), one with beta = -40 (in training
    mode every element gated under ReLU, every row an all-zero tie), one with beta = +40 (nothing gated);
  * `const`: channel CONST_CHANNEL holds the single value 1/8 in every sample: var = 0, every neighbourhood an exact tie;
  * grad (the incoming gradient) lies on the lattice k / 16, |k| <= 32, never zero;
  * the running buffers on entry: running_mean = 0.1 * randn, running_var uniform in [0.5, 1.5]; momentum 0.3.

make() asserts, and the unmarked tests re-check independently with torch.nn.functional.batch_norm in float64:
  relu cases    min |y64| >= GATE_MARGIN over ALL elements (in evaluation mode too where the case is run there);
  pooled cases  top-1 minus top-2 of act(y64) >= GAP_MARGIN in every row that is not a tie by construction (gamma == 0,
                all-gated rows, the constant channel).
A case that misses a threshold gets another seed or a finer candidate grid; the thresholds stay, and no element is left out.

Out of scope: count == 1 (B * HW == 1, where torch itself refuses to train), non-finite inputs, and — for the one `randn`
case, whose only business is the 32-chunk grid — everything except the truth / yardstick comparison.
"""
import collections
import functools

import numpy as np
import torch

from gn_cases import GAP_MARGIN, GATE_MARGIN, TABLE_ROWS

EPS = 1e-5
MOMENTUM = 0.3
BETA_GRID = np.linspace(-0.5, 0.5, 401).astype(np.float32)
CONST_CHANNEL = 3

# kind "plain": dims = (HW,); kind "pooled": dims = (P, S).  data: "lattice" | "randn".  shift: added to every x.
# const: channel CONST_CHANNEL is the constant 1/8.  misalign: "" | "all" (x, grad, y, dx start one float into their buffers)
# | "out" (only y and dx do).  running: the running buffers are passed (else None).  ev: also run in evaluation mode.
Case = collections.namedtuple("Case", "kind B C dims relu seed data shift const misalign running ev")


def plain(B, C, HW, relu, seed=0, data="lattice", shift=0.0, const=False, misalign="", running=True, ev=False):
    return Case("plain", B, C, (HW,), relu, seed, data, shift, const, misalign, running, ev)


def pooled(B, C, P, S, relu, seed=0, const=False, ev=False):
    return Case("pooled", B, C, (P, S), relu, seed, "lattice", 0.0, const, "", True, ev)


def case_id(c):
    s = "%s-%dx%dx%s-r%d" % (c.kind, c.B, c.C, "x".join(map(str, c.dims)), c.relu)
    return s + ("-randn" if c.data == "randn" else "") + ("-shift" if c.shift else "") + ("-const" if c.const else "") + \
        ("-mis_" + c.misalign if c.misalign else "") + ("" if c.running else "-norun") + ("-ev" if c.ev else "")


# bn_chunks(b, c, hw): chunks doubles while b * c * chunks < 2048 and hw / (2 * chunks) >= 4096
PLAIN_CASES = [
    plain(2, 4, 7, 1),                                  # tiny
    plain(2, 8, 185, 1, ev=True),                       # hw % 4 != 0: every scalar path
    plain(2, 8, 1028, 1, ev=True),                      # vector path, one float4 past the first 256 threads
    plain(2, 8, 1024, 1, misalign="all"),               # tensors 4 bytes into their buffers: scalar fallbacks at hw % 4 == 0
    plain(2, 8, 1024, 1, misalign="out"),               # only y / dx misaligned: the OR-ed alignment test
    plain(1, 2, 8192, 1, ev=True),                      # chunks = 2
    plain(1, 2, 8194, 1),                               # chunks = 2 on the scalar paths
    plain(2, 2, 8192, 1),                               # chunks = 2, two samples: grid x and z both count in the slab index
    plain(1, 1, 65536, 1),                              # chunks = 16
    plain(1, 64, 131072, 0, data="randn"),              # chunks = 32 (b * c * 32 reaches 2048)
    plain(3, 8, 260, 0),                                # relu = 0
    plain(2, 8, 1028, 1, shift=64.0),                   # mean >> spread
    plain(2, 8, 260, 1, const=True),                    # var = 0 in one channel
    plain(2, 8, 260, 1, running=False),                 # training without running buffers
]

# rows_per_block = 256 / (S / 4); bx = ceil(P / rows_per_block), halved while bx * C * B > 8192; the backward sums' bs =
# ceil(P / 256), halved while bs * C * B > 4096
POOLED_CASES = [pooled(2, 8, P, S, relu, ev=(relu == 1 and S in (4, 256)))      # every L = S / 4, two workgroups, the last ragged
                for (P, S) in ((257, 4), (129, 8), (65, 16), (33, 32), (17, 64), (9, 128), (5, 256)) for relu in (0, 1)]
POOLED_CASES += [
    pooled(2, 8, 1, 64, 1),                             # P = 1
    pooled(2, 1024, 300, 16, 1),                        # bx 5 -> 3: a strided row loop with clamped tail rows
    pooled(2, 1024, 520, 4, 1),                         # the backward sums' bs 3 -> 2 (bx stays 3)
    pooled(2, 8, 33, 32, 0, const=True),                # a whole channel of exact ties, arg = 0
]

STATS_SLOTS = (1, 3, 32)
STATS_PLAIN = plain(2, 8, 185, 1, ev=True)
STATS_POOLED = pooled(2, 8, 65, 16, 1)
DET_PLAIN = plain(2, 2, 8192, 1)
DET_POOLED = pooled(2, 1024, 300, 16, 1)

ALL_CASES = PLAIN_CASES + POOLED_CASES
EVAL_CASES = [c for c in ALL_CASES if c.ev]


def special_channels(C):
    """(gamma == 0, beta == -40, beta == +40) channels, or () below 8 channels; the last has a negative gamma."""
    return (1, 2, 4) if C >= 8 else ()


def _x(c, rng):
    n = int(np.prod(c.dims))
    if c.data == "randn":
        return (rng.standard_normal((c.B, c.C, n), dtype=np.float32) * 2 + np.float32(0.7)).reshape((c.B, c.C) + c.dims)
    if c.kind == "pooled":
        P, S = c.dims
        table = np.stack([rng.permutation(511)[:S] - 255 for _ in range(TABLE_ROWS)]).astype(np.int32)
        q = table[rng.integers(0, TABLE_ROWS, (c.B, c.C, P))]
    else:
        q = rng.integers(-255, 256, (c.B, c.C) + c.dims).astype(np.int32)
    x = q.astype(np.float32) / np.float32(8) + np.float32(c.shift)
    if c.const:
        x[:, CONST_CHANNEL] = np.float32(0.125)
    return x


def _stats(c, x):
    """float64 mean, biased variance per channel."""
    r = np.moveaxis(x.astype(np.float64).reshape(c.B, c.C, -1), 1, 0).reshape(c.C, -1)
    mean = r.mean(axis=1)
    return mean, ((r - mean[:, None]) ** 2).mean(axis=1)


def _maps(c, d):
    """[(mean, a)] float64 per channel of the modes the case is run in: y = a * (x - mean) + beta."""
    g = d["gamma"].astype(np.float64)
    mean, var = _stats(c, d["x"])
    maps = [(mean, g / np.sqrt(var + EPS))]
    if c.ev:
        maps.append((d["running_mean"].astype(np.float64), g / np.sqrt(d["running_var"].astype(np.float64) + EPS)))
    return maps


def _presence(c, q):
    """(C, 511) bool: which lattice values occur in each channel of q (B, C, ...) (integers in [-255, 255])."""
    q = np.moveaxis(q.reshape(c.B, c.C, -1), 1, 0).reshape(c.C, -1) + 255
    n = np.bincount((q + np.arange(c.C)[:, None] * 511).ravel(), minlength=c.C * 511)
    return n.reshape(c.C, 511) > 0


def _pick_beta(c, d, rng):
    """beta[ch]: the grid candidate that maximises the smallest margin, in units of its threshold, over the lattice values v
    present in the channel and the modes the case is run in:  |a * (v - mean) + beta| / GATE_MARGIN — and, in a pooled ReLU
    case, / GAP_MARGIN for the values that are the extreme of some neighbourhood (its maximum where gamma >= 0, its minimum
    where gamma < 0): when every other element of the row is gated, the row's gap is that value itself.  The last of equally
    good candidates."""
    x, gamma = d["x"], d["gamma"]
    if c.data == "randn" or not c.relu:      # nothing is gated: any beta will do
        return BETA_GRID[rng.integers(0, len(BETA_GRID), c.C)].copy()
    q = np.rint((x.astype(np.float64) - c.shift) * 8).astype(np.int64)
    weight = np.where(_presence(c, q), 1.0 / GATE_MARGIN, 0.0)
    if c.kind == "pooled":
        ext = np.where((gamma >= 0)[None, :, None], q.max(axis=3), q.min(axis=3))
        weight = np.where(_presence(c, ext), 1.0 / GAP_MARGIN, weight)
    values = (np.arange(511) - 255) / 8.0 + c.shift
    beta = np.empty(c.C, np.float32)
    cand = BETA_GRID.astype(np.float64)
    maps = _maps(c, d)
    for ch in range(c.C):
        keep = weight[ch] > 0
        m = np.full(len(cand), np.inf)
        for mean, a in maps:
            y0 = (values[keep] - mean[ch]) * a[ch]
            m = np.minimum(m, (np.abs(y0[None, :] + cand[:, None]) * weight[ch][keep][None, :]).min(axis=1))
        beta[ch] = BETA_GRID[np.flatnonzero(m == m.max())[-1]]
    return beta


@functools.lru_cache(maxsize=2)
def make(c):
    """dict: x (B, C, *dims), gamma, beta, running_mean, running_var (C), grad (B, C, HW) or (B, C, P) — fp32 numpy — and the
    margins gate (min |y64|) and gap (smallest top-1 minus top-2 of act(y64) outside the ties by construction; inf if not
    pooled), the smaller of training and evaluation mode where the case runs in both."""
    rng = np.random.default_rng([c.seed, c.B, c.C, c.relu, 77] + list(c.dims))
    d = {"x": _x(c, rng)}
    gamma = rng.uniform(0.5, 1.5, c.C).astype(np.float32)
    gamma[4::5] *= np.float32(-1)
    sp = special_channels(c.C)
    if sp:
        gamma[sp[0]] = 0.0
    d["gamma"] = gamma
    d["running_mean"] = (rng.standard_normal(c.C) * 0.1).astype(np.float32)
    d["running_var"] = rng.uniform(0.5, 1.5, c.C).astype(np.float32)
    d["beta"] = _pick_beta(c, d, rng)
    if sp:
        d["beta"][sp[1]], d["beta"][sp[2]] = -40.0, 40.0
    gshape = (c.B, c.C) + (c.dims if c.kind == "plain" else c.dims[:1])
    k = rng.integers(1, 33, gshape) * rng.choice([-1, 1], gshape)
    d["grad"] = (k / 16.0).astype(np.float32)
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
        tie[:, CONST_CHANNEL] = True
    return tie


def margins(c, d):
    """(min |y64| over all elements, smallest top-1 minus top-2 of act(y64) over the rows that are no tie by construction),
    over the modes the case is run in."""
    gate, gap = float("inf"), float("inf")
    ex = (None, slice(None)) + (None,) * len(c.dims)
    for mean, a in _maps(c, d):
        y = (d["x"].astype(np.float64) - mean[ex]) * a[ex] + d["beta"].astype(np.float64)[ex]
        gate = min(gate, float(np.abs(y).min()))
        if c.kind != "pooled":
            continue
        tie = tie_rows(c, d, y)
        act = np.maximum(y, 0.0) if c.relu else y
        top = np.partition(act, act.shape[3] - 2, axis=3)[..., -2:]
        gaps = (top[..., 1] - top[..., 0])[~tie]
        if gaps.size:
            gap = min(gap, float(gaps.min()))
    return gate, gap


def host_partials(c, x, slots):
    """float64 (sum, sum of squares) of `slots` slices of every channel of x, layout [slot][channel][2] — what a producing
    convolution hands to the `stats` argument of the forward entry points.  The slices are uneven on purpose."""
    r = np.moveaxis(x.astype(np.float64).reshape(c.B, c.C, -1), 1, 0).reshape(c.C, -1)
    n = r.shape[1]
    k = np.arange(1, slots)
    edges = np.unique(np.concatenate([[0, n], (k * n // slots + k % 3).clip(0, n)]))   # (a slot left over stays zero)
    out = np.zeros((slots, c.C, 2))
    for s in range(len(edges) - 1):
        piece = r[:, edges[s]:edges[s + 1]]
        out[s, :, 0] = piece.sum(axis=1)
        out[s, :, 1] = (piece * piece).sum(axis=1)
    return out


def first_max(act):
    """Index of the FIRST maximum along the last dimension (torch.argmax semantics, spelled out)."""
    m = act.max(dim=-1, keepdim=True)[0]
    pos = torch.arange(act.shape[-1], device=act.device).expand_as(act)
    return torch.where(act == m, pos, act.shape[-1]).min(dim=-1)[0]


def reference(c, d, training=True, device="cpu"):
    """The float64 truth, by torch on `device`, written out (no batch_norm operator):
        training    mean, var (biased) per channel over (B, HW);  evaluation  mean, var = the running buffers
        rstd = 1 / sqrt(var + EPS),  y = (x - mean) * rstd * gamma + beta,  optional ReLU
        pooled      arg = first maximum of act(y) over the neighbourhood, out = act(y) at arg
        dy'         the incoming gradient, gated by y > 0 under ReLU — and, pooled, scattered to arg
        dbeta = sum dy',  dgamma = sum dy' * (x - mean) * rstd
        dx = gamma * rstd * (dy' - [training] (dbeta + xhat * dgamma) / n)
        running_mean / running_var after the call: updated with MOMENTUM and the UNBIASED variance in training mode when the
        case passes the buffers, else as they were.
    Keys: y, arg (pooled), mean, rstd, running_mean, running_var, dx, dgamma, dbeta, dyp.  test_reference_is_torch_batch_norm
    holds this against torch's float64 batch_norm and its autograd."""
    B, C = c.B, c.C
    n = B * int(np.prod(c.dims))
    col = (None, slice(None), None)
    t = lambda a: torch.from_numpy(a).to(device).double()  # noqa: E731
    x, gamma, beta, grad = t(d["x"]).reshape(B, C, -1), t(d["gamma"]), t(d["beta"]), t(d["grad"])
    rm, rv = t(d["running_mean"]), t(d["running_var"])
    if training:
        mean = x.mean(dim=(0, 2))
        var = ((x - mean[col]) ** 2).mean(dim=(0, 2))
    else:
        mean, var = rm, rv
    rstd = (var + EPS).rsqrt()
    xhat = (x - mean[col]) * rstd[col]
    y = xhat * gamma[col] + beta[col]
    act = torch.relu(y) if c.relu else y
    out = {}
    if c.kind == "pooled":
        P, S = c.dims
        act = act.reshape(B, C, P, S)
        arg = first_max(act)
        res = act.gather(3, arg.unsqueeze(3)).squeeze(3)
        gated = grad * (res > 0) if c.relu else grad
        dyp = torch.zeros_like(act).scatter_(3, arg.unsqueeze(3), gated.unsqueeze(3)).reshape(B, C, -1)
        out["arg"] = arg.to(torch.int32)
    else:
        res = act
        dyp = grad * (y > 0) if c.relu else grad
    del act, y
    db = dyp.sum(dim=(0, 2))
    dg = (dyp * xhat).sum(dim=(0, 2))
    dx = dyp.clone()
    if training:
        dx -= (db[col] + xhat * dg[col]) / n
    dx *= (gamma * rstd)[col]
    if training and c.running:
        rm = (1 - MOMENTUM) * rm + MOMENTUM * mean
        rv = (1 - MOMENTUM) * rv + MOMENTUM * var * (n / (n - 1.0))
    shape = (B, C) + c.dims
    out.update(y=res.reshape(shape if c.kind == "plain" else shape[:3]), mean=mean, rstd=rstd, running_mean=rm, running_var=rv,
               dx=dx.reshape(shape), dgamma=dg, dbeta=db, dyp=dyp.reshape(shape))
    return out

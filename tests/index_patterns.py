"""Adversarial neighbour-index tensors and exact integer references for tests/test_index_patterns_gpu.py (host only, numpy).

Two families of generators:

  * pattern / patterns        (B, P, S) int32 tensors into n points — the grouping tensors of the set-abstraction and
                              feature-propagation layers; flattened T = P * S, t = p * S + s;
  * nb_pattern / nb_patterns  (B, N, k) int32 neighbour lists of a cloud in itself — the smoothness loss.

Every tensor has B = 2 and its second sample carries a DIFFERENT pattern (PARTNER / NB_PARTNER), so that an error in a
per-sample offset cannot cancel.

Exact sums: the values handed to the kernels are small integers or dyadic fractions, all multiples of one power of two
(`unit`).  While sum |term| / unit < 2**24 holds for an output element, every partial sum of its terms, in any order and any
grouping, is an integer multiple of the unit below 2**24 units and therefore exactly representable in fp32: the kernel must
EQUAL the int64 reference.  scatter_units checks that precondition for every output element before it returns.
"""
import functools

import numpy as np

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
EXACT_LIMIT = 2 ** 24

NAMES = ("hub", "two_hubs", "cyclic", "sorted", "ball_rows", "straddle", "stray")
# the pattern of the second sample
PARTNER = {"hub": "sorted", "two_hubs": "cyclic", "cyclic": "ball_rows", "sorted": "straddle", "ball_rows": "cyclic",
           "straddle": "ball_rows", "stray": "stray_straddle"}

NB_NAMES = ("self_only", "first_copies", "self_first", "hub", "ball_rows", "cyclic")
NB_PARTNER = {"self_only": "first_copies", "first_copies": "self_first", "self_first": "hub", "hub": "ball_rows",
              "ball_rows": "cyclic", "cyclic": "self_only"}


# ---- (P, S) grouping tensors --------------------------------------------------------------------------------------------------
def _hub(P, S, n, rng):
    return np.full(P * S, n - 1, np.int64)


def _two_hubs(P, S, n, rng):
    if n == 1:
        return _hub(P, S, n, rng)
    return np.where(np.arange(P * S) % 2 == 0, n - 1, 0).astype(np.int64)


def _cyclic(P, S, n, rng):
    return np.arange(P * S, dtype=np.int64) % n


def _sorted(P, S, n, rng):
    T = P * S
    return np.arange(T, dtype=np.int64) * n // T


def ball_keep(P, S, rng):
    """Entries kept per row: every value 1 .. S occurs (when P >= S), in a random row order."""
    return rng.permutation(np.arange(P) % S + 1)


def _ball_rows(P, S, n, rng):
    rows = rng.integers(0, n, (P, S))
    keep = ball_keep(P, S, rng)
    return np.where(np.arange(S)[None, :] < keep[:, None], rows, rows[:, :1]).reshape(-1)


def _straddle(P, S, n, rng):
    """Random filler with runs of 17 .. 40 equal indices laid from positions = 15 (mod 16): every run crosses at least one
    aligned group of 16.  Above one chunk of 8192 positions one run covers 8185 .. 8200 (the chunk boundary, inside a group
    on either side)."""
    T = P * S
    idx = rng.integers(0, n, T)
    value = int(rng.integers(0, n))

    def another():
        nonlocal value
        value = (value + 1 + int(rng.integers(0, max(n - 1, 1)))) % n
        return value

    def lay(lo, hi):                  # a run over [lo, hi) that the filler on either side does not extend
        idx[lo:hi] = another()
        idx[lo - 1] = (value + 1) % n
        if hi < T:
            idx[hi] = (value + 1) % n

    reserved = (8176, 8208) if T > 8192 else (0, 0)
    pos = 15
    while True:
        length = int(rng.integers(17, 41))
        if pos + length > T:
            break
        if pos + length < reserved[0] or pos > reserved[1]:
            lay(pos, pos + length)
        pos = (pos + length) // 16 * 16 + 16 + 15      # at least 16 positions of filler between two runs
    if T > 8192:
        lay(8185, min(8201, T))
    return idx


def _stray_of(base):
    def gen(P, S, n, rng):
        idx = base(P, S, n, rng)
        bad = np.array([-1, n, n + 7, INT32_MIN, INT32_MAX], np.int64)
        hit = rng.random(idx.shape[0]) < 0.05
        return np.where(hit, bad[rng.integers(0, bad.shape[0], idx.shape[0])], idx)
    return gen


_GEN = {"hub": _hub, "two_hubs": _two_hubs, "cyclic": _cyclic, "sorted": _sorted, "ball_rows": _ball_rows,
        "straddle": _straddle, "stray": _stray_of(_ball_rows), "stray_straddle": _stray_of(_straddle)}


def pattern(name, B, P, S, n, rng):
    """The (B, P, S) int32 tensor of pattern `name`: sample 0 carries the pattern, every further sample PARTNER[name]."""
    rows = [_GEN[name if b == 0 else PARTNER[name]](P, S, n, rng) for b in range(B)]
    return np.stack(rows).reshape(B, P, S).astype(np.int32)


def patterns(B, P, S, n, rng):
    """Yields (name, idx (B, P, S) int32) for every pattern of NAMES ('stray' last: out-of-range entries)."""
    for name in NAMES:
        yield name, pattern(name, B, P, S, n, rng)


# ---- (N, k) neighbour lists of a cloud in itself ------------------------------------------------------------------------------
def _nb_self_only(N, k, rng):
    return np.repeat(np.arange(N)[:, None], k, 1)


def _nb_first_copies(N, k, rng):
    return np.repeat(((np.arange(N) + 1) % N)[:, None], k, 1)


def _nb_self_first(N, k, rng):
    idx = rng.integers(0, N, (N, k))
    me = np.arange(N)[:, None]
    idx = np.where(rng.random((N, k)) < 0.25, me, idx)      # later copies of the point itself
    idx[:, 0] = me[:, 0]
    return idx


def _nb_hub(N, k, rng):
    return np.zeros((N, k), np.int64)


def _nb_ball_rows(N, k, rng):
    return _ball_rows(N, k, N, rng).reshape(N, k)


def _nb_cyclic(N, k, rng):
    return (np.arange(N * k, dtype=np.int64) % N).reshape(N, k)


_NB_GEN = {"self_only": _nb_self_only, "first_copies": _nb_first_copies, "self_first": _nb_self_first, "hub": _nb_hub,
           "ball_rows": _nb_ball_rows, "cyclic": _nb_cyclic}


def nb_pattern(name, B, N, k, rng):
    rows = [_NB_GEN[name if b == 0 else NB_PARTNER[name]](N, k, rng) for b in range(B)]
    return np.stack(rows).astype(np.int32)


def nb_patterns(B, N, k, rng):
    for name in NB_NAMES:
        yield name, nb_pattern(name, B, N, k, rng)


# ---- host definitions of what the list builders must produce ------------------------------------------------------------------
def run_heads(flat):
    """(B, T) bool: the positions ogc_group_reverse keeps — the first of every run of equal indices inside an aligned group
    of 16 positions (raw values: a run of one out-of-range value is a run too)."""
    head = np.ones(flat.shape, bool)
    head[:, 1:] = flat[:, 1:] != flat[:, :-1]
    head[:, ::16] = True
    return head


def list_lengths(flat, n, heads_only=False):
    """(B, n) entries per point: all in-range positions, or only the run heads among them (what the gather form walks)."""
    out = np.zeros((flat.shape[0], n), np.int64)
    ok = (flat >= 0) & (flat < n)
    if heads_only:
        ok &= run_heads(flat)
    for b in range(flat.shape[0]):
        out[b] = np.bincount(flat[b][ok[b]], minlength=n)
    return out


def nb_edges(idx):
    """The transposed lists ogc_reverse_neighbours must hold for idx (N, k): (sorted int64 keys of the (destination, source,
    first-flag) edges, rev_mult (N,)).  Self edges are dropped; the copies of a row's first entry are merged into that first
    edge, whose weight is the row's multiplicity."""
    N, k = idx.shape
    idx = idx.astype(np.int64)
    me = np.arange(N)[:, None]
    first = idx[:, :1]
    col = np.arange(k)[None, :]
    dup = (col > 0) & (idx == first)
    keep = (idx != me) & ~dup
    mult = np.where(first[:, 0] == me[:, 0], 1, (idx == first).sum(1))
    keys = edge_keys(idx[keep], np.broadcast_to(me, idx.shape)[keep], np.broadcast_to(col == 0, idx.shape)[keep], N)
    return np.sort(keys), mult


def edge_keys(dst, src, first, N):
    return (dst.astype(np.int64) * N + src.astype(np.int64)) * 2 + first.astype(np.int64)


# ---- exact references -----------------------------------------------------------------------------------------------------------
def scatter_units(idx, terms, n, what=""):
    """out[b, c, idx[b, t]] += terms[b, c, t] in int64 (np.add.at), entries outside [0, n) skipped.  idx (B, T), terms (B, C, T)
    integers (multiples of the unit).  Asserts the exactness precondition sum |term| < 2**24 units for every output element."""
    B, C, T = terms.shape
    terms = terms.astype(np.int64)
    out = np.zeros((B, C, n), np.int64)
    mass = np.zeros((B, C, n), np.int64)
    for b in range(B):
        ok = (idx[b] >= 0) & (idx[b] < n)
        j = idx[b][ok].astype(np.int64)
        np.add.at(out[b].T, j, terms[b][:, ok].T)
        np.add.at(mass[b].T, j, np.abs(terms[b][:, ok]).T)
    assert mass.max(initial=0) < EXACT_LIMIT, "%s: exactness precondition violated (%d units)" % (what, mass.max())
    return out


def scatter_naive(idx, terms, n):
    """scatter_units as a plain Python loop (for the tiny sizes of the CPU tests)."""
    B, C, T = terms.shape
    out = np.zeros((B, C, n), np.int64)
    for b in range(B):
        for t in range(T):
            j = int(idx[b, t])
            if 0 <= j < n:
                for c in range(C):
                    out[b, c, j] += int(terms[b, c, t])
    return out


def dwx_units(g, rel4, what=""):
    """dwx[c, k] = sum over samples and positions of g[b, c, t] * rel4[b, k, t] in int64; g (B, C, T), rel4 (B, 3, T) integers."""
    g, rel4 = g.astype(np.int64), rel4.astype(np.int64)
    mass = np.einsum("bct,bkt->ck", np.abs(g), np.abs(rel4))
    assert mass.max(initial=0) < EXACT_LIMIT, "%s: exactness precondition violated (%d units)" % (what, mass.max())
    return np.einsum("bct,bkt->ck", g, rel4)


def nc_grad_units(mask4, idx, go8, what=""):
    """Gradient of the p = 1 neighbour-consistency term in units of 1 / (8 k): mask4 (B, N, C) integers (mask * 4), idx (B, N, k),
    go8 (B, N) integers (grad_out * 8):  grad[i] = G_i sum_j sign(m_i - m_idx[i,j]) - sum_{(i',j): idx[i',j] = i} G_i' sign(m_i' - m_i)."""
    B, N, C = mask4.shape
    out = np.zeros((B, N, C), np.int64)
    mass = np.zeros((B, N, C), np.int64)
    for b in range(B):
        m = mask4[b].astype(np.int64)
        j = idx[b].astype(np.int64)
        contrib = go8[b].astype(np.int64)[:, None, None] * np.sign(m[:, None, :] - m[j])     # (N, k, C)
        out[b] = contrib.sum(1)
        mass[b] = np.abs(contrib).sum(1)
        np.add.at(out[b], j.reshape(-1), -contrib.reshape(-1, C))
        np.add.at(mass[b], j.reshape(-1), np.abs(contrib).reshape(-1, C))
    assert mass.max(initial=0) < EXACT_LIMIT, "%s: exactness precondition violated (%d units)" % (what, mass.max())
    return out


def nc_grad_naive(mask4, idx, go8):
    B, N, C = mask4.shape
    k = idx.shape[2]
    out = np.zeros((B, N, C), np.int64)
    for b in range(B):
        for i in range(N):
            for jj in range(k):
                d = int(idx[b, i, jj])
                for c in range(C):
                    s = int(np.sign(int(mask4[b, i, c]) - int(mask4[b, d, c]))) * int(go8[b, i])
                    out[b, i, c] += s
                    out[b, d, c] -= s
    return out


# ---- the cases: inputs and references, built once per (shape, pattern) and shared by the modes ------------------------------------
def _seed(*key):
    return abs(hash(tuple(key))) % (2 ** 32)     # tuples of ints hash reproducibly (the names enter as their position)


@functools.lru_cache(maxsize=None)
def group_case(n, P, S, C, name):
    """Grouping gradient: idx (2, P, S), g (2, C, P, S) integers in [-4, 4], rel (2, 3, T) multiples of 1/4 in [-2, 2];
    ref (2, C, n) int64 = scatter of g, dwx (C, 3) int64 in units of 1/4."""
    rng = np.random.default_rng(_seed(1, n, P, S, C, NAMES.index(name)))
    B, T = 2, P * S
    idx = pattern(name, B, P, S, n, rng)
    g = rng.integers(-4, 5, (B, C, P, S))
    rel4 = rng.integers(-8, 9, (B, 3, T))
    flat = idx.reshape(B, T)
    what = "group n=%d T=%d %s" % (n, T, name)
    case = dict(idx=idx, g=g.astype(np.float32), rel=(rel4 / 4.0).astype(np.float32), g_int=g, rel4=rel4,
                ref=scatter_units(flat, g.reshape(B, C, T), n, what), dwx=dwx_units(g.reshape(B, C, T), rel4, what))
    return case


@functools.lru_cache(maxsize=None)
def interp_case(m, N, C, name):
    """Interpolation gradient: idx (2, N, 3) into m points, g (2, C, N) integers in [-4, 4], w (2, N, 3) from {1/4, 1/2, 1, 2};
    position t = 3 i + k carries g[i] * w[i, k]; ref (2, C, m) int64 in units of 1/4."""
    rng = np.random.default_rng(_seed(2, m, N, C, NAMES.index(name)))
    B = 2
    idx = pattern(name, B, N, 3, m, rng)
    g = rng.integers(-4, 5, (B, C, N))
    w4 = np.array([1, 2, 4, 8])[rng.integers(0, 4, (B, N, 3))]
    terms = (g[:, :, :, None] * w4[:, None, :, :]).reshape(B, C, 3 * N)
    return dict(idx=idx, g=g.astype(np.float32), w=(w4 / 4.0).astype(np.float32),
                ref=scatter_units(idx.reshape(B, 3 * N), terms, m, "interp m=%d N=%d %s" % (m, N, name)))


@functools.lru_cache(maxsize=None)
def nb_case(N, k, name):
    """Neighbour lists (2, N, k) of pattern `name` with, per sample, the edges and multiplicities of their transposed lists."""
    rng = np.random.default_rng(_seed(3, N, k, NB_NAMES.index(name)))
    idx = nb_pattern(name, 2, N, k, rng)
    edges = [nb_edges(idx[b]) for b in range(2)]
    return dict(idx=idx, keys=[e[0] for e in edges], mult=np.stack([e[1] for e in edges]))


@functools.lru_cache(maxsize=None)
def nc_case(N, k, C, name):
    """p = 1 gradient with exact sums: mask (2, N, C) from {0, 1/4, 1/2}, grad_out (2, N) multiples of 1/8 in [-2, 2];
    ref (2, N, C) int64 in units of 1 / (8 k) (k a power of two: 1 / k is exact)."""
    rng = np.random.default_rng(_seed(4, N, k, C, NB_NAMES.index(name)))
    idx = nb_case(N, k, name)["idx"]
    mask4 = rng.integers(0, 3, (2, N, C))
    go8 = rng.integers(-16, 17, (2, N))
    return dict(mask=(mask4 / 4.0).astype(np.float32), go=(go8 / 8.0).astype(np.float32),
                ref=nc_grad_units(mask4, idx, go8, "nc N=%d k=%d C=%d %s" % (N, k, C, name)))


def units_to_f32(ref, unit):
    """The int64 reference back in fp32 (exact: |ref| < 2**24 and the unit is a power of two)."""
    out = (ref.astype(np.float64) * unit).astype(np.float32)
    assert np.array_equal(out.astype(np.float64), ref.astype(np.float64) * unit)
    return out


def order_free_bound(lengths, mass, extra=0):
    """|fl(sum of L terms, any order) - sum| <= gamma_L * sum |term|, gamma_L = L u / (1 - L u), u = 2**-24 (L - 1 additions and
    `extra` further roundings per term, e.g. the product of the interpolation form)."""
    L = (lengths + extra).astype(np.float64) * 2.0 ** -24
    return L / (1.0 - L) * mass

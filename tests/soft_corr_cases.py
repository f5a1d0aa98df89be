"""Decided inputs and a float64 reference for the soft-correspondence kernels (csrc/soft_nn.hip: ogc_soft_nn_target, both forms;
csrc/soft_carry.hip: ogc_soft_carry), for tests/test_soft_corr_truth_gpu.py.  Host side: numpy for the inputs and the conditions,
torch float64 for the reference, torch float32 for the yardstick; no GPU needed, the library is not imported.  The twin of
tests/bn_cases.py.  "Decided" here: rounding is negligible, so every row of every output can be held against float64 tightly
enough that a structural mistake (a dropped candidate, a mis-merged lane group, a mask slot of the next row, padding with weight)
shows, and no row sits near the 1e-10 clamp unless it is meant to:

  * candidates p2: lattice points q / 16 + off, q integer in a cube of half-width round(cbrt(2 n2) / 2) steps, duplicates
    allowed: tens to hundreds of candidates carry weight for every query.  off = 8 keeps a padding slot's origin far away;
    off = 0 (`origin` cases) centres the cloud on it;
  * query i is candidate i % n2 moved by one lattice step or none per axis;
  * all coordinates are multiples of 1/16 below 16 in magnitude, so (-2a) . b + |a|^2 + |b|^2 is an integer below 2^24 in units
    of 1/256 at every partial sum: exact in fp32 in any order;
  * temperature TAU = 1/8: the division is exact;
  * soft-NN masks are dyadic: candidates 0.75 on their label and 0.25 on (label + 1) % k, queries the label of their source
    candidate with 0.25 on (label - 1) % k; labels uniform in [0, k), so slot k - 1 and the next row's slot 0 are both populated.
    Every product and every sum of the consistency <m1, m2> is exact in fp32;
  * every eleventh query from the fifth is a CLAMP ROW, m1 = 2^-40 onehot(label): A / Z < 1e-10 and the output is
    (V / Z) * 1e10, about 1e-2, in which Z does NOT cancel;
  * soft-carry x: rows on the lattice n / 64, non-negative, summing to 1 over the first c - 1 columns (half of the mass on a
    random column of the row's own), a last column of ones; c = 1 is the ones column alone;
  * B > 1: every sample is drawn independently.

The reference is the op sequence of the original (oa_icp.py:62-72;  softmax(-cdist / tau) @ x  for the carry) in torch float64 on
the host; the same sequence in float32 on the host is the yardstick.  The gate of an output tensor and row class is
test_group_norm_truth_gpu.Table's:  max(4 * err_torch32, 8 * 2**-24 * max|truth|), separately for the clamp rows and the others.

make() asserts, and the unmarked tests re-check by another route (torch, weights normalised by softmax):
  1  d2 exact in fp32 (two summation orders against sum (a - b)^2 in float64); masks and x exactly on their lattices;
  2  coverage.  n1 >= n2: every candidate j has a query whose float64 output moves by >= COVER x that row's gate when j is left
     out (closed form, all j at once).  n1 < n2 (the n1-edge cases): every query has two candidates that each hold >= 1/16 of
     the row's weight.  A c = 1 carry case has no coverage to ask for: its only column is 1 whatever the weights;
  3  clamp.  Non-clamp rows have A / Z >= 1e-3; clamp rows have A / Z <= 1e-11 and move by >= COVER x their gate when Z doubles;
  4  `origin` cases: counting the kernel's padding slots as real candidates at the origin (zero mask, zero x) moves some row by
     >= COVER x its gate — for soft-NN a clamp row (elsewhere Z cancels).
A case that misses one gets another seed; the thresholds stay, and no row is left out.
"""
import collections
import functools

import numpy as np
import torch

TAU = 0.125
STEP = 1.0 / 16
U = 2.0 ** -24
COVER = 32.0
CLAMP_SCALE = 2.0 ** -40
MIN_SHARE = 1.0 / 16

# op "nn": k = mask slots; op "carry": k = columns of x.  off: added to every coordinate (8, or 0 for the origin cases).
Case = collections.namedtuple("Case", "op B n1 n2 k seed off")


def nn(B, n1, n2, k, seed=0, off=8.0):
    return Case("nn", B, n1, n2, k, seed, off)


def carry(B, n1, n2, c, seed=0, off=8.0):
    return Case("carry", B, n1, n2, c, seed, off)


def case_id(c):
    return "%s-%dx%dx%dx%d%s%s" % (c.op, c.B, c.n1, c.n2, c.k, "-origin" if c.off == 0 else "", "-s%d" % c.seed if c.seed else "")


N1_EDGES = (1, 31, 32, 33, 63, 64, 65)

# ogc_soft_nn_target: n2 < 256 the lane-per-query kernel (8 wavefronts split the candidates: per = ceil(n2 / 8); chunks of 8;
# KMAX 8 / 16 / 32 by k; SN_TILE 64, or 32 at KMAX 32; 64 queries per workgroup)
NN_LANE_CASES = [
    nn(1, 70, 1, 3),                    # n2 = 1: seven wavefronts with an empty share
    nn(1, 70, 7, 1),                    # per = 1: one wavefront empty; k = 1
    nn(1, 70, 8, 8),                    # per = 1, no wavefront empty; k = 8: KMAX 8 full
    nn(1, 70, 9, 9),                    # per = 2: three wavefronts empty, the fifth holds one candidate; KMAX 16 from below
    nn(3, 130, 100, 16),                # a share of 13: one full chunk and a ragged one; KMAX 16 full; B = 3; three query blocks
    nn(1, 130, 100, 17),                # KMAX 32 from below, SN_TILE 32
    nn(1, 130, 100, 6, off=0.0),        # padding at the origin: 28 padded chunk slots
    nn(1, 255, 255, 6),                 # the last size of the lane form: shares of 32 (31 in the last wavefront)
    nn(1, 255, 255, 32),                # KMAX 32 full: the share fills SN_TILE = 32 exactly
]
# n2 >= 256 the matrix-core form (tiles of 16 candidates, tiles_pad = ceil(tiles / 16) * 16, 8 wavefronts of tiles_pad / 8 tiles;
# NM = 2 / 3 / 4 / 8 mask MFMAs by k; 32 queries per workgroup)
NN_MFMA_CASES = [
    nn(1, 256, 256, 1, seed=28),        # no padding at all; k = 1 (every candidate consistent with every query: the thinnest
                                        # coverage of the list, hence the seed)
    nn(3, 257, 257, 8),                 # one real candidate in the second group of 16 tiles, 255 padding slots: the fifth
                                        # wavefront holds it alone, three have nothing but padding; NM = 2 full; B = 3
    nn(1, 257, 257, 9),                 # NM = 3 from below
    nn(1, 257, 257, 10, off=0.0),       # padding at the origin
    nn(1, 300, 257, 12),                # NM = 3 full; n1 % 32 != 0
    nn(1, 300, 257, 13),                # NM = 4 from below
    nn(1, 257, 257, 16),                # NM = 4 full
    nn(1, 257, 257, 17),                # NM = 8 from below
    nn(1, 257, 257, 32),                # NM = 8 full
    nn(1, 511, 511, 10),                # one slot short of two groups
    nn(1, 512, 512, 10),                # two groups, no padding
    nn(1, 513, 513, 10),                # three groups: per = 6 tiles
]
# n1 around the query blocks (64 lane, 32 matrix-core) with the candidates fixed.  Below n2 queries every row must lean on two
# candidates (condition 2): on so dense a cloud that needs few consistent candidates per row, hence 10 and 20 slots, and for
# three of the matrix-core cases another seed
NN_EDGE_CASES = [nn(1, n1, 64, 10) for n1 in N1_EDGES] + \
    [nn(1, n1, 256, 20, seed={33: 1, 63: 2, 64: 1}.get(n1, 0)) for n1 in N1_EDGES]
NN_CASES = NN_LANE_CASES + NN_MFMA_CASES + NN_EDGE_CASES
# the matrix-core sizes once more through the lane form (beyond one staged tile per wavefront; one child process)
NN_LANE_LARGE = [c for c in NN_MFMA_CASES + NN_EDGE_CASES if c.n2 >= 256]

# ogc_soft_carry: tiles_pad = ceil(ceil(n2 / 16) / 4) * 4, 4 wavefronts; NT = ceil(c / 16) channel tiles; QT = 4 query tiles per
# workgroup up to 32 columns, 2 above; the wrapper splits x beyond 64 columns
CARRY_CASES = [
    carry(1, 70, 40, 1),                # the ones column alone
    carry(1, 70, 1, 5),                 # n2 = 1: 63 padding slots, three wavefronts all padding
    carry(3, 70, 15, 16),               # NT = 1 full; one ragged tile; B = 3
    carry(1, 70, 16, 17),               # NT = 2 from below; one full tile
    carry(1, 70, 17, 32),               # NT = 2 full; the second tile holds one candidate
    carry(1, 70, 63, 33),               # NT = 3 from below, QT = 2; four tiles, the last ragged
    carry(1, 70, 64, 48),               # NT = 3 full; no padding
    carry(1, 70, 65, 49),               # NT = 4 from below; tiles_pad = 8, three of them padding
    carry(1, 70, 65, 21, off=0.0),      # padding at the origin: 63 slots
    carry(1, 257, 257, 64),             # NT = 4 full; 20 tiles, per = 5
    carry(3, 130, 100, 65),             # the wrapper's column split: 64 + 1
    carry(1, 130, 100, 100),            # 64 + 36
]
# n1 around the query blocks (64 queries up to 32 columns, 32 above); two tiles of candidates, two wavefronts all padding
CARRY_EDGE_CASES = [carry(1, n1, 30, 20) for n1 in N1_EDGES] + [carry(1, n1, 30, 40) for n1 in N1_EDGES]
CARRY_ALL = CARRY_CASES + CARRY_EDGE_CASES

# the memory-contract tests of soft-NN, one per form
CONTRACT_CASES = [nn(2, 203, 149, 10), nn(2, 300, 300, 10)]
REUSE_BIG, REUSE_SMALL = nn(1, 513, 513, 10), nn(1, 257, 257, 10, off=0.0)

ALL_CASES = NN_CASES + CARRY_ALL


def half_width(n2):
    return int(round(np.cbrt(2.0 * n2) / 2))


def clamp_rows(n1):
    r = np.zeros(n1, bool)
    r[5::11] = True
    return r


def nn_lane_padding(n2):
    """Padding slots the lane-per-query kernel weighs for one query: each wavefront's share, rounded up to chunks of 8."""
    per = -(-n2 // 8)
    shares = [max(0, min(n2, (w + 1) * per) - w * per) for w in range(8)]
    return sum(-(-s // 8) * 8 - s for s in shares)


def nn_mfma_padding(n2):
    tiles = -(-n2 // 16)
    return -(-tiles // 16) * 16 * 16 - n2


def carry_padding(n2):
    tiles = -(-n2 // 16)
    return -(-tiles // 4) * 4 * 16 - n2


def padding_slots(c):
    if c.op == "carry":
        return carry_padding(c.n2)
    return nn_mfma_padding(c.n2) if c.n2 >= 256 else nn_lane_padding(c.n2)


def _d2_is_exact(p1, p2):
    """The kernels' (-2a) . b + |a|^2 + |b|^2 in fp32, in two summation orders, against sum (a - b)^2 in float64."""
    a, b = p1[:, :, None, :], p2[:, None, :, :]
    want = ((a.astype(np.float64) - b.astype(np.float64)) ** 2).sum(-1)
    an = ((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2]).astype(np.float32)
    bn = ((b[..., 0] * b[..., 0] + b[..., 1] * b[..., 1]) + b[..., 2] * b[..., 2]).astype(np.float32)
    m = np.float32(-2) * a
    one = (((m[..., 0] * b[..., 0] + m[..., 1] * b[..., 1]) + m[..., 2] * b[..., 2]) + an) + bn
    two = (an + bn) + (m[..., 2] * b[..., 2] + (m[..., 1] * b[..., 1] + m[..., 0] * b[..., 0]))
    assert one.dtype == np.float32 and two.dtype == np.float32
    return bool((one.astype(np.float64) == want).all() and (two.astype(np.float64) == want).all())


def reference(c, d, dtype):
    """The op sequence of the original in torch `dtype` on the host -> (B, n1, 3) targets or (B, n1, c) carried values."""
    p1, p2 = torch.from_numpy(d["p1"]).to(dtype), torch.from_numpy(d["p2"]).to(dtype)
    corr = (-torch.cdist(p1, p2) / TAU).softmax(-1)
    if c.op == "carry":
        return corr @ torch.from_numpy(d["x"]).to(dtype)
    m1, m2 = torch.from_numpy(d["m1"]).to(dtype), torch.from_numpy(d["m2"]).to(dtype)
    corr = corr * torch.einsum("bmk,bnk->bmn", m1, m2)
    corr = corr / corr.sum(-1, keepdim=True).clamp(1e-10)
    return torch.einsum("bmn,bnj->bmj", corr, p2)


def class_gates(c, truth, yard):
    """{row class: (rows (n1,) bool, gate, err_torch32)} — Table's gate per class, from the host yardstick."""
    clamp = clamp_rows(c.n1) if c.op == "nn" else np.zeros(c.n1, bool)
    out = {}
    for name, rows in (("rows", ~clamp), ("clamp", clamp)):
        if rows.any():
            t = truth[:, rows].double()
            err = float((yard[:, rows].double() - t).abs().max())
            out[name] = (rows, max(4 * err, 8 * U * float(t.abs().max())), err)
    return out


@functools.lru_cache(maxsize=None)
def inputs(c):
    """dict: p1 (B, n1, 3), p2 (B, n2, 3), and m1 (B, n1, k), m2 (B, n2, k) or x (B, n2, c) — fp32 numpy, condition 1 asserted."""
    rng = np.random.default_rng([c.seed, c.B, c.n1, c.n2, c.k, int(c.off), 31 if c.op == "nn" else 32])
    B, n1, n2, k = c.B, c.n1, c.n2, c.k
    h = half_width(n2)
    q2 = rng.integers(-h, h + 1, (B, n2, 3))
    src = np.arange(n1) % n2
    q1 = q2[:, src] + rng.integers(-1, 2, (B, n1, 3))
    d = {"p1": (q1 * STEP + c.off).astype(np.float32), "p2": (q2 * STEP + c.off).astype(np.float32)}
    assert _d2_is_exact(d["p1"], d["p2"]), case_id(c)
    clamp = clamp_rows(n1) if c.op == "nn" else np.zeros(n1, bool)
    if c.op == "nn":
        lab2 = rng.integers(0, k, (B, n2))
        lab1 = lab2[:, src]
        eye = np.eye(k, dtype=np.float32)
        d["m2"] = np.float32(0.75) * eye[lab2] + np.float32(0.25) * eye[(lab2 + 1) % k]
        m1 = np.float32(0.75) * eye[lab1] + np.float32(0.25) * eye[(lab1 - 1) % k]
        m1[:, clamp] = np.float32(CLAMP_SCALE) * eye[lab1[:, clamp]]
        d["m1"] = m1
        assert set(np.unique(d["m2"])) <= {0.0, 0.25, 0.75, 1.0}
        assert set(np.unique(m1[:, ~clamp])) <= {0.0, 0.25, 0.75, 1.0} and set(np.unique(m1[:, clamp])) <= {0.0, CLAMP_SCALE}
    else:
        x = np.ones((B, n2, k), np.float32)
        if k > 1:
            own = np.eye(k - 1)[rng.integers(0, k - 1, (B, n2))]
            x[..., :k - 1] = rng.multinomial(64, 0.5 * own + 0.5 / (k - 1)) / 64.0
        d["x"] = x
        x64 = x.astype(np.float64) * 64
        assert bool((x64 == np.rint(x64)).all() and (x64 >= 0).all() and (x[..., -1] == 1).all())
        assert k == 1 or bool((x64[..., :-1].sum(-1) == 64).all())
    return d


@functools.lru_cache(maxsize=None)
def make(c):
    """inputs(c) and: truth (torch float64) and yard (torch float32) from reference(), gates (class_gates), and what the
    conditions measured: cover (smallest over candidates of the largest movement in units of the row's gate; n1 >= n2), share
    (smallest second-largest weight share of a row; n1 < n2), az_rows / az_clamp (extremes of A / Z), z2 (smallest movement of a
    clamp row when Z doubles, in gates), pad (largest movement when the padding slots count, in gates; origin cases)."""
    d = dict(inputs(c))
    B, n1, n2, k = c.B, c.n1, c.n2, c.k
    clamp = clamp_rows(n1) if c.op == "nn" else np.zeros(n1, bool)
    d["truth"], d["yard"] = reference(c, d, torch.float64), reference(c, d, torch.float32)
    d["gates"] = class_gates(c, d["truth"], d["yard"])
    gate_row = np.zeros(n1)
    for rows, gate, _ in d["gates"].values():
        gate_row[rows] = gate

    # the conditions, in float64 with the weights unnormalised (exp(-d / tau) stays far from underflow on these clouds)
    a, b = d["p1"].astype(np.float64), d["p2"].astype(np.float64)
    e = np.exp(-np.sqrt(((a[:, :, None] - b[:, None]) ** 2).sum(-1)) / TAU)                  # (B, n1, n2)
    Z = e.sum(-1)
    pad_e = padding_slots(c) * np.exp(-np.sqrt((a * a).sum(-1)) / TAU)                       # (B, n1): the padding as candidates
    with np.errstate(divide="ignore", invalid="ignore"):
        if c.op == "nn":
            W = e * np.einsum("bmk,bnk->bmn", d["m1"].astype(np.float64), d["m2"].astype(np.float64))
            A, V = W.sum(-1), W @ b
            target = lambda z, a_, v: (v / z[..., None]) / np.maximum(a_ / z, 1e-10)[..., None]      # noqa: E731
            out = target(Z, A, V)
            left = target(Z[..., None] - e, A[..., None] - W, V[:, :, None] - W[..., None] * b[:, None])
            az = A / Z
            d["az_rows"] = float(az[:, ~clamp].min())
            assert d["az_rows"] >= 1e-3, (case_id(c), d["az_rows"])
            if clamp.any():
                d["az_clamp"] = float(az[:, clamp].max())
                d["z2"] = float((np.abs(target(2 * Z, A, V) - out).max(-1) / gate_row)[:, clamp].min())
                assert d["az_clamp"] <= 1e-11 and d["z2"] >= COVER, (case_id(c), d["az_clamp"], d["z2"])
            padded = target(Z + pad_e, A, V)
            share = W / A[..., None]
        else:
            x = d["x"].astype(np.float64)
            S = e @ x
            out = S / Z[..., None]
            left = (S[:, :, None] - e[..., None] * x[:, None]) / (Z[..., None] - e)[..., None]
            padded = S / (Z + pad_e)[..., None]
            share = e / Z[..., None]
        assert float(np.abs(out - d["truth"].numpy()).max()) <= 1e-12 * float(np.abs(out).max()), case_id(c)
        move = np.abs(left - out[:, :, None]).max(-1)                                        # (B, n1, n2)
        move[~(Z[..., None] - e > 0)] = np.inf                                               # the only candidate: nothing is left
    if n1 >= n2 and not (c.op == "carry" and k == 1):
        d["cover"] = float((move / gate_row[None, :, None]).max(axis=1).min())
        assert d["cover"] >= COVER, (case_id(c), d["cover"])
    if n1 < n2:
        d["share"] = float(np.sort(share, axis=-1)[..., -2].min())
        assert d["share"] >= MIN_SHARE, (case_id(c), d["share"])
    if c.off == 0 and padding_slots(c):
        ratio = np.abs(padded - out).max(-1) / gate_row
        d["pad"] = float((ratio[:, clamp] if c.op == "nn" else ratio).max())
        assert d["pad"] >= COVER, (case_id(c), d["pad"])
    return d

"""Decided inputs and a float64 reference for the dynamic and invariance terms of the unsupervised loss (csrc/seg_loss.hip:
ogc_rigid_moments / _translation / _blend, ogc_mask_iou, ogc_matched_distance; csrc/kabsch.hip between them), for
tests/test_seg_loss_truth_gpu.py.  Host side: numpy for the inputs and the exact sums, torch float64 for the reference, torch
float32 for the yardstick; no GPU needed, the library is not imported.  The twin of tests/bn_cases.py and
tests/soft_corr_cases.py.  "Decided": no sign of a residual component, no norm and no arg-max is within rounding of its
threshold, so every row of every tensor is compared — tightly enough that a dropped point, a row of the next block, a wrong
slab or a slot beyond the first pass of an LDS fill shows.

The reference is the op sequence of the original written afresh in torch (losses/seg_loss_unsup.py:10-98 for the dynamic term,
:212-262 for the invariance term), with  c1^T diag(m) c2  as  (c1 * m)^T c2  (the original builds an N x N diagonal matrix per
slot) and, where S is exactly zero (every rotation is optimal), R = I: what torch's SVD of a zero matrix and the kernel both give.

Dynamic term, a case (VB, N, K):
  * pc: multiples of 1/16, |.| <= 3.  The regular points come in PAIRS that share position, label and second slot and carry
    opposite offsets (below): the offsets then cancel in every moment and the fit is the motion up to the lattice rounding — with
    four points in a slot as with four hundred.  The rows are shuffled, partners lie anywhere;
  * mask: 0.75 on the point's label slot, 0.25 on a second one (K = 1, and the planar / mirrored slots' points: both on the
    label, 1.0).  Every product and every partial sum of the 16 moments is an integer below 2^53 in units of 2^-14: exact in
    float64 in any order (`moments`);
  * pc2 = round16(R_l p + t_l) + o: a rotation about the origin by 0.005..0.015 rad about a random axis and a translation of
    +-1/16 per axis, per (cloud, label); o = +-{3, 4, 5}/16 on every axis;
  * zero rows (N >= 63: two per cloud): mask row all zero, pc2 the origin: residual, and both gradient rows, exactly 0.
    N = 1: both live slots hold that one point, R = I, t = q - p, and the residual is exactly 0 as well;
  * special "zs": slot 1 has weight 0 at every point (W = 0 -> NaN means -> invalid -> R = I, t = 0 bit for bit); slot K - 1
    has one live point (S = 0 exactly, valid, R = I, t = the fp32 difference of its two positions);
  * special "all", also: slot 2 is planar (its points have z = 3/16; no other point puts weight there: S has rank 2); slot 4
    is mirrored (pc2 = the motion of the point reflected in z, the thin axis of its box 3 x 2 x 0.75: det S < 0).

  make_dyn() asserts, and the unmarked tests re-derive from the moments with torch float64:
    1  every fitted slot (two live points or more) has (sigma2 + sign(det S) sigma3) / sigma1 >= MIN_RATIO;
    2  outside the zero rows every residual component is >= MIN_RESIDUAL in magnitude (p = 1 and, a fortiori, the p = 2 norm);
    3  replacing the (R, t) of any slot with a live point by the identity moves some row of the p = 1 and of the p = 2 residual
       by >= COVER x that tensor's gate; every live weight is >= 0.25, so leaving a point out moves the exact W of its slots.
  A case that misses one gets another seed; the thresholds stay and no row is left out.

Invariance term, a case (PB, N, K):
  * masks are multiples of 1/64 below 1; the label slot of a row exceeds the others by 1..4 steps; from K = 4 the last K // 4
    slots of mask1 are never an arg-max (all-zero IoU rows and columns: the matching is tie-broken by scipy's rule);
  * mask2 is mask1 with the slots permuted (no fixed point) and every entry moved by up to two steps; 85 % of the rows keep
    their (permuted) label, the others take another one;
  * tie rows (every 29th from 7 in mask1, every 31st from 11 in mask2): two used slots hold the same maximum, the first wins;
  * equal rows (every 23rd from 13, no tie row among them): mask2[i, col12] == mask1[i] exactly: d12 = 0 and the p = 2
    gradient row is exactly 0.  col12 is scipy's assignment on the final masks (make_inv() iterates to the fixed point).
  make_inv() asserts the top-2 gap >= 1/64 outside the tie rows, the ties, the equal rows and that col12 is not the identity.

The gate of a float comparison is test_group_norm_truth_gpu.Table's, max(4 * err_torch32, 8 * 2**-24 * max|truth|); everything
else is exact equality.
"""
import collections
import functools

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

U = 2.0 ** -24
MIN_RATIO = 1.0 / 8
MIN_RESIDUAL = 2.0 ** -10
COVER = 32.0
KMAX = 32          # SL_KMAX
THREADS = 256      # SL_THREADS

Dyn = collections.namedtuple("Dyn", "VB N K seed special")
Inv = collections.namedtuple("Inv", "PB N K seed")


def dyn(VB, N, K, seed=0, special=""):
    return Dyn(VB, N, K, seed, special)


def inv(PB, N, K, seed=0):
    return Inv(PB, N, K, seed)


def case_id(c):
    s = "%s-%dx%dx%d" % ("dyn" if isinstance(c, Dyn) else "inv", c[0], c.N, c.K)
    return s + ("-" + c.special if getattr(c, "special", "") else "") + ("-s%d" % c.seed if c.seed else "")


def sl_chunks(n, rows):
    """sl_chunks of csrc/seg_loss.hip -> (chunks before the halving, after)."""
    first = chunks = -(-n // THREADS)
    while chunks > 1 and chunks * rows > 4096:
        chunks = (chunks + 1) // 2
    return first, chunks


N_EDGES = (1, 63, 64, 65, 70, 255, 256, 257)
# ogc_rigid_moments: grid (sl_chunks(N, VB * K), K, VB) of 256 threads, block_sum_doubles over 4 wavefronts; ogc_rigid_blend: grid
# (ceil(N / 256), VB), the R | t of all slots in LDS: K * 12 floats filled by 256 threads
DYN_EDGE_CASES = [dyn(2, N, K) for N in N_EDGES for K in (1, 2, 3)]   # one row; a wavefront less one, full, plus one; 70; a block
#                                                                       less one, full, plus one: the second block and moment chunk
DYN_SLOT_CASES = [
    dyn(2, 257, 21, special="zs"),      # 252 of 256: the last K whose LDS fill is a single pass
    dyn(2, 257, 22, special="zs"),      # 264: the second pass, 8 entries (slot 21 from its fifth)
    dyn(2, 257, 31, special="zs"),      # 372
    dyn(2, 257, 32, seed=1, special="zs"),   # 384: SL_KMAX.  Four pairs of points per slot: seed 0 misses condition 1
    dyn(3, 257, 8, special="all"),      # VB = 3: the batch strides; every special slot
]
DYN_CHUNK_CASES = [
    dyn(5, 6657, 32),                   # 27 chunks -> 14: the moment loop strides twice in 13 of them; 26 full blend blocks + 1 row
    dyn(32, 1025, 32),                  # 5 -> 3
    dyn(128, 600, 32),                  # 3 -> 2 -> 1: one workgroup strides three times, the last ragged
]
DYN_CASES = DYN_EDGE_CASES + DYN_SLOT_CASES + DYN_CHUNK_CASES

# ogc_mask_iou: grid (sl_chunks(N, PB), PB), K * K counters in LDS zeroed and flushed by 256 threads; ogc_matched_distance: grid
# (ceil(N / 256), PB)
INV_EDGE_CASES = [inv(2, N, K) for N in (1, 255, 256, 257) for K in (1, 2, 16, 17, 31, 32)]   # K * K = 256 one pass, 289 two
INV_CASES = INV_EDGE_CASES + [
    inv(3, 257, 10),                    # PB = 3
    inv(64, 16641, 2),                  # 66 chunks -> 33: the first workgroup strides three times
    inv(2048, 600, 2),                  # 3 -> 2
]


# ---- dynamic term: inputs -----------------------------------------------------------------------------------------------------------
def slot_roles(c):
    """{"zero": slot | None, "single": ..., "planar": ..., "mirror": ..., "plain": [slots]}"""
    r = dict(zero=None, single=None, planar=None, mirror=None)
    if c.special:
        r["zero"], r["single"] = 1, c.K - 1
    if c.special == "all":
        r["planar"], r["mirror"] = 2, 4
    r["plain"] = [s for s in range(c.K) if s not in r.values()]
    return r


def _rotation(axis, angle):
    axis = axis / np.linalg.norm(axis)
    kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * kx + (1 - np.cos(angle)) * (kx @ kx)


def _cloud(c, rng):
    """One cloud: q (N, 3) and q2 (N, 3) in lattice steps (int64), w (N, K) in quarters (int64)."""
    N, K = c.N, c.K
    roles = slot_roles(c)
    plain = roles["plain"]
    n_zero = 2 if N >= 63 else 0
    n_units = N - n_zero - (1 if roles["single"] is not None else 0)
    n_pairs, odd = n_units // 2, n_units % 2
    cycle = list(plain)
    for s in (roles["planar"], roles["mirror"]):
        if s is not None:
            cycle += [s] * 3
    cycle = [cycle[i] for i in rng.permutation(len(cycle))]
    u = n_pairs + odd                                               # distinct positions; the last is unpaired when odd
    label = np.array([cycle[i % len(cycle)] for i in range(u)] + ([roles["single"]] if roles["single"] is not None else []), int)
    tot = len(label)
    second = label.copy()
    for i in range(tot):
        others = [s for s in plain if s != label[i]]
        if others and label[i] != roles["mirror"]:
            second[i] = others[rng.integers(len(others))]
    pos = rng.integers(-48, 49, (tot, 3))
    pos[label == roles["planar"], 2] = 3
    thin = label == roles["mirror"]
    pos[thin, 1] = rng.integers(-32, 33, int(thin.sum()))
    pos[thin, 2] = rng.integers(-12, 13, int(thin.sum()))
    moved = np.empty((tot, 3))
    for s in range(K):
        rot = _rotation(rng.standard_normal(3), rng.uniform(0.005, 0.015) * rng.choice([-1, 1]))
        shift = rng.choice([-1.0, 1.0], 3)
        src = pos[label == s].astype(np.float64)
        if s == roles["mirror"]:
            src = src * np.array([1.0, 1.0, -1.0])
        moved[label == s] = src @ rot.T + shift
    moved = np.rint(moved).astype(np.int64)
    off = rng.integers(3, 6, (tot, 3)) * rng.choice([-1, 1], (tot, 3))
    rep = np.concatenate([np.arange(n_pairs), np.arange(tot)])      # the pairs' second halves, then every unit once
    sign = np.concatenate([-np.ones(n_pairs, int), np.ones(tot, int)])
    q, q2 = pos[rep], moved[rep] + sign[:, None] * off[rep]
    w = np.zeros((len(rep), K), np.int64)
    np.add.at(w, (np.arange(len(rep)), label[rep]), 3)
    np.add.at(w, (np.arange(len(rep)), second[rep]), 1)
    q = np.concatenate([q, rng.integers(-48, 49, (n_zero, 3))])
    q2 = np.concatenate([q2, np.zeros((n_zero, 3), np.int64)])
    w = np.concatenate([w, np.zeros((n_zero, K), np.int64)])
    order = rng.permutation(N)
    return q[order], q2[order], w[order]


@functools.lru_cache(maxsize=2)
def dyn_inputs(c):
    """dict: pc, pc2 (VB, N, 3), mask (VB, N, K), grad (VB, N) — fp32 numpy; zero_rows (VB, N) bool; live (VB, K) points with
    weight per slot."""
    rng = np.random.default_rng([c.seed, c.VB, c.N, c.K, len(c.special), 41])
    clouds = [_cloud(c, rng) for _ in range(c.VB)]
    q, q2, w = (np.stack([cl[i] for cl in clouds]) for i in range(3))
    d = {"pc": (q / 16.0).astype(np.float32), "pc2": (q2 / 16.0).astype(np.float32), "mask": (w / 4.0).astype(np.float32)}
    k = rng.integers(1, 33, (c.VB, c.N)) * rng.choice([-1, 1], (c.VB, c.N))
    d["grad"] = (k / 16.0).astype(np.float32)
    d["zero_rows"] = (w == 0).all(axis=2) | (c.N == 1)
    d["live"] = (w > 0).sum(axis=1)
    assert np.abs(q).max() <= 48 and np.abs(q2).max() < 64 * 16
    assert set(np.unique(w)) <= {0, 1, 3, 4}
    return d


def moments(d):
    """The 16 exact moments per (cloud, slot), numpy float64 (VB, K, 16): {W, sum w p (3), sum w q (3), sum w p q^T (9)}."""
    w, p, q = (d[n].astype(np.float64) for n in ("mask", "pc", "pc2"))
    VB, _, K = w.shape
    wp = np.einsum("bnk,bni->bnki", w, p)
    return np.concatenate([w.sum(axis=1)[..., None], wp.sum(axis=1), np.einsum("bnk,bni->bki", w, q),
                           np.einsum("bnki,bnj->bkij", wp, q).reshape(VB, K, 9)], axis=2)


def finalized(mom):
    """(S (VB, K, 9), means (VB, K, 6)) fp32 numpy: rigid_finalize_kernel's float64 operations in its order — two divisions, one
    product and one difference per entry of S, then the casts."""
    with np.errstate(divide="ignore", invalid="ignore"):
        W = mom[..., :1]
        pm, qm = mom[..., 1:4] / W, mom[..., 4:7] / W
        prod = mom[..., 1:4, None] * qm[..., None, :]
        S = mom[..., 7:].reshape(mom.shape[:2] + (3, 3)) - prod
    return S.reshape(mom.shape[:2] + (9,)).astype(np.float32), np.concatenate([pm, qm], axis=2).astype(np.float32)


# ---- dynamic term: the reference ------------------------------------------------------------------------------------------------------
def fit_motion(pc1, pc2, mask):
    """losses/seg_loss_unsup.py:10-61 (the masked branch): pc (M, N, 3), mask (M, N) -> R (M, 3, 3), t (M, 3), S, valid."""
    m1 = torch.einsum("bnd,bn->bd", pc1, mask) / mask.sum(dim=1, keepdim=True)
    m2 = torch.einsum("bnd,bn->bd", pc2, mask) / mask.sum(dim=1, keepdim=True)
    c1, c2 = pc1 - m1.unsqueeze(1), pc2 - m2.unsqueeze(1)
    S = (c1 * mask.unsqueeze(2)).transpose(1, 2).bmm(c2)
    valid = ~torch.isnan(S).any(dim=1).any(dim=1)
    eye = torch.eye(3, dtype=pc1.dtype)
    R, t = eye.unsqueeze(0).repeat(len(S), 1, 1), torch.zeros(len(S), 3, dtype=pc1.dtype)
    if valid.any():
        Sv = S[valid]
        u, _, vh = torch.linalg.svd(Sv)
        v = vh.transpose(1, 2)
        diag = torch.ones_like(Sv[..., 0])
        diag[:, 2] = torch.det(v.bmm(u.transpose(1, 2)))
        Rv = v.bmm(torch.diag_embed(diag).bmm(u.transpose(1, 2)))
        Rv[(Sv == 0).all(dim=1).all(dim=1)] = eye
        R[valid] = Rv
        t[valid] = m2[valid] - Rv.bmm(m1[valid].unsqueeze(2)).squeeze(2)
    return R, t, S, valid


def blend_residual(pc, pc2, mask, R, t, p):
    """:89-97 per point: pc, pc2 (B, N, 3), mask (B, N, K), R (B * K, 3, 3), t (B * K, 3) -> (B, N), or for p = 0 the difference
    vector (B, N, 3)."""
    B, N, K = mask.shape
    moved = torch.einsum("bkij,bnj->bkni", R.view(B, K, 3, 3), pc) + t.view(B, K, 1, 3)
    diff = (mask.transpose(1, 2).unsqueeze(-1) * moved).sum(dim=1) - pc2
    return diff if p == 0 else diff.norm(p=p, dim=-1)


def dyn_reference(d, dtype, R=None, t=None):
    """The dynamic term in torch `dtype` on the host.  Keys: S, valid, R, t (per (cloud, slot), flattened); diff (B, N, 3);
    out1, out2 (B, N); g1, g2 (B, N, K) the gradients of sum(out * grad) w.r.t. the mask (the fit is detached, :91); flow
    (B, N, 3) the p = 0 form with pc2 = pc.  R, t: use these instead of the fit."""
    pc, pc2, grad = (torch.from_numpy(d[n]).to(dtype) for n in ("pc", "pc2", "grad"))
    mask = torch.from_numpy(d["mask"]).to(dtype).requires_grad_(True)
    B, N, K = mask.shape
    out = {}
    if R is None:
        flat = mask.detach().transpose(1, 2).reshape(B * K, N)
        rep = lambda x: x.unsqueeze(1).expand(B, K, N, 3).reshape(B * K, N, 3)  # noqa: E731
        R, t, out["S"], out["valid"] = fit_motion(rep(pc), rep(pc2), flat)
    out["R"], out["t"] = R, t
    for p in (1, 2):
        res = blend_residual(pc, pc2, mask, R, t, p)
        out["g%d" % p], = torch.autograd.grad((res * grad).sum(), [mask])
        out["out%d" % p] = res.detach()
    with torch.no_grad():
        out["diff"] = blend_residual(pc, pc2, mask, R, t, 0)
        out["flow"] = blend_residual(pc, pc, mask, R, t, 0)
    return out


def gate(truth, yard):
    """(Table's max-abs gate, the yardstick's own error)."""
    err = float((yard.double() - truth.double()).abs().max())
    return max(4 * err, 8 * U * float(truth.abs().max())), err


def conditioning(S):
    """(sigma2 + sign(det S) sigma3) / sigma1 per matrix, float64 torch (M, 3, 3)."""
    s = torch.linalg.svdvals(S)
    return (s[:, 1] + torch.sign(torch.det(S)) * s[:, 2]) / s[:, 0]


def identity_moves(d, ref, p):
    """(VB, K): the largest change of a row of the p-residual when that slot's (R, t) becomes the identity (float64)."""
    pc, mask = torch.from_numpy(d["pc"]).double(), torch.from_numpy(d["mask"]).double()
    B, N, K = mask.shape
    moved = torch.einsum("bkij,bnj->bkni", ref["R"].view(B, K, 3, 3), pc) + ref["t"].view(B, K, 1, 3)
    diff = ref["diff"].unsqueeze(1) - mask.transpose(1, 2).unsqueeze(-1) * (moved - pc.unsqueeze(1))
    return (diff.norm(p=p, dim=-1) - ref["out%d" % p].unsqueeze(1)).abs().max(dim=2)[0]


@functools.lru_cache(maxsize=2)
def make_dyn(c):
    """dyn_inputs(c) and: mom, S32, means32 (the exact moments and rigid_finalize_kernel's results), truth / yard
    (dyn_reference in float64 / float32), fitted (VB * K,) bool, and what the conditions measured: ratio, residual, cover."""
    d = dict(dyn_inputs(c))
    d["mom"] = moments(d)
    d["S32"], d["means32"] = finalized(d["mom"])
    truth, yard = dyn_reference(d, torch.float64), dyn_reference(d, torch.float32)
    d["truth"], d["yard"] = truth, yard
    live = torch.from_numpy(d["live"]).reshape(-1)
    d["fitted"] = live >= 2
    assert torch.equal(truth["valid"], live >= 1) and torch.equal(yard["valid"], live >= 1), case_id(c)
    d["ratio"] = float(conditioning(truth["S"][d["fitted"]]).min()) if d["fitted"].any() else float("inf")
    assert d["ratio"] >= MIN_RATIO, (case_id(c), d["ratio"])
    rows = ~torch.from_numpy(d["zero_rows"])
    d["residual"] = float(truth["diff"][rows].abs().min()) if rows.any() else float("inf")
    assert d["residual"] >= MIN_RESIDUAL, (case_id(c), d["residual"])
    assert not bool(truth["diff"][~rows].any()) and not bool(yard["diff"][~rows].any()), case_id(c)
    d["cover"] = float("inf")
    if rows.any():
        for p in (1, 2):
            g, _ = gate(truth["out%d" % p], yard["out%d" % p])
            d["cover"] = min(d["cover"], float(identity_moves(d, truth, p).reshape(-1)[live >= 1].min()) / g)
        assert d["cover"] >= COVER, (case_id(c), d["cover"])
    return d


# ---- invariance term ------------------------------------------------------------------------------------------------------------------
def used_slots(K):
    return K if K < 4 else K - K // 4


def tie_rows(N, which):
    r = np.zeros(N, bool)
    r[(7, 11)[which]::(29, 31)[which]] = True
    return r


def equal_rows(N):
    r = np.zeros(N, bool)
    r[13::23] = True
    return r & ~tie_rows(N, 0) & ~tie_rows(N, 1)


def _top(v, label, rng):
    """Raise v[i, label[i]] to 1..4 steps above the rest of its row."""
    rows = np.arange(len(v))
    v[rows, label] = -1
    v[rows, label] = v.max(axis=1) + rng.integers(1, 5, len(v))


def _ties(v, label, used, rows, rng):
    """In `rows`: a second used slot is raised to the row's maximum."""
    for i in np.flatnonzero(rows):
        others = [s for s in used if s != label[i]]
        v[i, others[rng.integers(len(others))]] = v[i, label[i]]


def first_max(v):
    """Index of the first maximum of every row, spelled out."""
    K = v.shape[-1]
    return np.where(v == v.max(axis=-1, keepdims=True), np.arange(K), K).min(axis=-1)


def confusion(a1, a2, K):
    """(PB, K, K) int64 counts of (a1, a2) pairs."""
    PB = len(a1)
    flat = (np.arange(PB)[:, None] * K + a1) * K + a2
    return np.bincount(flat.ravel(), minlength=PB * K * K).reshape(PB, K, K)


def iou_fp32(counts):
    """mask_iou_kernel's expression in numpy float32: inter / max((row + col) - inter, 1e-10)."""
    inter = counts.astype(np.float32)
    row, col = counts.sum(axis=2).astype(np.float32), counts.sum(axis=1).astype(np.float32)
    uni = (row[:, :, None] + col[:, None, :]) - inter
    out = inter / np.maximum(uni, np.float32(1e-10))
    assert out.dtype == np.float32
    return out


def assignment(score):
    """scipy's maximising assignment per matrix: (PB, K, K) -> (PB, K) int32."""
    return np.stack([linear_sum_assignment(s, maximize=True)[1] for s in score]).astype(np.int32)


def _sample(c, rng):
    N, K = c.N, c.K
    nu = used_slots(K)
    perm = np.roll(np.arange(K), 1 + rng.integers(max(K - 1, 1))) if K > 1 else np.zeros(1, int)
    label1 = rng.integers(0, nu, N)
    v1 = rng.integers(0, 24, (N, K))
    _top(v1, label1, rng)
    v2 = np.empty_like(v1)
    v2[:, perm] = np.clip(v1 + rng.integers(-2, 3, (N, K)), 0, 23)
    used2 = perm[:nu]
    label2 = np.where(rng.random(N) < 0.85, perm[label1], used2[rng.integers(0, nu, N)])
    _top(v2, label2, rng)
    if nu >= 2:
        _ties(v1, label1, list(range(nu)), tie_rows(N, 0), rng)
        _ties(v2, label2, list(used2), tie_rows(N, 1), rng)
    return v1, v2


def inv_reference(m1, m2, col12, col21, g12, g21, dtype):
    """:252-262 and :273-276 per point, torch `dtype` on the host: {p: (d12, d21, grad_mask1, grad_mask2)} for p in (1, 2); the
    permuted operands are detached."""
    out = {}
    c12, c21 = torch.from_numpy(col12).long(), torch.from_numpy(col21).long()
    for p in (1, 2):
        a = torch.from_numpy(m1).to(dtype).requires_grad_(True)
        b = torch.from_numpy(m2).to(dtype).requires_grad_(True)
        K = a.shape[2]
        t1 = torch.gather(b.detach(), 2, c12.unsqueeze(1).expand(-1, a.shape[1], K))
        t2 = torch.gather(a.detach(), 2, c21.unsqueeze(1).expand(-1, a.shape[1], K))
        d12, d21 = (a - t1).norm(p=p, dim=-1), (b - t2).norm(p=p, dim=-1)
        ga, gb = torch.autograd.grad((d12 * torch.from_numpy(g12).to(dtype)).sum() + (d21 * torch.from_numpy(g21).to(dtype)).sum(),
                                     [a, b])
        out[p] = (d12.detach(), d21.detach(), ga, gb)
    return out


@functools.lru_cache(maxsize=2)
def make_inv(c):
    """dict: mask1, mask2 (PB, N, K), g12, g21 (PB, N) — fp32 numpy; arg1, arg2 (first maxima), counts (PB, K, K) int64, iou
    fp32, col12, col21 (PB, K) int32 by scipy; truth / yard = inv_reference in float64 / float32; gap (smallest top-2 gap outside
    the tie rows, in steps of 1/64)."""
    rng = np.random.default_rng([c.seed, c.PB, c.N, c.K, 43])
    PB, N, K = c.PB, c.N, c.K
    v = [_sample(c, rng) for _ in range(PB)]
    v1, v2 = np.stack([s[0] for s in v]), np.stack([s[1] for s in v])
    eq = equal_rows(N)
    for _ in range(4):                                  # equal rows need col12, which needs the arg-maxima of the final mask2
        counts = confusion(first_max(v1), first_max(v2), K)
        col12 = assignment(iou_fp32(counts))
        want = np.take_along_axis(v2, np.broadcast_to(col12[:, None, :], v1.shape), axis=2)
        if np.array_equal(want[:, eq], v1[:, eq]):
            break
        for b in range(PB):
            v2[b][np.ix_(eq, col12[b])] = v1[b][eq]
    else:
        raise AssertionError((case_id(c), "the equal rows do not settle"))
    d = {"mask1": (v1 / 64.0).astype(np.float32), "mask2": (v2 / 64.0).astype(np.float32)}
    assert v1.max() < 64 and v2.max() < 64 and v1.min() >= 0 and v2.min() >= 0
    for name in ("g12", "g21"):
        k = rng.integers(1, 33, (PB, N)) * rng.choice([-1, 1], (PB, N))
        d[name] = (k / 16.0).astype(np.float32)
    d["arg1"], d["arg2"] = first_max(v1), first_max(v2)
    d["counts"] = confusion(d["arg1"], d["arg2"], K)
    d["iou"] = iou_fp32(d["counts"])
    d["col12"], d["col21"] = assignment(d["iou"]), assignment(d["iou"].transpose(0, 2, 1))
    assert np.array_equal(d["col12"], col12)
    d["gap"] = float("inf")
    if K > 1:
        for which, vv in ((0, v1), (1, v2)):
            top = np.sort(vv, axis=2)[..., -2:]
            gaps = top[..., 1] - top[..., 0]
            tie = tie_rows(N, which) & (used_slots(K) >= 2)
            assert not gaps[:, tie].any(), case_id(c)
            if (~tie).any():
                d["gap"] = min(d["gap"], float(gaps[:, ~tie].min()))
        assert d["gap"] >= 1, (case_id(c), d["gap"])
        assert not np.array_equal(d["col12"], np.broadcast_to(np.arange(K), (PB, K))), case_id(c)
    args = (d["mask1"], d["mask2"], d["col12"], d["col21"], d["g12"], d["g21"])
    d["truth"], d["yard"] = inv_reference(*args, torch.float64), inv_reference(*args, torch.float32)
    for p in (1, 2):
        assert not bool(d["truth"][p][0][:, eq].any()) and not bool(d["truth"][p][2][:, eq].any()), case_id(c)
    return d

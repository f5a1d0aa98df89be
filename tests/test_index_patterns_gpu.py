"""Adversarial neighbour-index tensors for the scatter / gather forms of the grouping, interpolation and smoothness-loss
gradients, with EXACT sums.

Method.  Gradient values are integers in [-4, 4] (fp32, or bf16 for the _h forms), interpolation weights come from
{1/4, 1/2, 1, 2}, relative coordinates are multiples of 1/4 in [-2, 2], the loss takes masks from {0, 1/4, 1/2} and outer
gradients that are multiples of 1/8 in [-2, 2].  index_patterns.py checks on the host, for every output element, that
sum |term| / unit < 2**24; then every partial sum in any order is exact in fp32 and each kernel — atomics, LDS images, gathers,
bf16 inputs, deterministic mode — must EQUAL the int64 np.add.at reference.  A red case is one lost, doubled or misrouted term or
a broken list, never rounding.  One randn case per entry point stays, against a float64 scatter-add under the order-free bound
|err_j| <= L_j u / (1 - L_j u) * sum |g_t| (u = 2**-24, L_j terms), so that non-integer values stay covered.

Every index tensor has two samples with different patterns (index_patterns.PARTNER), so that per-sample offsets cannot cancel.

Section 3 — ogc_group_reverse (group_reverse_kernel) and the gathers over its lists (group_bwd_rev_kernel), C = 3:
  n = 1, 512 | 513, 1025, 2049, 4097, 8193, 16384 at T = 8208     the NA = 1 / 2 / 4 / 8 / 16 / 32 points-per-thread variants of
                                                                 group_bwd_rev_kernel (16 is the last with prefetched bounds), and
                                                                 for n > 4096 the second .. fourth round (with `carry`) of the
                                                                 histogram scan of group_reverse_kernel; 16384 is the 64 KiB histogram
  T = 16, 8176, 8192, 8208, 24560 at n = 513 and 4097            one partial chunk; one group short of a chunk; exactly one; one chunk
                                                                 plus ONE group of 16 (the double-buffered fetch of a nearly empty
                                                                 chunk); three chunks with a ragged last one (8176 positions)
  interpolation form: N = 16, 2736, 5472 (T = 3 N) at m = 513, 4097, and the _bs form at channel offsets 0 and 5 of a wider tensor
  hub        one run per aligned 16 positions: the list of n - 1 is T / 16 long — one thread walks it while its wavefront waits
  two_hubs   no runs: two lists of T / 2 entries, i.e. 4096 LDS reads per chunk for two threads
  cyclic     every list as short as possible; empty lists where T < n
  sorted     runs of T / n positions that cross groups of 16 and the chunk boundary (a run is cut at both)
  ball_rows  rows of `keep` hits then copies of entry 0, keep = 1 .. S: what the searches emit
  straddle   runs of 17 .. 40 from positions = 15 (mod 16), and one over 8185 .. 8200: `heads` at group and chunk edges
  stray      5 % of -1, n, n + 7, INT32_MIN, INT32_MAX: ogc_group_reverse ignores them (both uses of an index are guarded); only
             this family sees them
Section 4 — the scatter-adds of group_bwd (ogc_group_points_grad, ogc_group_concat_grad, ogc_group_linear_bwd):
  (n, P, S) = (100, 13, 3)           group_bwd_kernel<false> (T % 4 != 0)
  n = 300, T = 4080                  group_bwd_kernel<true>, just below the LDS threshold
  T = 4096, 4112                     group_bwd_lds_kernel at and one group above its threshold (the 16th thread of 257 works alone)
  T = 16400                          two splits of 12288 positions, the second a ragged 4112
  T = 4112, (n, C) = (100, 1), (100, 3), (100, 11), (200, 5), (400, 3), (16384, 2)
                                     CC = 1 (shrunk from 8 by `cc / 2 >= c`), 4 with 3 channels, 8 with a last group of 3, 4 with a
                                     last group of 1, 2 with a last group of 1, and the 64 KiB image
  hub / two_hubs                     same-address LDS atomics from every lane; in deterministic mode det_sort_ints' heap sort
Section 5 — ogc_reverse_neighbours (rev_count / rev_scan / rev_fill / rev_sort kernels) and ogc_neighbour_consistency_bwd:
  N = 31, 32, 33 (one workgroup of nc_bwd_kernel holds 32 points), 1025 (rev_scan_kernel: two counts per thread)
  k = 1, 2, 16, 64: the row-wise ballot path of rev_count_kernel (64 = a whole wavefront per row); k = 3, 24: the generic path
  self_only (no edge at all), first_copies (every row ONE flagged edge of multiplicity k), self_first (copies of the first entry
  that are self edges: multiplicity stays 1), hub (N - 1 flagged edges on point 0), ball_rows, cyclic
Section 6 — all of it again in deterministic mode (det.hip; the sorted branches of group_reverse_kernel and rev_sort_kernel), the
  lists ascending, and ogc_group_points_grad / ogc_three_interpolate_grad with the BITS of the fp32 left-to-right sum in ascending
  position order.  The two in-place insertion sorts get hub / two_hubs only where the longest list has <= 1024 entries.
"""
import contextlib

import numpy as np
import pytest
import torch

import index_patterns as ip

gpu = pytest.mark.gpu
DEV = "cuda"
B = 2
C3 = 3


# ---- the cases ------------------------------------------------------------------------------------------------------------------
GROUP_SHAPES = [(n, 513, 16) for n in (1, 512, 513, 1025, 2049, 4097, 8193, 16384)]
GROUP_SHAPES += [(n, T // 16, 16) for n in (513, 4097) for T in (16, 8176, 8192, 24560)]
TWO_HUBS_SORT_SHAPE = (513, 128, 16)      # T = 2048: the longest list the insertion sort gets from two_hubs
INTERP_SHAPES = [(m, N) for m in (513, 4097) for N in (16, 2736, 5472)]


def _sortable(det, name, n, T):
    """May this pattern go through the in-place insertion sorts of the deterministic list builders?  (L^2 / 2 steps by one thread)"""
    if not det:
        return True
    if n == 1:
        return name == "hub"              # with one point every pattern is the hub
    return not (name == "hub" and T > 16384) and not (name == "two_hubs" and T > 2048)


def _group_params():
    out = []
    for det in (False, True):
        for n, P, S in GROUP_SHAPES:
            out += [(det, n, P, S, name) for name in ip.NAMES if _sortable(det, name, n, P * S)]
        out.append((det,) + TWO_HUBS_SORT_SHAPE + ("two_hubs",))
    return out


def _interp_params():
    return [(det, m, N, name) for det in (False, True) for m, N in INTERP_SHAPES for name in ip.NAMES
            if _sortable(det, name, m, 3 * N)]


SCATTER_NAMES = tuple(name for name in ip.NAMES if name != "stray")      # the atomic and LDS kernels require valid indices
THRESHOLD_SHAPES = [(300, T // 16, 16, C3) for T in (4080, 4096, 4112, 16400)]
SCATTER_SHAPES = THRESHOLD_SHAPES + [(100, 13, 3, C3)] + [(n, 257, 16, c) for n, c in
                                                          ((100, 1), (100, 3), (100, 11), (200, 5), (400, 3), (16384, 2))]
CONCAT_SHAPES = [(n, P, S) for n, P, S, _ in THRESHOLD_SHAPES] + [(100, 13, 3)]
LINEAR_SHAPES = [(300, T // 16, 16) for T in (4096, 4112, 16400)]         # the fused form exists on the LDS path only

NB_SHAPES = [(N, k) for N in (31, 32, 33, 1025) for k in (1, 2, 16, 64, 3, 24)]
NB_CHANNELS = (1, 7, 40)
NB_FLOAT_NAMES = ("ball_rows", "cyclic", "self_first")


def _id(v):
    return ("det" if v else "fast") if isinstance(v, bool) else str(v)


def _modes(rows):
    return [(det,) + tuple(r) for det in (False, True) for r in rows]


# ---- helpers --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nat():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    import ogc_amd  # noqa: F401  (fails loudly if libogc_ops.so is missing)
    from ogc_amd import pointnet2_cuda
    return pointnet2_cuda


@contextlib.contextmanager
def deterministic(on):
    from ogc_amd import _lib
    before = _lib.DETERMINISTIC
    _lib.set_deterministic(on)
    try:
        yield
    finally:
        _lib.set_deterministic(before)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def sentinel(*shape):
    return torch.full(shape, float("nan"), device=DEV)      # the gather kernels overwrite: nothing of this may survive


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def check_group_lists(idx, n, tc, rev, ascending):
    """The structural contract of ogc_group_reverse for idx (B, P, S): the lists of chunk ch start at ch * tc, rev_start is
    non-decreasing, every in-range run head appears exactly once and in the list of ITS point and chunk, nothing else appears, the
    `heads` bits are the host's; in deterministic mode every list is ascending."""
    nb = idx.shape[0]
    flat = idx.reshape(nb, -1)
    T = flat.shape[1]
    rs, rp, hd = rev[0].cpu().numpy(), rev[1].cpu().numpy().view(np.uint16), rev[2].cpu().numpy().view(np.uint16)
    assert rs.shape == (nb, (T + tc - 1) // tc, n + 1)
    head = ip.run_heads(flat)
    valid = head & (flat >= 0) & (flat < n)
    for b in range(nb):
        seen = []
        for ch in range(rs.shape[1]):
            r = rs[b, ch].astype(np.int64)
            assert r[0] == ch * tc and (np.diff(r) >= 0).all() and r[-1] <= min(T, (ch + 1) * tc)
            pos = ch * tc + rp[b, r[0]:r[-1]].astype(np.int64)
            assert (pos < min(T, (ch + 1) * tc)).all()
            owner = np.repeat(np.arange(n), np.diff(r))
            assert np.array_equal(flat[b][pos], owner), "a position sits in the list of another point"
            if ascending and pos.size > 1:
                inside = owner[1:] == owner[:-1]
                assert (np.diff(pos)[inside] > 0).all(), "a list is not ascending"
            seen.append(pos)
        assert np.array_equal(np.sort(np.concatenate(seen)), np.nonzero(valid[b])[0])      # every run head exactly once
        bits = (hd[b][:, None] >> np.arange(16)) & 1
        assert np.array_equal(bits.reshape(-1).astype(bool), head[b])


def check_neighbour_lists(case, rev, ascending):
    """What test_neighbour_consistency checks of ogc_reverse_neighbours, for one case of index_patterns.nb_case."""
    idx = case["idx"]
    nb, N, _ = idx.shape
    rs, src, mult = rev[0].cpu().numpy().astype(np.int64), rev[1].cpu().numpy(), rev[2].cpu().numpy()
    assert np.array_equal(mult, case["mult"])
    for b in range(nb):
        want = case["keys"][b]
        assert rs[b, 0] == 0 and rs[b, N] == want.size and (np.diff(rs[b]) >= 0).all()
        raw = src[b, :rs[b, N]]
        source, first = raw & 0x7FFFFFFF, raw < 0
        dst = np.repeat(np.arange(N), np.diff(rs[b]))
        assert np.array_equal(np.sort(ip.edge_keys(dst, source, first, N)), want)
        if ascending and raw.size > 1:
            inside = dst[1:] == dst[:-1]
            assert (np.diff(source.astype(np.int64))[inside] >= 0).all(), "a list is not ascending by source point"
    return int(sum(k.size for k in case["keys"]))


def composed(mask, idx, p):
    """losses/seg_loss_unsup.py:123-129 with torch ops (as tests/test_fused_loss_gpu.py)."""
    nb, N, C = mask.shape
    k = idx.shape[2]
    nn_mask = torch.gather(mask, 1, idx.long().reshape(nb, N * k, 1).expand(nb, N * k, C)).view(nb, N, k, C)
    return (mask.unsqueeze(2) - nn_mask).norm(p=p, dim=-1).mean(dim=-1)


# ---- 1. the generators and the host references (no GPU) ------------------------------------------------------------------------
def _runs_crossing(flat, boundary):
    """Positions p = 0 (mod boundary), p > 0, that continue the run of p - 1."""
    p = np.arange(boundary, flat.shape[0], boundary)
    return p[flat[p] == flat[p - 1]]


def test_patterns_have_the_properties_they_are_there_for():
    P, S, n = 513, 16, 100
    T = P * S
    got = dict(ip.patterns(B, P, S, n, np.random.default_rng(0)))
    assert tuple(got) == ip.NAMES
    for name, idx in got.items():
        assert idx.shape == (B, P, S) and idx.dtype == np.int32
        assert not np.array_equal(idx[0], idx[1]), "%s: the second sample repeats the first" % name
        if not name.startswith("stray"):
            assert idx.min() >= 0 and idx.max() < n
    flat = {name: idx.reshape(B, T) for name, idx in got.items()}
    # hub: one list of T entries (deterministic lists), T / 16 run heads (gather form)
    assert ip.list_lengths(flat["hub"][:1], n)[0, n - 1] == T
    assert ip.list_lengths(flat["hub"][:1], n, heads_only=True)[0].tolist() == [0] * (n - 1) + [T // 16]
    # two hubs: two lists of T / 2 and not one run to fold
    two = ip.list_lengths(flat["two_hubs"][:1], n, heads_only=True)[0]
    assert two[0] == T // 2 and two[n - 1] == T // 2 and two.sum() == T
    # cyclic: lists as even as possible, empty ones when T < n
    cyc = ip.list_lengths(flat["cyclic"][:1], n)[0]
    assert cyc.max() - cyc.min() <= 1
    assert (ip.list_lengths(ip.pattern("cyclic", B, 1, 16, n, np.random.default_rng(0)).reshape(B, 16)[:1], n)[0] == 0).sum() == n - 16
    # sorted: non-decreasing, every point present, runs over group and chunk boundaries
    s0 = flat["sorted"][0]
    assert (np.diff(s0) >= 0).all() and np.unique(s0).size == n
    assert _runs_crossing(s0, 16).size > 0 and _runs_crossing(s0, 8192).size == 1
    # straddle: runs over group boundaries, and the one over the chunk boundary inside a group on either side
    st = flat["straddle"][0]
    assert _runs_crossing(st, 16).size >= T // 64
    assert (st[8185:8201] == st[8185]).all() and st[8184] != st[8185] and st[8201] != st[8185]
    starts = np.nonzero(np.diff(st) != 0)[0] + 1
    long_runs = starts[:-1][np.diff(starts) >= 17]
    assert long_runs.size >= T // 64 and set((long_runs % 16).tolist()) <= {15, 8185 % 16}
    # stray: 3 .. 8 % out of range in either sample, every kind of stray value present
    for b in range(B):
        bad = (flat["stray"][b] < 0) | (flat["stray"][b] >= n)
        assert 0.03 <= bad.mean() <= 0.08
        assert set(flat["stray"][b][bad].tolist()) == {-1, n, n + 7, ip.INT32_MIN, ip.INT32_MAX}
    assert ip.pattern("two_hubs", B, 4, 4, 1, np.random.default_rng(0)).max() == 0       # falls back to the hub


def test_ball_rows_take_every_keep_value():
    P, S, n = 64, 16, 1000
    rows = ip.pattern("ball_rows", 1, P, S, n, np.random.default_rng(5))[0]
    rng = np.random.default_rng(5)
    hits = rng.integers(0, n, (P, S))
    keep = ip.ball_keep(P, S, rng)
    assert sorted(set(keep.tolist())) == list(range(1, S + 1))       # keep == 1 and keep == S included
    for p in range(P):
        assert np.array_equal(rows[p, :keep[p]], hits[p, :keep[p]]) and (rows[p, keep[p]:] == rows[p, 0]).all()


def test_neighbour_patterns_have_the_properties_they_are_there_for():
    N, k = 33, 16
    got = dict(ip.nb_patterns(B, N, k, np.random.default_rng(1)))
    assert tuple(got) == ip.NB_NAMES
    me = np.arange(N)[:, None]
    for name, idx in got.items():
        assert idx.shape == (B, N, k) and idx.dtype == np.int32 and idx.min() >= 0 and idx.max() < N
        assert not np.array_equal(idx[0], idx[1])
    assert (got["self_only"][0] == me).all()
    fc = got["first_copies"][0]
    assert (fc == fc[:, :1]).all() and (fc != me).all()
    sf = got["self_first"][0]
    assert (sf[:, 0] == me[:, 0]).all() and (sf[:, 1:] == me).any() and (sf[:, 1:] != me).any()
    assert (got["hub"][0] == 0).all()
    assert np.array_equal(got["cyclic"][0].reshape(-1), np.arange(N * k) % N)
    keys, mult = ip.nb_edges(got["self_only"][0])
    assert keys.size == 0 and (mult == 1).all()
    keys, mult = ip.nb_edges(got["hub"][0])
    assert np.array_equal(keys, ip.edge_keys(np.zeros(N - 1, int), np.arange(1, N), np.ones(N - 1, bool), N))
    assert mult.tolist() == [1] + [k] * (N - 1)
    keys, mult = ip.nb_edges(got["first_copies"][0])
    assert keys.size == N and (keys % 2 == 1).all() and (mult == k).all()
    keys, mult = ip.nb_edges(sf)
    assert (mult == 1).all() and (keys % 2 == 0).all()                  # the first entry is the self edge: nothing is merged


def test_host_references_agree_with_naive_loops():
    rng = np.random.default_rng(2)
    n, P, S, C = 7, 6, 8, 2
    for name, idx in ip.patterns(B, P, S, n, rng):
        terms = rng.integers(-32, 33, (B, C, P * S))
        flat = idx.reshape(B, -1)
        assert np.array_equal(ip.scatter_units(flat, terms, n), ip.scatter_naive(flat, terms, n)), name
    g, rel4 = rng.integers(-4, 5, (B, C, 48)), rng.integers(-8, 9, (B, 3, 48))
    want = [[sum(int(g[b, c, t]) * int(rel4[b, k, t]) for b in range(B) for t in range(48)) for k in range(3)] for c in range(C)]
    assert ip.dwx_units(g, rel4).tolist() == want
    N, k = 9, 4
    for name, idx in ip.nb_patterns(B, N, k, rng):
        mask4, go8 = rng.integers(0, 3, (B, N, 3)), rng.integers(-16, 17, (B, N))
        assert np.array_equal(ip.nc_grad_units(mask4, idx, go8), ip.nc_grad_naive(mask4, idx, go8)), name
        for b in range(B):      # the edge definition, as the loop of tests/test_fused_loss_gpu.py states it
            want, mult = [], []
            for i in range(N):
                row = idx[b, i]
                mult.append(1 if row[0] == i else int((row == row[0]).sum()))
                want += [(int(d) * N + i) * 2 + (j == 0) for j, d in enumerate(row) if d != i and not (j > 0 and d == row[0])]
            keys, got_mult = ip.nb_edges(idx[b])
            assert keys.tolist() == sorted(want) and got_mult.tolist() == mult, name
    with pytest.raises(AssertionError):          # the precondition is checked, not assumed
        ip.scatter_units(np.zeros((1, 4), np.int32), np.full((1, 1, 4), 2 ** 22), 1)


def test_exactness_precondition_of_the_gather_cases():
    for _, n, P, S, name in _group_params():
        ip.group_case(n, P, S, C3, name)             # asserts sum |term| / unit < 2**24 for every output element
    for _, m, N, name in _interp_params():
        ip.interp_case(m, N, C3, name)


def test_exactness_precondition_of_the_scatter_cases():
    for n, P, S, c in SCATTER_SHAPES:
        for name in SCATTER_NAMES:
            ip.group_case(n, P, S, c, name)
    for n, P, S in CONCAT_SHAPES:
        for name in SCATTER_NAMES:
            ip.group_case(n, P, S, 3 + 5, name)
    for n, P, S in LINEAR_SHAPES:
        for name in SCATTER_NAMES:
            ip.group_case(n, P, S, 5, name)


def test_exactness_precondition_of_the_loss_cases():
    for N, k in NB_SHAPES:
        if k & (k - 1) == 0:
            for name in ip.NB_NAMES:
                for c in NB_CHANNELS:
                    ip.nc_case(N, k, c, name)


# ---- 3. the grouping gradient as a gather ---------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("det,n,P,S,name", _group_params(), ids=_id)
def test_group_gradient_as_a_gather(nat, det, n, P, S, name):
    from ogc_amd import fused
    case = ip.group_case(n, P, S, C3, name)
    want = dev(ip.units_to_f32(case["ref"], 1.0))
    want_dwx = dev(ip.units_to_f32(case["dwx"], 0.25))
    g, rel = dev(case["g"]), dev(case["rel"])
    g_h = g.bfloat16()
    assert torch.equal(g_h.float(), g)
    with deterministic(det):
        rev = fused.group_reverse(dev(case["idx"]), n)
        assert rev is not None
        check_group_lists(case["idx"], n, nat.group_reverse_chunk(n, P, S), rev, ascending=det)
        got = sentinel(B, C3, n)
        nat.group_points_grad_rev_wrapper(B, C3, n, P, S, g, rev[0], rev[1], rev[2], got)
        assert torch.equal(got, want)
        got_h = sentinel(B, C3, n)
        nat.group_points_grad_rev_wrapper(B, C3, n, P, S, g_h, rev[0], rev[1], rev[2], got_h)
        assert same_bits(got_h, got)
        for grad in (g, g_h):
            gp, dwx = sentinel(B, C3, n), sentinel(C3, 3)
            nat.group_points_grad_rev_dwx_wrapper(B, C3, n, P, S, grad, rev[0], rev[1], rev[2], rel, gp, dwx)
            assert same_bits(gp, got)
            assert torch.equal(dwx, want_dwx)


@gpu
@pytest.mark.parametrize("det,m,N,name", _interp_params(), ids=_id)
def test_interpolation_gradient_as_a_gather(nat, det, m, N, name):
    from ogc_amd import fused
    case = ip.interp_case(m, N, C3, name)
    want = dev(ip.units_to_f32(case["ref"], 0.25))
    g, w = dev(case["g"]), dev(case["w"])
    wide = torch.randn(B, C3 + 5, N, device=DEV)     # what the other channels hold must not matter
    with deterministic(det):
        rev = fused.group_reverse(dev(case["idx"]), m)
        assert rev is not None
        check_group_lists(case["idx"], m, nat.group_reverse_chunk(m, N, 3), rev, ascending=det)
        got = sentinel(B, C3, m)
        nat.three_interpolate_grad_rev_wrapper(B, C3, N, m, g, w, rev[0], rev[1], rev[2], got)
        assert torch.equal(got, want)
        for off in (0, 5):                           # batch stride (C + 5) N, the slice at channel offset 0 and 5
            wide.normal_()
            wide[:, off:off + C3] = g
            sliced = sentinel(B, C3, m)
            nat.three_interpolate_grad_rev_sliced_wrapper(B, C3, N, m, wide[:, off:off + C3], w, rev[0], rev[1], rev[2], sliced)
            assert same_bits(sliced, got)


def _float_bound(flat, terms, n, extra=0):
    """float64 scatter-add of terms (B, C, T) over flat (B, T) and the order-free error bound of its fp32 evaluation."""
    nb, c, _ = terms.shape
    want, mass = np.zeros((nb, c, n)), np.zeros((nb, c, n))
    for b in range(nb):
        np.add.at(want[b].T, flat[b], terms[b].T)
        np.add.at(mass[b].T, flat[b], np.abs(terms[b]).T)
    return want, ip.order_free_bound(ip.list_lengths(flat, n)[:, None, :], mass, extra)


def _within(got, want, bound):
    err = np.abs(got.double().cpu().numpy() - want)
    assert (err <= bound).all(), "error %.3e over its bound at %s" % ((err - bound).max(), np.unravel_index((err - bound).argmax(), err.shape))


@gpu
@pytest.mark.parametrize("det", [False, True], ids=_id)
def test_gather_forms_with_float_values(nat, det):
    """One randn case per entry point of section 3 (ball_rows; n = 513 with T = 8208, m = 513 with N = 2736)."""
    from ogc_amd import fused
    n, P, S, N = 513, 513, 16, 2736
    T = P * S
    rng = np.random.default_rng(11)
    idx = ip.pattern("ball_rows", B, P, S, n, rng)
    flat = idx.reshape(B, T)
    rel = rng.standard_normal((B, 3, T)).astype(np.float32)
    g_f = torch.from_numpy(rng.standard_normal((B, C3, P, S)).astype(np.float32))
    with deterministic(det):
        rev = fused.group_reverse(dev(idx), n)
        for g in (g_f, g_f.bfloat16()):
            g64 = g.double().numpy().reshape(B, C3, T)
            want, bound = _float_bound(flat, g64, n)
            prod = np.einsum("bct,bkt->bckt", g64, rel.astype(np.float64))
            want_dwx, mass_dwx = prod.sum((0, 3)), np.abs(prod).sum((0, 3))
            got = sentinel(B, C3, n)
            nat.group_points_grad_rev_wrapper(B, C3, n, P, S, g.to(DEV), rev[0], rev[1], rev[2], got)
            _within(got, want, bound)
            gp, dwx = sentinel(B, C3, n), sentinel(C3, 3)
            nat.group_points_grad_rev_dwx_wrapper(B, C3, n, P, S, g.to(DEV), rev[0], rev[1], rev[2], dev(rel), gp, dwx)
            assert same_bits(gp, got)
            _within(dwx, want_dwx, ip.order_free_bound(np.float64(B * T), mass_dwx, extra=1))
        idx3 = ip.pattern("ball_rows", B, N, 3, n, rng)
        w = rng.random((B, N, 3)).astype(np.float32)
        gi = rng.standard_normal((B, C3, N)).astype(np.float32)
        terms = (gi.astype(np.float64)[:, :, :, None] * w.astype(np.float64)[:, None]).reshape(B, C3, 3 * N)
        want, bound = _float_bound(idx3.reshape(B, -1), terms, n, extra=1)
        rev3 = fused.group_reverse(dev(idx3), n)
        got = sentinel(B, C3, n)
        nat.three_interpolate_grad_rev_wrapper(B, C3, N, n, dev(gi), dev(w), rev3[0], rev3[1], rev3[2], got)
        _within(got, want, bound)
        wide = torch.randn(B, C3 + 5, N, device=DEV)
        wide[:, 5:] = dev(gi)
        sliced = sentinel(B, C3, n)
        nat.three_interpolate_grad_rev_sliced_wrapper(B, C3, N, n, wide[:, 5:], dev(w), rev3[0], rev3[1], rev3[2], sliced)
        _within(sliced, want, bound)


# ---- 4. the scatter-add kernels -------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", SCATTER_NAMES)
@pytest.mark.parametrize("det,n,P,S,c", _modes(SCATTER_SHAPES), ids=_id)
def test_group_points_grad_exact(nat, det, n, P, S, c, name):
    case = ip.group_case(n, P, S, c, name)
    got = torch.zeros(B, c, n, device=DEV)
    with deterministic(det):
        nat.group_points_grad_wrapper(B, c, n, P, S, dev(case["g"]), dev(case["idx"]), got)
    assert torch.equal(got, dev(ip.units_to_f32(case["ref"], 1.0)))


@gpu
@pytest.mark.parametrize("name", SCATTER_NAMES)
@pytest.mark.parametrize("det,n,P,S", _modes(CONCAT_SHAPES), ids=_id)
def test_group_concat_grad_exact(nat, det, n, P, S, name):
    c = 5
    case = ip.group_case(n, P, S, 3 + c, name)       # 3 + c channels per sample: the coordinate channels are skipped
    got = torch.zeros(B, c, n, device=DEV)
    with deterministic(det):
        nat.group_concat_grad_wrapper(B, c, n, P, S, dev(case["g"]), dev(case["idx"]), got)
    assert torch.equal(got, dev(ip.units_to_f32(case["ref"][:, 3:], 1.0)))


@gpu
@pytest.mark.parametrize("name", SCATTER_NAMES)
@pytest.mark.parametrize("det,n,P,S", _modes(LINEAR_SHAPES), ids=_id)
def test_group_linear_bwd_exact(nat, det, n, P, S, name):
    m = 5
    case = ip.group_case(n, P, S, m, name)
    grad_p, dwx = torch.zeros(B, m, n, device=DEV), torch.zeros(m, 3, device=DEV)      # both zeroed by the caller
    with deterministic(det):
        nat.group_linear_bwd_wrapper(B, m, n, P, S, dev(case["g"]), dev(case["idx"]), dev(case["rel"]), grad_p, dwx)
    assert torch.equal(grad_p, dev(ip.units_to_f32(case["ref"], 1.0)))
    assert torch.equal(dwx, dev(ip.units_to_f32(case["dwx"], 0.25)))


@gpu
@pytest.mark.parametrize("det", [False, True], ids=_id)
def test_scatter_adds_with_float_values(nat, det):
    """One randn case per entry point of section 4 (ball_rows, n = 300, T = 4112: the LDS path)."""
    n, P, S, c = 300, 257, 16, 5
    T = P * S
    rng = np.random.default_rng(12)
    idx = ip.pattern("ball_rows", B, P, S, n, rng)
    flat = idx.reshape(B, T)
    g = rng.standard_normal((B, 3 + c, P, S)).astype(np.float32)
    rel = rng.standard_normal((B, 3, T)).astype(np.float32)
    g64 = g.astype(np.float64).reshape(B, 3 + c, T)
    want, bound = _float_bound(flat, g64, n)
    with deterministic(det):
        got = torch.zeros(B, 3 + c, n, device=DEV)
        nat.group_points_grad_wrapper(B, 3 + c, n, P, S, dev(g), dev(idx), got)
        _within(got, want, bound)
        got = torch.zeros(B, c, n, device=DEV)
        nat.group_concat_grad_wrapper(B, c, n, P, S, dev(g), dev(idx), got)
        _within(got, want[:, 3:], bound[:, 3:])
        grad_p, dwx = torch.zeros(B, 3 + c, n, device=DEV), torch.zeros(3 + c, 3, device=DEV)
        nat.group_linear_bwd_wrapper(B, 3 + c, n, P, S, dev(g), dev(idx), dev(rel), grad_p, dwx)
        _within(grad_p, want, bound)
        prod = np.einsum("bct,bkt->bckt", g64, rel.astype(np.float64))
        _within(dwx, prod.sum((0, 3)), ip.order_free_bound(np.float64(B * T), np.abs(prod).sum((0, 3)), extra=1))


# ---- 5. the transposed neighbour lists of the loss ------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ip.NB_NAMES)
@pytest.mark.parametrize("det,N,k", _modes(NB_SHAPES), ids=_id)
def test_transposed_neighbour_lists_and_loss_gradient(nat, det, N, k, name):
    from ogc_amd import fused
    case = ip.nb_case(N, k, name)
    idx = dev(case["idx"])
    rowwise = k & (k - 1) == 0
    with deterministic(det):
        rev = fused.reverse_neighbours(idx)
        edges = check_neighbour_lists(case, rev, ascending=det)
        assert name != "self_only" or (case["keys"][0].size == 0 and edges == N)      # no edge at all (sample 1: first_copies)
        for c in NB_CHANNELS:
            if rowwise:                                         # p = 1, 1 / k exact: the sums are exact
                nc = ip.nc_case(N, k, c, name)
                got = sentinel(B, N, c)
                nat.neighbour_consistency_bwd_wrapper(B, N, c, k, 1, dev(nc["mask"]), idx, rev[0], rev[1], rev[2], dev(nc["go"]), got)
                assert torch.equal(got, dev(ip.units_to_f32(nc["ref"], 1.0 / (8 * k))))
                if name == "self_only":
                    assert not got[0].any()                     # nothing but self edges: an all-zero gradient
            if name in NB_FLOAT_NAMES:
                gen = torch.Generator().manual_seed(N * 100 + k + c)
                mask = torch.rand(B, N, c, generator=gen).softmax(-1)
                twin = mask[:, 1::5].clone()
                mask[:, ::5][:, :twin.shape[1]] = twin                        # equal rows: sign(0) / zero norm
                go = torch.rand(B, N, generator=gen)
                for p in ((2,) if rowwise else (1, 2)):
                    # (the composition runs on the host: the scatter of its backward would serialise on the hub of sample 1)
                    ref_mask = mask.double().requires_grad_(True)
                    (composed(ref_mask, torch.from_numpy(case["idx"]), p) * go.double()).sum().backward()
                    got = sentinel(B, N, c)
                    nat.neighbour_consistency_bwd_wrapper(B, N, c, k, p, mask.to(DEV), idx, rev[0], rev[1], rev[2], go.to(DEV), got)
                    torch.testing.assert_close(got.double().cpu(), ref_mask.grad, rtol=1e-4, atol=2e-5)


# ---- 6. deterministic mode: the order IS the definition -------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ["hub", "two_hubs", "ball_rows"])
def test_deterministic_sums_are_left_to_right_in_position_order(nat, name):
    """ogc_group_points_grad and ogc_three_interpolate_grad in deterministic mode have the bits of the fp32 sum taken left to right
    over ascending positions (np.add.at on a float32 array applies its updates one after the other, in order) — lists far above
    32 entries go through the heap sort of det_sort_ints.  n = 300; T = 4112, and 3 * 1371 = 4113 for the interpolation."""
    n, P, S, N = 300, 257, 16, 1371
    rng = np.random.default_rng(13)
    idx = ip.pattern(name, B, P, S, n, rng)
    g = rng.standard_normal((B, C3, P, S)).astype(np.float32)
    idx3 = ip.pattern(name, B, N, 3, n, rng)
    gi = rng.standard_normal((B, C3, N)).astype(np.float32)
    w = rng.random((B, N, 3)).astype(np.float32)
    want, want3 = np.zeros((B, C3, n), np.float32), np.zeros((B, C3, n), np.float32)
    for b in range(B):
        for c in range(C3):
            np.add.at(want[b, c], idx[b].reshape(-1), g[b, c].reshape(-1))
            prod = gi[b, c][:, None] * w[b]                    # the float32 product first
            assert prod.dtype == np.float32
            np.add.at(want3[b, c], idx3[b].reshape(-1), prod.reshape(-1))
    with deterministic(True):
        got = torch.zeros(B, C3, n, device=DEV)
        nat.group_points_grad_wrapper(B, C3, n, P, S, dev(g), dev(idx), got)
        got3 = torch.zeros(B, C3, n, device=DEV)
        nat.three_interpolate_grad_wrapper(B, C3, N, n, dev(gi), dev(idx3), dev(w), got3)
    assert same_bits(got, dev(want))
    assert same_bits(got3, dev(want3))

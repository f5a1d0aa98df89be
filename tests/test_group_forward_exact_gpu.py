"""The forward side of the grouping kernels, pinned at every launch-shape edge with inputs whose results are exact.

Inputs are small integers (|value| <= 8, weights in -2 .. 2): every product and every sum is exact in fp32, the largest output
(3 * 2 * 16 + 4 * 2 * 8 = 160 < 256) is exact in bf16, the fp32 partial sums of squares stay below 2^24 and the fp64 statistics are
exact whatever the order of their atomics.  So every assertion is EQUALITY against numpy.  Outputs are pre-filled with NaN between
two guard bands that must come back untouched.  (The backward side: tests/test_index_patterns_gpu.py.)"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 64   # floats (16-bit elements: twice as many bytes would do; the band is in elements), a multiple of 4: keeps the alignment
DEV = "cuda:0"


@pytest.fixture(scope="module")
def nat():
    from ogc_amd import pointnet2_cuda
    global SLOTS
    SLOTS = pointnet2_cuda.conv1x1_gn_slots()  # copies of the statistics accumulator (GL_SLOTS)
    return pointnet2_cuda


SLOTS = None


def _ints(rng, shape, lim):
    return rng.integers(-lim, lim + 1, size=shape).astype(np.float32)


def _guarded(count, dtype=torch.float32, offset=0):
    """(whole buffer, the view of `count` elements the kernel writes): NaN everywhere, `offset` elements past the aligned start"""
    buf = torch.full((GUARD + offset + count + GUARD,), float("nan"), dtype=dtype, device=DEV)
    return buf, buf[GUARD + offset:GUARD + offset + count]


def _check_guarded(buf, count, want, offset=0):
    got = buf.float().cpu().numpy()
    assert np.isnan(got[:GUARD + offset]).all() and np.isnan(got[GUARD + offset + count:]).all(), "guard band written"
    body = got[GUARD + offset:GUARD + offset + count]
    assert not np.isnan(body).any(), "output element left unwritten"
    assert np.array_equal(body, want.reshape(-1))


def _scene(seed, b, n, npoints, nsample):
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, n, size=(b, npoints, nsample)).astype(np.int32)
    idx[:, :, nsample // 2:] = idx[:, :, :1]  # rows end in runs of one index, as ball-query and clamped kNN rows do
    xyz = _ints(rng, (b, n, 3), 8)
    new_xyz = _ints(rng, (b, npoints, 3), 8)
    return rng, idx, xyz, new_xyz


def _rel(idx, xyz, new_xyz):
    b = idx.shape[0]
    g = np.stack([xyz[i][idx[i]] for i in range(b)])            # (b, npoints, nsample, 3)
    return np.ascontiguousarray((g - new_xyz[:, :, None, :]).transpose(0, 3, 1, 2))  # (b, 3, npoints, nsample)


def _gather(points, idx):
    b = idx.shape[0]
    return np.stack([points[i][:, idx[i]] for i in range(b)])   # (b, c, npoints, nsample)


# (b, c, n, npoints, nsample, offset): T = 1, 1020, 1024, 1028 (4-wide), 1023 (scalar), 1024 with `out` 4 bytes off (scalar by
# misalignment), and 255 channels at T = 8192 where a workgroup takes 2 channels and the last one a single channel
GATHER_CASES = [(2, 5, 37, 1, 1, 0), (2, 5, 37, 255, 4, 0), (2, 5, 37, 256, 4, 0), (2, 5, 37, 257, 4, 0), (2, 5, 37, 341, 3, 0),
                (2, 5, 37, 256, 4, 1), (2, 255, 512, 512, 16, 0)]


@pytest.mark.parametrize("b,c,n,npoints,nsample,offset", GATHER_CASES)
def test_group_points_gather_points_group_concat(nat, b, c, n, npoints, nsample, offset):
    T = npoints * nsample
    rng, idx, xyz, new_xyz = _scene(T + c, b, n, npoints, nsample)
    points = _ints(rng, (b, c, n), 8)
    want = _gather(points, idx)
    d = lambda a: torch.from_numpy(a).to(DEV)
    idx_d, points_d = d(idx), d(points)
    buf, out = _guarded(b * c * T, offset=offset)
    nat.group_points_wrapper(b, c, n, npoints, nsample, points_d, idx_d, out)
    _check_guarded(buf, b * c * T, want, offset)
    buf, out = _guarded(b * c * T, offset=offset)  # gather_points: the same kernel with nsample = 1
    nat.gather_points_wrapper(b, c, n, T, points_d, idx_d, out)
    _check_guarded(buf, b * c * T, want, offset)
    buf, out = _guarded(b * (3 + c) * T, offset=offset)
    nat.group_concat_wrapper(b, c, n, npoints, nsample, d(xyz), d(new_xyz), points_d, idx_d, out)
    _check_guarded(buf, b * (3 + c) * T, np.concatenate([_rel(idx, xyz, new_xyz), want], axis=1), offset)


@pytest.mark.parametrize("npoints,nsample,offset", [(1, 1, 0), (256, 4, 0), (341, 3, 0), (256, 4, 1)])
def test_group_concat_without_features(nat, npoints, nsample, offset):
    """c = 0: the coordinate rows alone (group_xyz_rel_kernel, the two-launch fallback)"""
    b, n, T = 2, 37, npoints * nsample
    rng, idx, xyz, new_xyz = _scene(T, b, n, npoints, nsample)
    d = lambda a: torch.from_numpy(a).to(DEV)
    buf, out = _guarded(b * 3 * T, offset=offset)
    nat.group_concat_wrapper(b, 0, n, npoints, nsample, d(xyz), d(new_xyz), None, d(idx), out)
    _check_guarded(buf, b * 3 * T, _rel(idx, xyz, new_xyz), offset)


def _stats_of(y, groups):
    b, m = y.shape[:2]
    v = y.astype(np.float64).reshape(b, groups, -1)
    return np.stack([v.sum(-1), (v * v).sum(-1)], axis=-1)      # (b, groups, 2)


def _run_linear(nat, form, bf16, b, m, n, npoints, nsample, groups, src, idx, rel, w):
    """form: "fwd" | "direct" | "pt"; returns (y as float32 numpy, summed statistics or None) after the guard checks"""
    T = npoints * nsample
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    buf, y = _guarded(b * m * T, torch.bfloat16 if bf16 else torch.float32)
    sbuf, stats = (None, None)
    if groups:
        sbuf, stats = _guarded(SLOTS * b * groups * 2, torch.float64)
    if form == "fwd":
        nat.group_linear_fwd_wrapper(b, m, n, npoints, nsample, groups, d(src), d(idx), d(rel), d(w), y, stats)
    elif form == "direct":
        nat.group_linear_fwd_direct_wrapper(b, m, src.shape[1], n, npoints, nsample, groups, d(src), d(idx), d(rel), d(w), y, stats)
    else:
        nat.group_linear_fwd_pt_wrapper(b, m, n, npoints, nsample, groups, d(src.transpose(0, 2, 1)), d(idx), d(rel), d(w), y, stats)
    got = buf.float().cpu().numpy()
    assert np.isnan(got[:GUARD]).all() and np.isnan(got[GUARD + b * m * T:]).all(), "guard band of y written"
    st = None
    if groups:
        s = sbuf.cpu().numpy()
        assert np.isnan(s[:GUARD]).all() and np.isnan(s[GUARD + SLOTS * b * groups * 2:]).all(), "guard band of stats written"
        st = s[GUARD:GUARD + SLOTS * b * groups * 2].reshape(SLOTS, b, groups, 2).sum(0)
    return got[GUARD:GUARD + b * m * T].reshape(b, m, npoints, nsample), st


# T = 4, 1024, 1028 and 17412 (blockIdx.x wraps the 16 slots: 17 workgroups of 1024 positions)
LINEAR_T = [(1, 4), (256, 4), (257, 4), (4353, 4)]
LINEAR_MG = [(16, 0), (16, 16), (48, 1), (32, 4)]


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("npoints,nsample", LINEAR_T)
def test_group_linear_fwd_and_direct(nat, bf16, npoints, nsample):
    b, n = 2, 96
    rng, idx, xyz, new_xyz = _scene(npoints, b, n, npoints, nsample)
    rel = _rel(idx, xyz, new_xyz)
    for m, groups in LINEAR_MG:
        P = _ints(rng, (b, m, n), 8)
        wx = _ints(rng, (m, 3), 2)
        want = _gather(P, idx) + np.einsum("mk,bkps->bmps", wx, rel)
        y, st = _run_linear(nat, "fwd", bf16, b, m, n, npoints, nsample, groups, P, idx, rel, wx)
        assert np.array_equal(y, want), ("fwd", m, groups)
        if groups:
            assert np.array_equal(st, _stats_of(want, groups)), ("fwd stats", m, groups)
        for cf in (1, 2, 3, 4):
            feats = _ints(rng, (b, cf, n), 8)
            w = _ints(rng, (m, 3 + cf), 2)
            want = np.einsum("mk,bkps->bmps", w[:, :3], rel) + np.einsum("mk,bkps->bmps", w[:, 3:], _gather(feats, idx))
            y, st = _run_linear(nat, "direct", bf16, b, m, n, npoints, nsample, groups, feats, idx, rel, w)
            assert np.array_equal(y, want), ("direct", cf, m, groups)
            if groups:
                assert np.array_equal(st, _stats_of(want, groups)), ("direct stats", cf, m, groups)


# T = 2, 2046, 2050 and 34818 (a workgroup takes 2048 positions: 18 workgroups wrap the 16 slots), which the channel-major form
# refuses (T % 4), and 4, 2048, 2052 and 34820, which both forms take: there the two must give the same y bits
@pytest.mark.parametrize("npoints,nsample", [(1, 2), (1023, 2), (1025, 2), (17409, 2), (2, 2), (1024, 2), (1026, 2), (17410, 2)])
def test_group_linear_fwd_pt_h(nat, npoints, nsample):
    b, n = 2, 96
    rng, idx, xyz, new_xyz = _scene(npoints, b, n, npoints, nsample)
    rel = _rel(idx, xyz, new_xyz)
    T = npoints * nsample
    compared = 0
    for m, groups in [(64, 0), (64, 4), (64, 2), (64, 1), (128, 0), (128, 8), (128, 4), (128, 2)]:  # m / groups in {16, 32, 64}
        P = _ints(rng, (b, m, n), 8)
        wx = _ints(rng, (m, 3), 2)
        want = _gather(P, idx) + np.einsum("mk,bkps->bmps", wx, rel)
        y, st = _run_linear(nat, "pt", True, b, m, n, npoints, nsample, groups, P, idx, rel, wx)
        assert np.array_equal(y, want), ("pt", m, groups)
        if groups:
            assert np.array_equal(st, _stats_of(want, groups)), ("pt stats", m, groups)
        if T % 4 == 0:  # the channel-major form gives the same bits and the same statistics
            y2, st2 = _run_linear(nat, "fwd", True, b, m, n, npoints, nsample, groups, P, idx, rel, wx)
            assert np.array_equal(y2.view(np.uint32), y.view(np.uint32)), ("pt against fwd_h", m, groups)
            if groups:
                assert np.array_equal(st2, st), ("pt against fwd_h stats", m, groups)
            compared += 1
    assert compared == (8 if T % 4 == 0 else 0)


def test_first_layer_refusals(nat):
    from ogc_amd._lib import OgcOpsError
    b, n, m = 1, 8, 64
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)

    def refused(fn, *args):
        with pytest.raises(OgcOpsError, match=r"status -3"):
            fn(*args)

    for bf16 in (False, True):
        dt = torch.bfloat16 if bf16 else torch.float32
        for T, groups, yoff in ((6, 4, 0), (8, 4, 1), (8, 3, 0)):  # T % 4, misaligned y, m % groups
            idx, rel, st = z(b, T, dt=torch.int32), z(b, 3, T), z(SLOTS * b * max(groups, 1) * 2, dt=torch.float64)
            y = z(b * m * T + 8, dt=dt)[yoff:yoff + b * m * T]
            refused(nat.group_linear_fwd_wrapper, b, m, n, T, 1, groups, z(b, m, n), idx, rel, z(m, 3), y, st)
            refused(nat.group_linear_fwd_direct_wrapper, b, m, 3, n, T, 1, groups, z(b, 3, n), idx, rel, z(m, 6), y, st)
    # the point-major form: odd T, m % 64, a group width outside {16, 32, 64}, misaligned y
    for T, mm, groups, yoff in ((7, 64, 4, 0), (8, 32, 2, 0), (8, 64, 8, 0), (8, 64, 3, 0), (8, 64, 4, 1)):
        idx, rel, st = z(b, T, dt=torch.int32), z(b, 3, T), z(SLOTS * b * groups * 2, dt=torch.float64)
        y = z(b * mm * T + 8, dt=torch.bfloat16)[yoff:yoff + b * mm * T]
        refused(nat.group_linear_fwd_pt_wrapper, b, mm, n, T, 1, groups, z(b, n, mm), idx, rel, z(mm, 3), y, st)

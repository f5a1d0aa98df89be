"""ogc_kittisf_unproject (ogc_amd/csrc/kittisf_prepare.hip) through ogc_amd/data_prepare/scan_ops.py::kittisf_unproject and the
raw wrapper.

The per-pixel arithmetic is float32 with one rounding per operation, and the generator of tests/golden/kittisf_prepare.npz found
the reference's own functions and this repository's mirror of them equal in every bit, so count, keep_idx, both clouds and the
labels must EQUAL the fixture and the mirror on any input: no tolerance, no excluded pixels.  Every run writes into buffers with
sentinels behind row M and behind the buffers' ends."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL_F, SENTINEL_I, GUARD = -12345.5, -77, 64
LABEL_IDS = (0, 6656, 6911, 6912, 7168, 7199, 7200, 7423, 7424, 65535)


@pytest.fixture(scope="module")
def mirror():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_kittisf_prepare_golden
    return make_kittisf_prepare_golden


@pytest.fixture(scope="module")
def golden():
    data = np.load(os.path.join(HERE, "golden", "kittisf_prepare.npz"))
    return data, json.loads(str(data["meta"]))


def tile():
    """OGC_SCAN_CROP_TILE as the library reports it: the pixels per workgroup of the unprojection kernels."""
    from ogc_amd import _lib
    from ogc_amd.data_prepare.scan_ops import SCAN_CROP_TILE
    t = _lib.load().ogc_scan_crop_tile()
    assert t == SCAN_CROP_TILE
    return t


def upload(array):
    from ogc_amd.pointnet2_cuda import U16
    return torch.from_numpy(np.ascontiguousarray(array).view(np.int16)).cuda().view(U16)


def run_guarded(maps, P, select=(26, 28), depth_thresh=35.0):
    """The raw entry point on sentinel-filled buffers -> (pc1, pc2, segm int64, keep_idx) numpy, after the checks of the memory
    contract: rows >= M and the guard behind every buffer untouched."""
    from ogc_amd import pointnet2_cuda as nat
    height, width = maps[0].shape
    n = height * width
    pc1 = torch.full((n * 3 + GUARD,), SENTINEL_F, dtype=torch.float32, device="cuda")
    pc2 = torch.full((n * 3 + GUARD,), SENTINEL_F, dtype=torch.float32, device="cuda")
    segm = torch.full((n + GUARD,), SENTINEL_I, dtype=torch.int32, device="cuda")
    keep_idx = torch.full((n + GUARD,), SENTINEL_I, dtype=torch.int32, device="cuda")
    count = torch.full((1 + GUARD,), SENTINEL_I, dtype=torch.int32, device="cuda")
    sel = torch.tensor(list(select) + [SENTINEL_I] * GUARD, dtype=torch.int32, device="cuda")
    nat.kittisf_unproject_wrapper(height, width, *(upload(m) for m in maps), np.float32(P[0, 0] * 0.54), P[0, 0], P[0, 2], P[0, 3],
                                  P[1, 2], P[1, 3], P[2, 3], depth_thresh,
                                  sel[:max(len(select), 1)], len(select), pc1[:n * 3].view(n, 3), pc2[:n * 3].view(n, 3), segm[:n],
                                  keep_idx[:n], count[:1])
    m = int(count[0].item())
    assert 0 <= m <= n
    for buf, per_row, sentinel in ((pc1, 3, SENTINEL_F), (pc2, 3, SENTINEL_F), (segm, 1, SENTINEL_I), (keep_idx, 1, SENTINEL_I)):
        assert bool((buf[m * per_row:] == sentinel).all())
    assert bool((count[1:] == SENTINEL_I).all()) and bool((sel[len(select):] == SENTINEL_I).all())
    return (pc1[:m * 3].view(m, 3).cpu().numpy(), pc2[:m * 3].view(m, 3).cpu().numpy(), segm[:m].cpu().numpy().astype(np.int64),
            keep_idx[:m].cpu().numpy())


def assert_equal_frames(got, want):
    assert got[3].shape == want[3].shape, (got[3].shape, want[3].shape)
    assert got[3].dtype == np.int32 and np.array_equal(got[3], want[3])
    assert (np.diff(got[3]) > 0).all()                                   # pixel order
    for k in (0, 1):
        assert got[k].dtype == np.float32 and np.array_equal(got[k].view(np.int32), want[k].view(np.int32))
    assert np.array_equal(got[2], want[2])


def draw(height, width, seed):
    from ogc_amd.utils.synthetic import make_kittisf_maps
    return make_kittisf_maps(height, width, np.random.RandomState(seed))


@pytest.mark.parametrize("name", ("a", "b"))
def test_equals_the_fixture(golden, name):
    from ogc_amd.data_prepare.scan_ops import kittisf_unproject
    data, meta = golden
    maps = [data["%s_%s" % (name, k)] for k in ("disp1", "disp2", "flow", "inst")]
    want = tuple(data["%s_%s" % (name, k)] for k in ("pc1", "pc2", "segm", "keep_idx"))
    assert_equal_frames(run_guarded(maps, data["P_rect"]), want)
    out = kittisf_unproject(*(upload(m) for m in maps), data["P_rect"])
    assert all(t.is_cuda for t in out) and [t.dtype for t in out] == [torch.float32, torch.float32, torch.int32, torch.int32]
    assert out[0].shape == (meta["cases"][name]["kept"], 3)
    assert_equal_frames((out[0].cpu().numpy(), out[1].cpu().numpy(), out[2].cpu().numpy().astype(np.int64), out[3].cpu().numpy()), want)


def shapes():
    t = tile()
    assert t == 1024
    return [(1, 1), (1, 63), (1, 65), (3, 341), (32, 32), (25, 41), (7, 293), (13, 401), (401, 13)]


@pytest.mark.parametrize("k", range(9))
def test_equals_the_mirror_at_every_shape(mirror, k):
    height, width = shapes()[k]
    t = tile()
    assert [h * w for h, w in shapes()] == [1, 63, 65, t - 1, t, t + 1, 2 * t + 3, 5 * t + 93, 5 * t + 93]
    maps = draw(height, width, 200 + k)
    P = mirror.p_rect()
    want = mirror.unproject_mirror(*maps, P)
    assert height * width < 63 or 0 < want[3].shape[0] < height * width
    assert_equal_frames(run_guarded(maps, P), want)


PATTERNS = ("none", "all", "first", "last", "tile_ends", "alternating", "middle_tile_dropped")
CAUSES = ("d1_zero", "d2_zero", "flag_0", "flag_2", "z1_far", "z2_far")


@pytest.mark.parametrize("pattern", PATTERNS)
def test_keep_patterns_by_every_cause(mirror, pattern):
    t = tile()
    height, width = 7, 293
    n = height * width
    assert n == 2 * t + 3
    i = np.arange(n)
    keep = {"none": np.zeros(n, bool), "all": np.ones(n, bool), "first": i == 0, "last": i == n - 1,
            "tile_ends": (i % t == t - 1) | (i % t == 0), "alternating": i % 2 == 0,
            "middle_tile_dropped": (i < t) | (i >= 2 * t)}[pattern].reshape(height, width)
    P = mirror.p_rect()
    rs = np.random.RandomState(17)
    for cause in CAUSES:
        # every pixel passes every test (depths of 8.3 .. 25 m), then the cause alone drops the others (2000 raw: 49.9 m)
        disp1, disp2 = rs.randint(4000, 12001, size=(2, height, width))
        flow = np.stack([32768 + rs.randint(-640, 641, size=(height, width)), 32768 + rs.randint(-640, 641, size=(height, width)),
                         np.ones((height, width), dtype=np.int64)], 2)
        inst = np.asarray([0, 6657, 7169, 6145])[rs.randint(0, 4, size=(height, width))]
        if cause == "d1_zero":
            disp1[~keep] = 0
        elif cause == "d2_zero":
            disp2[~keep] = 0
        elif cause == "flag_0":
            flow[~keep, 2] = 0
        elif cause == "flag_2":
            flow[~keep, 2] = 2
        elif cause == "z1_far":
            disp1[~keep] = 2000
        else:
            disp2[~keep] = 2000
        maps = [a.astype(np.uint16) for a in (disp1, disp2, flow, inst)]
        want = mirror.unproject_mirror(*maps, P)
        assert np.array_equal(want[3], np.nonzero(keep.reshape(-1))[0]), cause     # the cause decides alone
        assert_equal_frames(run_guarded(maps, P), want)


def test_the_threshold_is_strict_and_an_argument(mirror):
    maps = draw(7, 293, 31)
    P = mirror.p_rect()
    _, pc1, pc2 = mirror.unproject_points(maps[0], maps[1], maps[2], P)
    kept35 = mirror.unproject_mirror(*maps, P)[3]
    for cloud in (pc1, pc2):
        thresh = float(cloud.reshape(-1, 3)[kept35[kept35.shape[0] // 2], 2])     # the depth of a kept pixel, exactly
        want = mirror.unproject_mirror(*maps, P, depth_thresh=thresh)
        assert 0 < want[3].shape[0] < kept35.shape[0] and kept35[kept35.shape[0] // 2] not in want[3].tolist()
        assert_equal_frames(run_guarded(maps, P, depth_thresh=thresh), want)


def label_frame(ids, seed, height=7, width=293):
    """Every pixel kept, ids drawn from `ids`."""
    rs = np.random.RandomState(seed)
    disp1, disp2 = rs.randint(4000, 12001, size=(2, height, width))
    flow = np.stack([np.full((height, width), 32768), np.full((height, width), 32768), np.ones((height, width), dtype=np.int64)], 2)
    inst = np.asarray(ids)[rs.randint(0, len(ids), size=(height, width))]
    return [a.astype(np.uint16) for a in (disp1, disp2, flow, inst)]


def test_labels_at_the_edges_of_semantics_and_table_words(mirror):
    P = mirror.p_rect()
    maps = label_frame(LABEL_IDS, 5)
    assert set(maps[3].reshape(-1).tolist()) == set(LABEL_IDS)
    want = mirror.unproject_mirror(*maps, P)
    expected = {6656: 1, 6911: 2, 7168: 3, 7199: 4, 7200: 5, 7423: 6}     # 6912 is semantic 27, 7424 is 29
    assert np.array_equal(want[2], np.array([expected.get(i, 0) for i in maps[3].reshape(-1).tolist()]))
    assert_equal_frames(run_guarded(maps, P), want)
    # other selections: none; the first and the last semantic (id 0 is an id of semantic 0 like any other)
    want = mirror.unproject_mirror(*maps, P, select_semantics=())
    assert not want[2].any()
    assert_equal_frames(run_guarded(maps, P, select=()), want)
    want = mirror.unproject_mirror(*maps, P, select_semantics=(0, 255))
    assert set(want[2].tolist()) == {0, 1, 2} and (want[2][maps[3].reshape(-1) == 0] == 1).all() and (want[2][maps[3].reshape(-1) == 65535] == 2).all()
    assert_equal_frames(run_guarded(maps, P, select=(0, 255)), want)
    # a repeated and an out-of-range value in the list change nothing
    assert_equal_frames(run_guarded(maps, P, select=(28, 26, 26, 300, -1)), mirror.unproject_mirror(*maps, P))


def test_an_id_on_dropped_pixels_only_takes_no_number(mirror):
    P = mirror.p_rect()
    maps = label_frame((0, 6700, 7168, 7300), 6)
    gone = maps[3] == 7168
    assert gone.any() and (~gone).any()
    maps[0][gone] = 0                                                    # every pixel of id 7168 has no disparity
    want = mirror.unproject_mirror(*maps, P)
    assert set(want[2].tolist()) == {0, 1, 2} and (want[2][maps[3][~gone] == 7300] == 2).all()
    assert_equal_frames(run_guarded(maps, P), want)


def test_more_than_64_selected_ids(mirror):
    P = mirror.p_rect()
    ids = [26 * 256 + k for k in range(0, 256, 3)] + [28 * 256 + k for k in range(1, 256, 5)] + [27 * 256 + k for k in range(40)] + [0]
    maps = label_frame(ids, 7, height=13, width=401)
    want = mirror.unproject_mirror(*maps, P)
    assert want[2].max() == 86 + 51 and len(set(want[2].tolist())) == 86 + 51 + 1
    assert_equal_frames(run_guarded(maps, P), want)


def test_the_frame_size(mirror):
    maps = draw(375, 1242, 9)
    P = mirror.p_rect()
    want = mirror.unproject_mirror(*maps, P)
    assert 100000 < want[3].shape[0] < 300000
    assert_equal_frames(run_guarded(maps, P), want)


def test_two_calls_give_the_same_bits(mirror):
    maps = draw(13, 401, 41)
    a, b = run_guarded(maps, mirror.p_rect()), run_guarded(maps, mirror.p_rect())
    assert_equal_frames(a, b)


def test_an_empty_image_writes_count(mirror):
    P = mirror.p_rect()
    for shape in ((0, 5), (5, 0)):
        maps = [np.zeros(shape, np.uint16), np.zeros(shape, np.uint16), np.zeros(shape + (3,), np.uint16), np.zeros(shape, np.uint16)]
        got = run_guarded(maps, P)
        assert got[3].shape == (0,)


def test_bad_inputs_raise(mirror):
    from ogc_amd import pointnet2_cuda as nat
    from ogc_amd.data_prepare.scan_ops import kittisf_unproject
    P = mirror.p_rect()
    maps = [upload(m) for m in draw(16, 24, 1)]
    with pytest.raises(RuntimeError):
        kittisf_unproject(maps[0].repeat(1, 2)[:, :24], *maps[1:], P)    # a view with a row stride of 48
    with pytest.raises(ValueError):
        kittisf_unproject(maps[0], maps[1][:8].contiguous(), maps[2], maps[3], P)
    with pytest.raises(ValueError):
        kittisf_unproject(maps[0], maps[1], maps[2][..., :2].contiguous(), maps[3], P)
    with pytest.raises(TypeError):
        kittisf_unproject(maps[0], maps[1], maps[2], maps[3].to(torch.int32), P)
    with pytest.raises(ValueError):
        kittisf_unproject(*maps, P.astype(np.float64))
    for r, c in ((0, 1), (1, 0), (2, 0), (2, 1), (1, 1)):
        bad = P.copy()
        bad[r, c] += 1.0
        with pytest.raises(ValueError):
            kittisf_unproject(*maps, bad)
    with pytest.raises(ValueError):
        kittisf_unproject(*maps, P, select_semantics=range(257))
    # the C ABI's own checks
    n = 16 * 24
    out = (torch.empty(n, 3, device="cuda"), torch.empty(n, 3, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda"),
           torch.empty(n, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"))
    sel = torch.zeros(300, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="n_select"):
        nat.kittisf_unproject_wrapper(16, 24, *maps, 389.0, 721.0, 609.0, 44.0, 172.0, 0.2, 0.003, 35.0, sel, 257, *out)
    with pytest.raises(RuntimeError, match="32-bit indexing"):
        nat.kittisf_unproject_wrapper(65536, 65536, *maps, 389.0, 721.0, 609.0, 44.0, 172.0, 0.2, 0.003, 35.0, sel, 2, *out)

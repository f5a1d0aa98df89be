"""ogc_scan_crop_front / ogc_scan_crop_camera (ogc_amd/csrc/scan_prepare.hip) through ogc_amd/data_prepare/scan_ops.py.

The front predicate is all float32 with one rounding per operation, so count, keep_idx and out_pc must EQUAL numpy's on any
input, with no exclusions.  The camera predicate is compared with tests/golden/scan_prepare.npz, whose inputs the generator
chose so that equality is a fair demand (margins in its metadata), and with the generator's float64 mirror on a frame drawn here
under the same conditions."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL_F, SENTINEL_I, GUARD = -12345.5, -77, 64


@pytest.fixture(scope="module")
def mirror():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_scan_prepare_golden
    return make_scan_prepare_golden


@pytest.fixture(scope="module")
def golden():
    data = np.load(os.path.join(HERE, "golden", "scan_prepare.npz"))
    return data, json.loads(str(data["meta"]))


def waymo_frame(n, seed, keep=None):
    """(n, 6) float32: points that pass every range test when `keep` is given (column 5 then decides alone), else a mixture
    around every threshold."""
    rs = np.random.RandomState(seed)
    if keep is None:
        scan = np.stack([-20.0 + 90.0 * rs.rand(n), (rs.rand(n) - 0.5) * 130.0, -3.0 + 8.0 * rs.rand(n), rs.rand(n), rs.rand(n),
                         np.where(rs.rand(n) < 0.15, rs.randint(0, 2, size=n), -1)], 1)
    else:
        x = 2.0 + 30.0 * rs.rand(n)
        scan = np.stack([x, x * (rs.rand(n) - 0.5) * 1.8, -2.0 + 3.0 * rs.rand(n), rs.rand(n), rs.rand(n),
                         np.where(np.asarray(keep, dtype=bool), -1.0, 0.0)], 1)
    return scan.astype(np.float32)


def run_front(scan):
    from ogc_amd.data_prepare.scan_ops import crop_front
    pc, idx = crop_front(torch.from_numpy(scan).cuda())
    assert pc.is_cuda and idx.is_cuda and pc.dtype == torch.float32 and idx.dtype == torch.int32
    return pc.cpu().numpy(), idx.cpu().numpy()


def assert_equal_crop(got, want):
    assert got[1].shape == want[1].shape, (got[1].shape, want[1].shape)
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[0].view(np.int32), want[0].view(np.int32))
    assert (np.diff(got[1]) > 0).all()                                   # scan order


def sizes():
    from ogc_amd.pointnet2_cuda import SCAN_CROP_TILE as T
    return [0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, 5 * T + 17]


@pytest.mark.parametrize("k", range(10))
def test_front_equals_numpy_at_every_size(mirror, k):
    n = sizes()[k]
    scan = waymo_frame(n, 100 + k).reshape(n, 6)
    want = mirror.crop_front_mirror(scan)
    assert n < 64 or 0 < want[1].shape[0] < n
    assert_equal_crop(run_front(scan), want)


PATTERNS = ("none", "all", "first", "last", "tile_ends", "alternating", "middle_tile_dropped")


@pytest.mark.parametrize("pattern", PATTERNS)
def test_front_keep_patterns(mirror, pattern):
    from ogc_amd.pointnet2_cuda import SCAN_CROP_TILE as T
    n = 3 * T + 5
    i = np.arange(n)
    keep = {"none": np.zeros(n, bool), "all": np.ones(n, bool), "first": i == 0, "last": i == n - 1, "tile_ends": i % T == T - 1,
            "alternating": i % 2 == 0, "middle_tile_dropped": (i < T) | (i >= 2 * T)}[pattern]
    scan = waymo_frame(n, 7, keep=keep)
    want = mirror.crop_front_mirror(scan)
    assert np.array_equal(want[1], np.nonzero(keep)[0])                  # the range tests pass everywhere: column 5 decides
    assert_equal_crop(run_front(scan), want)


def test_front_every_comparison_rejects(mirror):
    """Rows that exactly one comparison rejects, for the four comparisons that can reject alone — |y| < 50 cannot: x > |y| and
    x < 35 imply it — and rows at and next to every threshold, NaN and inf among them."""
    f = np.float32
    up, down = (lambda v: np.nextafter(f(v), f(np.inf))), (lambda v: np.nextafter(f(v), f(-np.inf)))
    rows = [[10, 1, 0, -1], [10, 1, 0, 0], [10, 1, 0, 1], [10, 1, 0, down(-1)],          # flag
            [1, 2, 0, -1], [2, 2, 0, -1], [2, -2, 0, -1], [up(2), -2, 0, -1],               # x > |y|
            [34, 1, 50, -1], [0, 0, 60, -1], [30, 20, f(np.sqrt(2300.0)), -1], [30, 20, 47.9, -1],   # the range
            [35, 0, 0, -1], [down(35), 0, 0, -1], [up(35), 0, 0, -1],                       # x < 35
            [60, 55, 0, -1], [60, 50, 0, -1], [60, down(50), 0, -1], [70, -50, 0, -1],      # |y| < 50 (with others)
            [np.nan, 0, 0, -1], [10, np.nan, 0, -1], [10, 0, np.nan, -1], [10, 0, 0, np.nan], [np.inf, 0, 0, -1], [10, 0, np.inf, -1],
            [-0.0, 0.0, 0, -1], [0, 0, 0, -1]]
    scan = np.array([[r[0], r[1], r[2], 0.5, 0.5, r[3]] for r in rows], dtype=np.float32)
    x, y, z, flag = scan[:, 0], scan[:, 1], scan[:, 2], scan[:, 5]
    with np.errstate(all="ignore"):
        tests = np.stack([flag == -1, x > abs(y), (np.square(x) + np.square(y) + np.square(z)) < 3600, abs(y) < 50, x < 35], 1)
    alone = [int(((~tests[:, c]) & tests[:, [d for d in range(5) if d != c]].all(1)).sum()) for c in range(5)]
    assert all(a >= 1 for c, a in enumerate(alone) if c != 3) and alone[3] == 0 and (~tests[:, 3]).sum() >= 3
    want = mirror.crop_front_mirror(scan)
    assert np.array_equal(want[1], np.nonzero(tests.all(1))[0]) and 0 < want[1].shape[0] < len(rows)
    assert_equal_crop(run_front(scan), want)


def test_front_takes_wider_scans(mirror):
    scan = np.concatenate([waymo_frame(700, 3), np.full((700, 2), 9.0, np.float32)], 1)
    assert_equal_crop(run_front(scan), mirror.crop_front_mirror(scan))


def calib_of(data, name):
    calib = {"P": data["calib_P"], "V2C": data["calib_V2C"]}
    if name == "cam_r0":
        calib["R0"] = data["calib_R0"]
    return calib


@pytest.mark.parametrize("name", ("cam_r0", "cam_noR0"))
def test_camera_equals_the_fixture(golden, name):
    from ogc_amd.data_prepare.scan_ops import crop_camera
    data, meta = golden
    pc, idx = crop_camera(torch.from_numpy(data["cam_scan"]).cuda(), calib_of(data, name), meta["width"], meta["height"],
                          meta["clip_distance"], meta["depth_thresh"])
    assert pc.shape[0] == meta["cases"][name]["kept"]
    assert_equal_crop((pc.cpu().numpy(), idx.cpu().numpy()), (data[name + "_pc"], data[name + "_keep_idx"]))


def test_camera_equals_the_mirror_on_a_generated_frame(mirror):
    from ogc_amd.data_prepare.scan_ops import crop_camera
    from ogc_amd.pointnet2_cuda import SCAN_CROP_TILE as T
    rs = np.random.RandomState(5)
    scan = mirror.draw_scan(3 * T + 77, rs)
    for calib in (mirror.CALIB, {k: v for k, v in mirror.CALIB.items() if k != "R0"}):
        for _ in range(20):                                              # the generator's conditions, point by point
            bad = np.nonzero(~mirror.camera_point_ok(scan, calib))[0]
            if bad.size == 0:
                break
            scan[bad] = mirror.draw_scan(bad.size, rs)
    for calib in (mirror.CALIB, {k: v for k, v in mirror.CALIB.items() if k != "R0"}):
        assert mirror.camera_point_ok(scan, calib).all()
        want = mirror.crop_camera_mirror(scan, calib, mirror.WIDTH, mirror.HEIGHT, mirror.CLIP, mirror.DEPTH)
        assert T < want[1].shape[0] < scan.shape[0] - T
        pc, idx = crop_camera(torch.from_numpy(scan).cuda(), calib, mirror.WIDTH, mirror.HEIGHT, mirror.CLIP, mirror.DEPTH)
        assert_equal_crop((pc.cpu().numpy(), idx.cpu().numpy()), want)
        # other thresholds are arguments, not constants of the kernel
        want = mirror.crop_camera_mirror(scan, calib, 800, 300, 5.0, 20.0)
        pc, idx = crop_camera(torch.from_numpy(scan).cuda(), calib, 800, 300, 5.0, 20.0)
        assert_equal_crop((pc.cpu().numpy(), idx.cpu().numpy()), want)


def test_memory_contract(mirror, golden):
    """Rows >= M and a guard region behind each buffer keep their sentinel; count is written even for n == 0."""
    from ogc_amd import pointnet2_cuda as nat
    from ogc_amd.data_prepare.scan_ops import camera_block
    data, meta = golden
    front = waymo_frame(2 * nat.SCAN_CROP_TILE + 9, 12)
    cases = [("front", front, mirror.crop_front_mirror(front)),
             ("camera", data["cam_scan"], (data["cam_r0_pc"], data["cam_r0_keep_idx"])),
             ("front", np.zeros((0, 6), np.float32), (np.zeros((0, 3), np.float32), np.zeros(0, np.int32)))]
    cam = torch.from_numpy(camera_block(calib_of(data, "cam_r0"), meta["width"], meta["height"])).cuda()
    for kind, scan, want in cases:
        n = scan.shape[0]
        out_pc = torch.full((n * 3 + GUARD,), SENTINEL_F, dtype=torch.float32, device="cuda")
        keep_idx = torch.full((n + GUARD,), SENTINEL_I, dtype=torch.int32, device="cuda")
        count = torch.full((1 + GUARD,), SENTINEL_I, dtype=torch.int32, device="cuda")
        dev = torch.from_numpy(scan).cuda()
        if kind == "front":
            nat.scan_crop_front_wrapper(n, 6, dev, out_pc[:n * 3].view(n, 3), keep_idx[:n], count[:1])
        else:
            nat.scan_crop_camera_wrapper(n, 4, dev, cam, meta["clip_distance"], meta["depth_thresh"], out_pc[:n * 3].view(n, 3),
                                         keep_idx[:n], count[:1])
        m = int(count[0].item())
        assert m == want[1].shape[0]
        assert np.array_equal(out_pc[:m * 3].view(m, 3).cpu().numpy().view(np.int32), want[0].view(np.int32))
        assert np.array_equal(keep_idx[:m].cpu().numpy(), want[1])
        assert bool((out_pc[m * 3:] == SENTINEL_F).all()) and bool((keep_idx[m:] == SENTINEL_I).all())
        assert bool((count[1:] == SENTINEL_I).all())


def test_two_calls_give_the_same_bits():
    scan = waymo_frame(4000, 31)
    a, b = run_front(scan), run_front(scan)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.int32), b[0].view(np.int32))


def test_bad_inputs_raise():
    from ogc_amd import pointnet2_cuda as nat
    from ogc_amd.data_prepare.scan_ops import crop_camera, crop_front
    good = torch.from_numpy(waymo_frame(256, 1)).cuda()
    calib = {"P": np.eye(3, 4), "V2C": np.eye(3, 4)}
    with pytest.raises(RuntimeError):
        crop_front(good.t().contiguous().t())                            # column-major: not contiguous
    with pytest.raises(RuntimeError):
        crop_front(torch.cat([good, good], 1)[:, :6])                    # a view with a row stride of 12
    with pytest.raises(TypeError):
        crop_front(good.double())
    with pytest.raises(TypeError):
        crop_camera(good.half(), calib, 1242, 375)
    with pytest.raises(ValueError):
        crop_front(good[:, :4].contiguous())
    with pytest.raises(ValueError):
        crop_camera(good[:, :2].contiguous(), calib, 1242, 375)
    with pytest.raises(ValueError):
        crop_front(good[0])
    with pytest.raises(TypeError):
        crop_front(good.cpu().numpy())
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError):                                    # the C ABI's own check of the stride
        nat.scan_crop_front_wrapper(4, 5, good, torch.empty(4, 3, device="cuda"), torch.empty(4, dtype=torch.int32, device="cuda"), count)

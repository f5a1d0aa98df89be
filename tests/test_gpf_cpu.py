"""CPU-side checks of the ground-plane fixture (tests/golden/gpf.npz, written by tests/golden/make_gpf_golden.py from its float64
mirror `gpf_trace`) and of the boundary of ogc_amd/utils/gpf_util.py: no CPU path, and the library exports the entry point."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = {"g5": (1, 5), "g64": (1, 64), "g200": (1, 200), "g2048": (1, 2048), "g3000": (1, 3000), "g8192": (1, 8192),
         "ties": (1, 200), "neg": (1, 200), "axis2": (1, 200), "iter1": (1, 200), "retry": (1, 200), "tilted": (1, 200), "giveup": (1, 200),
         "batch": (4, 256)}
ARGS = ("n_iter", "n_lpr", "thresh_seed", "thresh_dist", "vertical_axis")


@pytest.fixture(scope="module")
def golden():
    data = np.load(os.path.join(HERE, "golden", "gpf.npz"))
    return data, json.loads(str(data["meta"]))


def test_fixture_loads_with_every_case(golden):
    data, meta = golden
    assert set(meta["cases"]) == set(SIZES)
    for name, (B, n) in SIZES.items():
        case = meta["cases"][name]
        pc = data[case["inputs"] + "_pc"]
        assert pc.shape == (B, n, 3) and pc.dtype == np.float32
        assert data[name + "_is_ground"].shape == (B, n) and data[name + "_is_ground"].dtype == np.bool_
        assert data[name + "_plane"].shape == (B, 6) and data[name + "_plane"].dtype == np.float64
        assert data[name + "_attempts"].shape == (B,) and data[name + "_attempts"].dtype == np.int32
        assert 1 <= case["n_lpr"] < n
    assert os.path.getsize(os.path.join(HERE, "golden", "gpf.npz")) < 256 * 1024


def test_recorded_margins_meet_the_thresholds(golden):
    _, meta = golden
    assert meta["thresholds"] == {"height": 1e-6, "dist": 1e-6, "rank": 1e-3, "final_s2_s1": 0.05, "final_s3_s2": 0.5}
    assert len(meta["smallest_height_margins"]) == 2 and min(meta["smallest_height_margins"]) >= 1e-6
    assert len(meta["smallest_dist_margins"]) == 2 and min(meta["smallest_dist_margins"]) >= 1e-6
    assert len(meta["smallest_rank_ratios"]) == 2 and min(meta["smallest_rank_ratios"]) >= 1e-3
    assert min(meta["smallest_final_s2_s1"]) >= 0.05 and max(meta["largest_final_s3_s2"]) <= 0.5


def test_fixture_covers_what_the_cases_are_for(golden):
    data, meta = golden
    assert len(set(data["batch_attempts"].tolist())) >= 3, "one launch must see clouds that need different numbers of fits"
    assert data["giveup_attempts"].tolist() == [8]
    assert not data["giveup_is_ground"].any() and not data["giveup_plane"].any()
    assert not data["batch_is_ground"][2].any() and not data["batch_plane"][2].any() and data["batch_attempts"][2] == 8
    assert 4 <= data["retry_attempts"][0] <= 7 and data["retry_is_ground"].any()
    assert 4 <= data["tilted_attempts"][0] <= 7 and data["tilted_is_ground"].any()
    line = data["tilted_pc"][0][np.argsort(data["tilted_pc"][0, :, 1])[:8]].astype(np.float64)
    assert np.ptp(line[:, 1]) == 0 and np.ptp(line[:, 0]) > 0 and np.ptp(line[:, 2]) > 0     # a line across two axes
    assert data["g5_attempts"][0] >= 2 and data["g5_is_ground"].any()
    assert meta["cases"]["iter1"]["inputs"] == "g200" and meta["cases"]["iter1"]["n_iter"] == 1
    assert meta["cases"]["axis2"]["vertical_axis"] == 2
    height = np.sort(data["ties_pc"][0, :, 1])
    kth, n_lpr = height[meta["cases"]["ties"]["n_lpr"] - 1], meta["cases"]["ties"]["n_lpr"]
    assert (height[:n_lpr] == kth).sum() >= 2 and (height[n_lpr:] == kth).sum() >= 2   # duplicates straddle the partition
    assert (data["neg_pc"][0, :, 1] < 0).any() and (data["neg_pc"][0, :, 1] > 0).any()
    for name in SIZES:     # planes: unit normals signed upwards, or all zero
        for plane in data[name + "_plane"]:
            if plane.any():
                assert abs(np.linalg.norm(plane[3:]) - 1.0) < 1e-12 and plane[3 + meta["cases"][name]["vertical_axis"]] >= 0


def test_the_mirror_reproduces_the_stored_results(golden):
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from make_gpf_golden import final_mask, gpf_trace
    data, meta = golden
    for name in SIZES:
        case = meta["cases"][name]
        kw = {k: case[k] for k in ARGS}
        for b, pc in enumerate(data[case["inputs"] + "_pc"]):
            mask, plane, attempts = gpf_trace(pc, **kw)
            assert np.array_equal(mask, data[name + "_is_ground"][b]) and attempts == data[name + "_attempts"][b]
            assert np.array_equal(plane, data[name + "_plane"][b])
            # the mask IS the reference's final line on the same points
            assert np.array_equal(final_mask(pc, plane, case["thresh_dist"]), mask)


def test_gpf_has_no_cpu_path():
    from ogc_amd.utils.gpf_util import ground_plane_fit_batch, ground_plane_fitting
    a = torch.zeros(8, 3)
    with pytest.raises(RuntimeError):
        ground_plane_fit_batch(a[None])
    with pytest.raises(RuntimeError):
        ground_plane_fitting(a)
    with pytest.raises(TypeError):
        ground_plane_fit_batch(a[None].double())
    with pytest.raises(TypeError):
        ground_plane_fit_batch(a[None].numpy())
    with pytest.raises(TypeError):
        ground_plane_fitting(a.double())
    with pytest.raises(TypeError):
        ground_plane_fitting(np.zeros((8, 3)))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            ground_plane_fitting(np.zeros((8, 3), np.float32))


def test_plane_mask_is_the_float64_formula():
    from ogc_amd.utils.gpf_util import plane_mask
    rs = np.random.RandomState(0)
    pts = (rs.rand(2, 50, 3) * 4 - 2).astype(np.float32)
    normal = rs.randn(2, 3)
    plane = np.concatenate([rs.randn(2, 3), normal / np.linalg.norm(normal, axis=1, keepdims=True)], 1)
    plane[1] = 0.0                                                      # a fit that gave up
    got = plane_mask(torch.from_numpy(pts), torch.from_numpy(plane), 0.4).numpy()
    want = np.abs(np.einsum("bnj,bj->bn", pts.astype(np.float64) - plane[:, None, :3], plane[:, 3:])) < 0.4
    assert got.dtype == np.bool_ and np.array_equal(got[0], want[0]) and 0 < want[0].sum() < 50
    assert not got[1].any()
    assert np.array_equal(plane_mask(torch.from_numpy(pts[0]), torch.from_numpy(plane[0]), 0.4).numpy(), want[0])


def test_library_exports_the_entry_point():
    from ogc_amd import _lib
    from ogc_amd.csrc import build as b
    lib = ctypes.CDLL(b.build())
    assert hasattr(lib, "ogc_ground_plane_fit")
    assert "ogc_ground_plane_fit" in _lib.SIGNATURES
    from ogc_amd import pointnet2_cuda
    assert callable(pointnet2_cuda.ground_plane_fit_wrapper)
    header = open(os.path.join(os.path.dirname(HERE), "include", "ogc_ops.h")).read()
    assert "#define OGC_GPF_MAX_POINTS 8192" in header

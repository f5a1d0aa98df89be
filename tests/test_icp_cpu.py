"""CPU-side checks of the rigid-ICP fixture (tests/golden/icp.npz, written by tests/golden/make_icp_golden.py from the
reference's `icp`) and of the boundary of ogc_amd/utils/icp_util.py: no CPU path, and the library exports the entry point."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ("a5", "a8", "a16", "b", "c", "d", "e", "f")
SIZES = {"a5": (1, 5), "a8": (1, 8), "a16": (1, 16), "b": (1, 200), "c": (1, 1024), "d": (1, 1500), "e": (3, 256), "f": (1, 1024)}


@pytest.fixture(scope="module")
def golden():
    data = np.load(os.path.join(HERE, "golden", "icp.npz"))
    return data, json.loads(str(data["meta"]))


def test_fixture_loads_with_every_case(golden):
    data, meta = golden
    assert set(meta["cases"]) == set(CASES)
    for name in CASES:
        case = meta["cases"][name]
        B, n = SIZES[name]
        src, dst = data[case["inputs"] + "_src"], data[case["inputs"] + "_dst"]
        assert src.shape == dst.shape == (B, n, 3) and src.dtype == dst.dtype == np.float32
        assert data[name + "_T"].shape == (B, 4, 4) and data[name + "_T"].dtype == np.float64
        assert data[name + "_distances"].shape == (B, n) and data[name + "_distances"].dtype == np.float64
        assert data[name + "_iters"].shape == (B,) and data[name + "_indices"].shape == (B, n)
        assert data[name + "_indices"].min() >= 0 and data[name + "_indices"].max() < n
        if case["has_init"]:
            assert data[case["inputs"] + "_init"].shape == (B, 4, 4)
    assert os.path.getsize(os.path.join(HERE, "golden", "icp.npz")) < 200 * 1024


def test_fixture_covers_what_the_cases_are_for(golden):
    data, meta = golden
    assert len(set(data["e_iters"].tolist())) == 3, "the batched pairs must stop at different iterations"
    assert data["f_iters"].tolist() == [2] and meta["cases"]["f"]["max_iterations"] == 3 and data["c_iters"][0] > 2
    assert meta["cases"]["f"]["inputs"] == "c"


def test_stored_transforms_are_rigid(golden):
    data, _ = golden
    for name in CASES:
        for T in data[name + "_T"]:
            R = T[:3, :3]
            assert np.abs(R.T @ R - np.eye(3)).max() < 1e-12
            assert abs(np.linalg.det(R) - 1.0) < 1e-12
            assert np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0])


def test_recorded_margins_meet_the_thresholds(golden):
    _, meta = golden
    assert meta["thresholds"] == {"gap": 1e-6, "tol_margin": 1e-6, "sv_ratio": 1e-4}
    assert len(meta["smallest_gaps"]) == 2 and min(meta["smallest_gaps"]) >= 1e-6
    assert len(meta["smallest_tol_margins"]) == 2 and min(meta["smallest_tol_margins"]) >= 1e-6
    assert meta["smallest_sv_ratio"] >= 1e-4


def test_icp_has_no_cpu_path():
    from ogc_amd.utils.icp_util import icp, icp_batch
    a = torch.zeros(8, 3)
    with pytest.raises(RuntimeError):
        icp(a, a)
    with pytest.raises(RuntimeError):
        icp_batch(a[None], a[None])
    with pytest.raises(TypeError):
        icp(a.double(), a.double())
    with pytest.raises(TypeError):
        icp(np.zeros((8, 3)), np.zeros((8, 3)))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            icp(np.zeros((8, 3), np.float32), np.zeros((8, 3), np.float32))


def test_library_exports_the_entry_point():
    from ogc_amd import _lib
    from ogc_amd.csrc import build as b
    lib = ctypes.CDLL(b.build())
    assert hasattr(lib, "ogc_rigid_icp")
    assert "ogc_rigid_icp" in _lib.SIGNATURES
    from ogc_amd import pointnet2_cuda
    assert callable(pointnet2_cuda.rigid_icp_wrapper)
    header = open(os.path.join(os.path.dirname(HERE), "include", "ogc_ops.h")).read()
    assert "#define OGC_ICP_MAX_POINTS" in header

"""CPU-side checks of the data-preparation kernels' fixture (tests/golden/scan_prepare.npz, written by
tests/golden/make_scan_prepare_golden.py) and of the boundary of ogc_amd/data_prepare/scan_ops.py: the library exports the entry
points, the exported tile sizes are the library's, and there is no CPU path."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
CAMERA_CASES, BOX_CASES = ("cam_r0", "cam_noR0"), ("box_a", "box_b")


@pytest.fixture(scope="module")
def golden():
    data = np.load(os.path.join(HERE, "golden", "scan_prepare.npz"))
    return data, json.loads(str(data["meta"]))


@pytest.fixture(scope="module")
def mirror():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_scan_prepare_golden
    return make_scan_prepare_golden


def calib_of(data, name):
    calib = {"P": data["calib_P"], "V2C": data["calib_V2C"]}
    if name == "cam_r0":
        calib["R0"] = data["calib_R0"]
    return calib


def test_fixture_is_small_and_complete(golden):
    data, meta = golden
    assert os.path.getsize(os.path.join(HERE, "golden", "scan_prepare.npz")) < 256 * 1024
    assert set(meta["cases"]) == set(CAMERA_CASES + BOX_CASES)
    scan = data["cam_scan"]
    assert scan.dtype == np.float32 and scan.shape == (meta["cases"]["cam_r0"]["n"], 4)
    for name in CAMERA_CASES:
        pc, idx = data[name + "_pc"], data[name + "_keep_idx"]
        assert pc.dtype == np.float32 and idx.dtype == np.int32 and pc.shape == (idx.shape[0], 3) == (meta["cases"][name]["kept"], 3)
        assert (np.diff(idx) > 0).all() and 0 < idx.shape[0] < scan.shape[0]
    for name in BOX_CASES:
        case = meta["cases"][name]
        assert data[name + "_pc"].shape == (case["n"], 3) and data[name + "_pc"].dtype == np.float32
        assert data[name + "_gt"].shape == (case["k"], 7) and data[name + "_gt"].dtype == np.float64
        for what in ("segm", "semantic_segm"):
            assert data["%s_%s" % (name, what)].shape == (case["n"],) and data["%s_%s" % (name, what)].dtype == np.int32
        assert case["in_three_boxes"] >= 5 and 0 < case["labelled"] < case["n"]


def test_recorded_margins_meet_the_thresholds(golden):
    _, meta = golden
    assert meta["thresholds"] == {"pixel": 1e-6, "face": 1e-7}
    assert meta["smallest_pixel_margin"] >= meta["thresholds"]["pixel"]
    assert meta["smallest_face_margin"] >= meta["thresholds"]["face"]
    assert meta["camera_points_redrawn"] >= 0 and meta["box_points_redrawn"] >= 0


def test_mirror_reproduces_the_stored_camera_crops(golden, mirror):
    data, meta = golden
    for name in CAMERA_CASES:
        calib = calib_of(data, name)
        pc, idx = mirror.crop_camera_mirror(data["cam_scan"], calib, meta["width"], meta["height"], meta["clip_distance"],
                                            meta["depth_thresh"])
        assert np.array_equal(idx, data[name + "_keep_idx"]) and np.array_equal(pc.view(np.int32), data[name + "_pc"].view(np.int32))
        ok = mirror.camera_point_ok(data["cam_scan"][:-3], calib)        # the conditions on the inputs still hold
        assert ok.all()
    assert not np.array_equal(data["cam_r0_pc"][:100], data["cam_noR0_pc"][:100])       # R0 is not a no-op


def test_mirror_reproduces_the_stored_box_labels(golden, mirror):
    from ogc_amd.data_prepare.kitti_io import waymo_boxes
    data, _ = golden
    for name in BOX_CASES:
        rows, ids = waymo_boxes(data[name + "_gt"], data[name + "_object_ids"], data[name + "_class_ids"])
        margins = []
        segm, semantic = mirror.box_segm_mirror(data[name + "_pc"], rows, ids, margins=margins)
        assert np.array_equal(segm, data[name + "_segm"]) and np.array_equal(semantic, data[name + "_semantic_segm"])
        assert min(margins) >= 1e-7
        # the last box wins: walking the boxes backwards and keeping the first hit is the same labelling
        first = np.zeros_like(segm)
        for k in range(rows.shape[0] - 1, -1, -1):
            hit = mirror.box_segm_mirror(data[name + "_pc"], rows[k:k + 1], ids[k:k + 1])[0]
            first = np.where((first == 0) & (hit != 0), hit, first)
        assert np.array_equal(first, segm)


def test_front_mirror_rejects_by_each_comparison(mirror):
    scan = np.array([[10, 1, 0, 0, 0, -1], [10, 1, 0, 0, 0, 0], [1, 2, 0, 0, 0, -1], [34, 1, 50, 0, 0, -1], [34.5, -33, 0, 0, 0, -1],
                     [35, 0, 0, 0, 0, -1], [60, 55, 0, 0, 0, -1], [np.nan, 0, 0, 0, 0, -1]], dtype=np.float32)
    pc, idx = mirror.crop_front_mirror(scan)
    assert idx.tolist() == [0, 4] and np.array_equal(pc, scan[[0, 4], :3])


def test_library_exports_the_entry_points_and_the_tile_sizes():
    from ogc_amd import pointnet2_cuda as nat
    from ogc_amd.csrc import build as b
    lib = ctypes.CDLL(b.build())
    for name in ("ogc_scan_crop_camera", "ogc_scan_crop_front", "ogc_box_segm"):
        assert hasattr(lib, name)
    lib.ogc_scan_crop_tile.restype = lib.ogc_box_segm_chunk.restype = ctypes.c_int
    assert lib.ogc_scan_crop_tile() == nat.SCAN_CROP_TILE and lib.ogc_box_segm_chunk() == nat.BOX_SEGM_CHUNK
    header = open(os.path.join(os.path.dirname(HERE), "include", "ogc_ops.h")).read()
    assert "#define OGC_SCAN_CROP_TILE %d\n" % nat.SCAN_CROP_TILE in header
    assert "#define OGC_BOX_SEGM_CHUNK %d\n" % nat.BOX_SEGM_CHUNK in header
    assert "#define OGC_BOX_SEGM_BOX_DOUBLES %d\n" % nat.BOX_SEGM_BOX_DOUBLES in header
    assert "#define OGC_SCAN_CROP_CAMERA_DOUBLES %d\n" % nat.SCAN_CROP_CAMERA_DOUBLES in header


def test_scan_ops_has_no_cpu_path(golden):
    from ogc_amd.data_prepare import scan_ops
    data, _ = golden
    assert scan_ops.SCAN_CROP_TILE == 1024 and scan_ops.BOX_SEGM_CHUNK == 128
    scan = torch.from_numpy(data["cam_scan"])
    with pytest.raises(RuntimeError):
        scan_ops.crop_camera(scan, calib_of(data, "cam_r0"), 1242, 375)
    with pytest.raises(RuntimeError):
        scan_ops.crop_front(torch.zeros(8, 6))
    with pytest.raises(RuntimeError):
        scan_ops.box_segm(torch.zeros(8, 3), torch.zeros(0, 18, dtype=torch.float64), torch.zeros(0, 2, dtype=torch.int32))
    with pytest.raises(TypeError):
        scan_ops.crop_front(torch.zeros(8, 6, dtype=torch.float64))


def test_camera_block_layout(golden):
    from ogc_amd.data_prepare.scan_ops import camera_block
    data, _ = golden
    block = camera_block(calib_of(data, "cam_r0"), 1242, 375)
    assert block.dtype == np.float64 and block.shape == (36,)
    assert np.array_equal(block[:12], data["calib_V2C"].reshape(-1)) and np.array_equal(block[12:21], data["calib_R0"].reshape(-1))
    assert np.array_equal(block[21:33], data["calib_P"].reshape(-1)) and block[33:].tolist() == [1242.0, 375.0, 1.0]
    block = camera_block(calib_of(data, "cam_noR0"), 1242, 375)
    assert block[35] == 0.0 and not block[12:21].any()

"""CPU-side checks of the preparation drivers' host parts: the synthetic raw roots hold what the drivers read, the parsers of
ogc_amd/data_prepare/kitti_io.py give back what the writers wrote, and the box rows built for KITTI-Det and Waymo, fed to the
float64 mirror of ogc_box_segm together with the mirror of the crop, label the synthetic points as they were constructed."""
import os
import pickle
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
N_POINTS = 3000


@pytest.fixture(scope="module")
def mirror():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_scan_prepare_golden
    return make_scan_prepare_golden


def clearance(pc, boxes, sign=(1, 1, 1)):
    """The smallest distance, over points and boxes, between a point and the box's surface along the axis that decides."""
    p = (np.asarray(pc, dtype=np.float32) * np.asarray(sign, dtype=np.float32)).astype(np.float64)
    out = np.inf
    for row in boxes:
        q = (p - row[9:12]) @ row[0:9].reshape(3, 3).T
        out = min(out, float(np.abs(np.minimum(q - row[12:15], row[15:18] - q).min(1)).min()))
    return out


@pytest.fixture(scope="module")
def kittidet(tmp_path_factory):
    from ogc_amd.utils.synthetic import write_kittidet_raw_root
    root = str(tmp_path_factory.mktemp("kittidet_raw"))
    return root, write_kittidet_raw_root(root, 2, N_POINTS)


@pytest.fixture(scope="module")
def semantickitti(tmp_path_factory):
    from ogc_amd.utils.synthetic import write_semantickitti_raw_root
    root = str(tmp_path_factory.mktemp("semantickitti_raw"))
    return root, write_semantickitti_raw_root(root, 2, N_POINTS, sequences=(0, 3))


@pytest.fixture(scope="module")
def waymo(tmp_path_factory):
    from ogc_amd.utils.synthetic import write_waymo_raw_root
    root = str(tmp_path_factory.mktemp("waymo_raw"))
    return root, write_waymo_raw_root(root, 2, 3, N_POINTS)


def test_kittidet_raw_root_and_parsers(kittidet):
    from ogc_amd.data_prepare import kitti_io
    from ogc_amd.data_prepare.process_kittidet import frame_ids
    root, frames = kittidet
    base = os.path.join(root, "training")
    assert frame_ids(os.path.join(base, "velodyne")) == [0, 1]
    for i, frame in enumerate(frames):
        scan = np.fromfile(os.path.join(base, "velodyne", "%06d.bin" % i), dtype=np.float32)
        assert scan.size % 4 == 0 and scan.size // 4 == frame["labels"].shape[0] and abs(scan.size // 4 - N_POINTS) < N_POINTS // 5
        calib = kitti_io.read_kittidet_calib(os.path.join(base, "calib", "%06d.txt" % i))
        for key, shape in (("P", (3, 4)), ("V2C", (3, 4)), ("R0", (3, 3))):
            assert calib[key].shape == shape and calib[key].dtype == np.float64 and np.array_equal(calib[key], frame["calib"][key])
        assert set(kitti_io.read_calib_file(os.path.join(base, "calib", "%06d.txt" % i))) >= {"P2", "R0_rect", "Tr_velo_to_cam"}
        assert kitti_io.image_size(os.path.join(base, "image_2", "%06d.png" % i)) == (1242, 375)
        objects = kitti_io.read_label(os.path.join(base, "label_2", "%06d.txt" % i))
        assert [o.type for o in objects] == ["Pedestrian", "Car", "DontCare", "Car", "Car"]
        for obj, (kind, h, w, l, tx, ty, tz, ry) in zip(objects, frame["objects"]):
            assert (obj.type, obj.h, obj.w, obj.l, obj.t, obj.ry) == (kind, h, w, l, (tx, ty, tz), ry)
        boxes, ids = kitti_io.kittidet_boxes(objects)
        assert boxes.shape == (3, 18) and boxes.dtype == np.float64 and ids.tolist() == [[2, 1], [4, 1], [5, 1]]
        assert np.array_equal(boxes[0, :9].reshape(3, 3), kitti_io.roty(-objects[1].ry)) and boxes[0, 9:12].tolist() == list(objects[1].t)
        assert np.allclose(boxes[0, 12:], [-objects[1].l / 2 - 0.01, -objects[1].h - 0.01, -objects[1].w / 2 - 0.01,
                                           objects[1].l / 2 + 0.01, 0.01, objects[1].w / 2 + 0.01], rtol=0, atol=1e-15)
    assert "cv2" not in sys.modules


def test_kittidet_boxes_label_the_synthetic_points_as_constructed(kittidet, mirror):
    from ogc_amd.data_prepare import kitti_io
    root, frames = kittidet
    base = os.path.join(root, "training")
    for i, frame in enumerate(frames):
        scan = np.fromfile(os.path.join(base, "velodyne", "%06d.bin" % i), dtype=np.float32).reshape(-1, 4)
        pc, keep_idx = mirror.crop_camera_mirror(scan, frame["calib"], 1242, 375)
        assert 512 <= pc.shape[0] < scan.shape[0]
        boxes, ids = kitti_io.kittidet_boxes(kitti_io.read_label(os.path.join(base, "label_2", "%06d.txt" % i)))
        segm, semantic = mirror.box_segm_mirror(pc, boxes, ids, sign=kitti_io.KITTIDET_SIGN)
        assert np.array_equal(segm, frame["labels"][keep_idx]) and np.array_equal(semantic, (segm > 0).astype(np.int32))
        assert len(set(segm.tolist())) >= 3
        assert clearance(pc, boxes, kitti_io.KITTIDET_SIGN) > 0.049          # RAW_MARGIN less the float32 rounding of the scan


def test_semantickitti_raw_root_and_parsers(semantickitti, mirror):
    from ogc_amd.data_prepare import kitti_io
    from ogc_amd.data_prepare.process_semantickitti import relabel
    root, written = semantickitti
    assert sorted(os.listdir(os.path.join(root, "sequences"))) == ["00", "03"]
    for sequence, record in written.items():
        base = os.path.join(root, "sequences", "%02d" % sequence)
        calib = kitti_io.read_semantickitti_calib(os.path.join(base, "calib.txt"))
        assert set(calib) == {"P", "V2C"} and np.array_equal(calib["P"], record["calib"]["P"])
        assert np.array_equal(calib["V2C"], record["calib"]["V2C"])
        assert sorted(os.listdir(os.path.join(base, "labels"))) == ["000000.label", "000001.label"]
        for i, label in enumerate(record["labels"]):
            scan = np.fromfile(os.path.join(base, "velodyne", "%06d.bin" % i), dtype=np.float32).reshape(-1, 4)
            words = np.fromfile(os.path.join(base, "labels", "%06d.label" % i), dtype=np.int32)
            assert np.array_equal(words, label) and words.shape[0] == scan.shape[0]
            assert set((words & 0xFFFF).tolist()) == {10, 18, 30, 40, 252} and (words >> 16).max() == 2
            pc, keep_idx = mirror.crop_camera_mirror(scan, calib, 1242, 375)
            assert 512 <= pc.shape[0] < scan.shape[0]
            segm = relabel(words[keep_idx])
            # person and road are one background; car, moving-car and truck keep their ranks by label word
            kept = sorted(w for w in set(words[keep_idx].tolist()) if (w & 0xFFFF) in (10, 18, 252))
            want = np.array([kept.index(w) + 1 if w in kept else 0 for w in words[keep_idx].tolist()])
            assert np.array_equal(segm, want) and len(kept) >= 2


def test_waymo_raw_root(waymo):
    from ogc_amd.utils.synthetic import WAYMO_RAW_BOXES
    root, written = waymo
    with open(os.path.join(root, "train.txt")) as f:
        listed = f.read().split()
    assert len(listed) == 3 and all(name.endswith(".tfrecord") for name in listed)
    assert sorted(written) == sorted(os.path.splitext(name)[0] for name in listed[:2])
    for seq, frames in written.items():
        with open(os.path.join(root, "waymo_processed_data", seq, seq + ".pkl"), "rb") as f:
            infos = pickle.load(f)
        assert len(infos) == len(frames) == 3
        for t, (info, frame) in enumerate(zip(infos, frames)):
            assert info["point_cloud"] == {"lidar_sequence": seq, "sample_idx": t}
            assert info["pose"].shape == (4, 4) and info["pose"].dtype == np.float64 and np.array_equal(info["pose"], frame["pose"])
            scan = np.load(os.path.join(root, "waymo_processed_data", seq, "%04d.npy" % t))
            vel = np.load(os.path.join(root, "scene_flow", seq, "%04d.npy" % t))
            assert scan.dtype == np.float32 and scan.shape == (frame["box"].shape[0], 6) and vel.dtype == np.float32
            assert vel.shape == (scan.shape[0], 4) and not vel[frame["static"], :3].any() and vel[~frame["static"], :3].any()
            assert set(scan[:, 5].tolist()) == {-1.0, 0.0, 1.0}
            x, y, z = scan[:, 0], scan[:, 1], scan[:, 2]
            assert (x <= abs(y)).any() and (x >= 35).any() and (abs(y) >= 50).any() and (x * x + y * y + z * z >= 3600).any()
            annos = info["annos"]
            assert sorted(annos["name"].tolist()) == sorted(name for name, _ in WAYMO_RAW_BOXES)
            assert annos["gt_boxes_lidar"].shape == (len(WAYMO_RAW_BOXES), 7) and annos["gt_boxes_lidar"].dtype == np.float64
            assert (annos["num_points_in_gt"] == 0).sum() == 1 and len(set(annos["obj_ids"].tolist())) == len(WAYMO_RAW_BOXES)


def test_waymo_boxes_label_the_synthetic_points_as_constructed(waymo, mirror):
    from ogc_amd.data_prepare import kitti_io
    from ogc_amd.data_prepare.process_waymo import CLASS_NAMES, filter_annos
    from ogc_amd.utils.synthetic import WAYMO_RAW_BOXES
    root, written = waymo
    for seq, frames in written.items():
        with open(os.path.join(root, "waymo_processed_data", seq, seq + ".pkl"), "rb") as f:
            infos = pickle.load(f)
        for t, (info, frame) in enumerate(zip(infos, frames)):
            scan = np.load(os.path.join(root, "waymo_processed_data", seq, "%04d.npy" % t))
            pc, keep_idx = mirror.crop_front_mirror(scan)
            assert 0 < pc.shape[0] < scan.shape[0]
            gt, names, trackings = filter_annos(info["annos"], True)
            assert sorted(names.tolist()) == sorted(n for n, counted in WAYMO_RAW_BOXES if counted and n in CLASS_NAMES)
            index = np.array([int(trk[-2:]) + 1 for trk in trackings], dtype=np.int32)       # the writer's box number
            boxes, ids = kitti_io.waymo_boxes(gt, index, [CLASS_NAMES.index(n) + 1 for n in names])
            segm, semantic = mirror.box_segm_mirror(pc, boxes, ids)
            truth = frame["box"][keep_idx]
            labelled = np.isin(truth, index)
            assert np.array_equal(segm, np.where(labelled, truth, 0)) and (truth[~labelled] > 0).any()
            assert clearance(pc, boxes) > 0.049
            classes = np.array([0] + [CLASS_NAMES.index(n) + 1 if n in CLASS_NAMES else 0 for n, _ in WAYMO_RAW_BOXES])
            assert np.array_equal(semantic, np.where(labelled, classes[truth], 0))
            unfiltered, _, _ = filter_annos(info["annos"], False)
            assert unfiltered.shape[0] == len(WAYMO_RAW_BOXES) - 1                            # `unknown` alone is dropped


def test_waymo_box_rows_are_the_closed_form_of_the_reference_rotation():
    from scipy.spatial.transform import Rotation
    from ogc_amd.data_prepare.kitti_io import waymo_boxes
    gt = np.array([[1.0, 2.0, 3.0, 4.0, 2.0, 1.5, 0.7], [0.0, 0.0, 0.0, 1.0, 1.0, 1.0, -2.9]])
    rows, ids = waymo_boxes(gt.astype(np.float32), [7, 9], [1, 3])
    assert rows.dtype == np.float64 and ids.dtype == np.int32 and ids.tolist() == [[7, 1], [9, 3]]
    for k in range(2):
        h = np.float64(np.float32(gt[k, 6]))
        assert np.allclose(rows[k, :9].reshape(3, 3), Rotation.from_euler("zyx", [-h, 0, 0]).as_matrix(), rtol=0, atol=1e-15)
    assert np.array_equal(rows[0, 9:12], gt[0, :3]) and rows[0, 15:].tolist() == [2.01, 0.76, 1.01]       # l on x, h on y, w on z
    assert np.array_equal(rows[0, 12:15], -rows[0, 15:])


def test_drivers_refuse_to_run_without_a_device(tmp_path, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from ogc_amd.data_prepare import process_kittidet, process_semantickitti, process_waymo
    with pytest.raises(RuntimeError):
        process_kittidet.main([str(tmp_path)])
    with pytest.raises(RuntimeError):
        process_semantickitti.main([str(tmp_path)])
    with pytest.raises(RuntimeError):
        process_waymo.main(["--data_root", str(tmp_path), "--save_root", str(tmp_path), "--split_file", str(tmp_path / "train.txt")])

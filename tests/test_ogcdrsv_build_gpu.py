"""The OGC-DRSV chain on a synthetic mesh root of 2 scenes x 4 frames (ogc_amd/utils/synthetic.py::write_ogcdr_mesh_root):
sample_pointcloud --keep_background -> build_ogcdrsv at 160 x 90 -> collect_segm -> the reader.  The written .pcd clouds
against the meshes (on a surface, nothing in front of them as seen from the eye), against the mirror pipeline of
tests/depth_render_cases.py in every bit, and the data/ tree collect_segm leaves."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import depth_render_cases as cases  # noqa: E402
import ogcdr_prepare_cases as prepare_cases  # noqa: E402

from ogc_amd.data_prepare import build_ogcdrsv, collect_segm, mesh_io, sample_pointcloud  # noqa: E402
from ogc_amd.datasets import OGCDynamicRoomDataset  # noqa: E402
from ogc_amd.utils.data_util import fps_downsample  # noqa: E402

WIDTH, HEIGHT = 160, 90
N_SAMPLE_POINT, N_FPS, N_SINGLE = 6000, 256, 64


@pytest.fixture(scope="module")
def roots(tmp_path_factory):
    base = tmp_path_factory.mktemp("ogcdrsv_chain")
    out = {"mesh": str(base / "mesh_root"), "complete": str(base / "complete"), "single": str(base / "single")}
    sample_pointcloud.main([out["mesh"], "--save_root", out["complete"], "--synthetic", "2", "--keep_background", "--n_sample_point", str(N_SAMPLE_POINT),
                            "--n_sample_point_fps", str(N_FPS)])
    out["built"] = build_ogcdrsv.main(["--src_root", out["mesh"], "--dest_root", out["single"], "--width", str(WIDTH), "--height", str(HEIGHT)])
    out["collected"] = collect_segm.main(["--src_root", out["complete"], "--dest_root", out["single"], "--n_sample_point", str(N_SINGLE)])
    out["ids"] = sorted(os.listdir(os.path.join(out["mesh"], "mesh")))
    return out


def object_meshes(mesh_root, name, frame_id):
    d = os.path.join(mesh_root, "mesh", name)
    return [mesh_io.read_obj(os.path.join(d, "object_%02d_%02d.obj" % (frame_id, k))) for k in range(int(name[:2]))]


def distance_to_mesh(points, vertices, faces):
    """The distance of every point to the nearest face it projects into (faces with area only): (P,) float64, inf where none."""
    points = np.asarray(points, dtype=np.float64)
    o, e1, e2 = vertices[faces[:, 0]], vertices[faces[:, 1]] - vertices[faces[:, 0]], vertices[faces[:, 2]] - vertices[faces[:, 0]]
    normal = np.cross(e1, e2)
    length = np.linalg.norm(normal, axis=1)
    o, e1, e2, normal = o[length > 0], e1[length > 0], e2[length > 0], normal[length > 0] / length[length > 0, None]
    d = points[:, None, :] - o[None]
    height = (d * normal[None]).sum(2)
    g11, g12, g22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
    b1, b2 = (d * e1[None]).sum(2), (d * e2[None]).sum(2)
    det = g11 * g22 - g12 * g12
    s, t = (g22 * b1 - g12 * b2) / det, (g11 * b2 - g12 * b1) / det
    inside = (s > -1e-4) & (t > -1e-4) & (s + t < 1 + 1e-4)
    return np.where(inside, np.abs(height), np.inf).min(1)


def nearer_hits(eye, points, vertices, faces, margin):
    """Per point the number of faces the segment eye -> point crosses in their interior before `1 - margin` of its length."""
    v0, e1, e2 = vertices[faces[:, 0]], vertices[faces[:, 1]] - vertices[faces[:, 0]], vertices[faces[:, 2]] - vertices[faces[:, 0]]
    directions = (np.asarray(points, dtype=np.float64) - eye)[:, None, :]
    pvec = np.cross(directions, e2[None])
    with np.errstate(all="ignore"):
        inv = 1.0 / (e1[None] * pvec).sum(-1)
        tvec = eye - v0
        u = (tvec[None] * pvec).sum(-1) * inv
        qvec = np.cross(tvec, e1)
        v = (directions * qvec[None]).sum(-1) * inv
        t = (e2 * qvec).sum(-1)[None] * inv
        crossed = (u > 1e-6) & (v > 1e-6) & (u + v < 1 - 1e-6) & (t > 0) & (t < 1 - margin)
    return crossed.sum(1)


def test_pcd_points_lie_on_the_object_meshes_and_face_the_eye(roots):
    assert roots["built"]["scenes"] == roots["ids"] and len(roots["ids"]) == 2
    total = 0
    for name in roots["ids"]:
        assert sorted(os.listdir(os.path.join(roots["single"], "pcd", name))) == ["pc_%02d.pcd" % t for t in range(4)]
        for t in range(4):
            pc = mesh_io.read_pcd(os.path.join(roots["single"], "pcd", name, "pc_%02d.pcd" % t))
            assert pc.dtype == np.float32 and pc.ndim == 2 and pc.shape[1] == 3 and pc.shape[0] > N_SINGLE
            total += pc.shape[0]
            meshes = object_meshes(roots["mesh"], name, t)
            # the float32 cast of a point of the surface: half an ulp per coordinate, sqrt(3) of it in norm, and as much again of slack
            on_mesh = 2 * np.sqrt(3.0) * 2.0 ** -24 * float(np.abs(pc).max())
            dist = np.min([distance_to_mesh(pc, *mesh) for mesh in meshes], 0)
            assert dist.max() < on_mesh, (name, t, dist.max(), on_mesh)
            vertices, faces, _ = sample_pointcloud.concat_meshes(meshes)
            eye = np.array(build_ogcdrsv.frame_view(vertices, WIDTH, HEIGHT, 60.0, 0.7).e)
            assert (nearer_hits(eye, pc, vertices, faces, 1e-5) == 0).all(), (name, t)
            assert len(np.unique(pc, axis=0)) == len(pc)
    assert roots["built"]["points"] == total


def test_written_clouds_equal_the_mirror_pipeline(roots):
    for name in roots["ids"]:
        for t in range(4):
            vertices, faces, offsets = sample_pointcloud.concat_meshes(object_meshes(roots["mesh"], name, t))
            view = cases.default_view_mirror(vertices.min(0), vertices.max(0), WIDTH, HEIGHT)
            want = cases.mirror_render(vertices, faces, view, WIDTH, HEIGHT)
            assert want["code"] == 0 and want["dropped_near"] == 0
            pc = mesh_io.read_pcd(os.path.join(roots["single"], "pcd", name, "pc_%02d.pcd" % t))
            assert pc.shape == want["points"].shape and np.array_equal(pc.view(np.uint32), want["points"].view(np.uint32)), (name, t)
            points, mesh_idx = build_ogcdrsv.render_frame(object_meshes(roots["mesh"], name, t), WIDTH, HEIGHT, 60.0, 0.7)
            assert np.array_equal(points.view(np.uint32), pc.view(np.uint32))
            assert np.array_equal(mesh_idx, np.searchsorted(offsets, want["face_of_point"], side="right") - 1) and len(set(mesh_idx)) >= 2


def test_collect_segm_leaves_the_data_tree_it_promises(roots):
    assert roots["collected"]["scenes"] == roots["ids"]
    for name in roots["ids"]:
        for t in range(4):
            d = os.path.join(roots["single"], "data", name)
            pc, segm, pose = (np.load(os.path.join(d, "%s_%02d.npy" % (what, t))) for what in ("pc", "segm", "pose"))
            src = os.path.join(roots["complete"], "data", name)
            src_pc, src_segm, src_pose = (np.load(os.path.join(src, "%s_%02d.npy" % (what, t))) for what in ("pc", "segm", "pose"))
            view = mesh_io.read_pcd(os.path.join(roots["single"], "pcd", name, "pc_%02d.pcd" % t))
            assert pc.dtype == np.float32 and pc.shape == (N_SINGLE, 3) and segm.dtype == np.int16 and segm.shape == (N_SINGLE,)
            assert np.array_equal(pc, view[fps_downsample(view, n_sample_point=N_SINGLE)])
            want, _ = prepare_cases.nearest_label_reference(pc[None], src_pc[None], src_segm[None])
            assert np.array_equal(segm, want[0]) and (segm > 0).any() and np.array_equal(pose, src_pose)
    for split in ("train", "val", "test"):
        assert open(os.path.join(roots["single"], "data", split + ".lst")).read() == open(os.path.join(roots["complete"], "data", split + ".lst")).read()
    dataset = OGCDynamicRoomDataset(roots["single"], "val", view_sels=[[0, 1], [2, 3]])
    assert len(dataset) == 2 * len(roots["ids"])
    pcs, segms, flows, valids = dataset[0]
    assert pcs.shape == (2, N_SINGLE, 3) and segms.shape == (2, N_SINGLE) and flows.shape == (2, N_SINGLE, 3)


def test_errors_name_scene_and_frame(roots, tmp_path):
    corner = np.array([[0.0, 0.0, 0.0], [0.01, 0.0, 0.0], [0.0, 0.01, 0.0]])
    two_corners = [(corner, np.array([[0, 1, 2]], dtype=np.int32)), (corner + np.array([1.0, 1.0, 0.0]), np.array([[0, 1, 2]], dtype=np.int32))]
    with pytest.raises(ValueError, match="scene 03_000007, frame 2 renders no point at 9 x 5"):
        build_ogcdrsv.render_frame(two_corners, 9, 5, 60.0, 0.7, where="scene 03_000007, frame 2")
    with pytest.raises(ValueError, match="somewhere holds no triangle"):
        build_ogcdrsv.render_frame([(corner, np.zeros((0, 3), dtype=np.int32))], 9, 5, 60.0, 0.7, where="somewhere")
    bad = corner.copy()
    bad[1, 1] = np.inf
    with pytest.raises(ValueError, match="not finite"):
        build_ogcdrsv.render_frame([(bad, np.array([[0, 1, 2]], dtype=np.int32))], 9, 5, 60.0, 0.7)
    # through the command line: a root whose only object is out of every centre's way at 1 x 1
    root = str(tmp_path / "sparse")
    os.makedirs(os.path.join(root, "mesh", "01_000000"))
    for t in range(4):
        vertices = np.concatenate([corner, corner + np.array([1.0, 1.0, 0.0])])
        mesh_io.write_obj(os.path.join(root, "mesh", "01_000000", "object_%02d_00.obj" % t), vertices, [[0, 1, 2], [3, 4, 5]])
    with pytest.raises(ValueError, match="scene 01_000000, frame 0 renders no point"):
        build_ogcdrsv.main(["--src_root", root, "--dest_root", str(tmp_path / "sparse_out"), "--width", "1", "--height", "1"])
    with pytest.raises(FileNotFoundError):
        build_ogcdrsv.main(["--src_root", os.path.join(roots["mesh"], "mesh"), "--dest_root", str(tmp_path / "nothing")])


def test_synthetic_flag_writes_the_mesh_root_first(tmp_path):
    src, dest = str(tmp_path / "src"), str(tmp_path / "dest")
    out = build_ogcdrsv.main(["--src_root", src, "--dest_root", dest, "--width", "64", "--height", "36", "--synthetic", "1"])
    assert len(out["scenes"]) == 1 and out["points"] > 0
    assert sorted(os.listdir(os.path.join(dest, "pcd", out["scenes"][0]))) == ["pc_%02d.pcd" % t for t in range(4)]

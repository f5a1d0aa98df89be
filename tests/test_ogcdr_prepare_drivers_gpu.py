"""The two drivers of the OGC-DR preparation (ogc_amd/data_prepare/sample_pointcloud.py, collect_segm.py) on a synthetic
mesh root of 2 scenes x 4 frames (ogc_amd/utils/synthetic.py::write_ogcdr_mesh_root), 6000 surface points sampled to 256: the written
clouds against the meshes, against the reference's crop expression and against the mirror pipeline of tests/ogcdr_prepare_cases.py,
the package's reader on the result, and collect_segm's labels against scipy's cdist."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ogcdr_prepare_cases as cases  # noqa: E402

from ogc_amd.data_prepare import collect_segm, mesh_io, mesh_ops, sample_pointcloud  # noqa: E402
from ogc_amd.datasets import OGCDynamicRoomDataset  # noqa: E402
from ogc_amd.utils import synthetic  # noqa: E402
from ogc_amd.utils.data_util import fps_downsample  # noqa: E402

N_SAMPLE_POINT, N_FPS, N_SINGLE = 6000, 256, 64
SIZES = ["--n_sample_point", str(N_SAMPLE_POINT), "--n_sample_point_fps", str(N_FPS)]


@pytest.fixture(scope="module")
def roots(tmp_path_factory):
    base = tmp_path_factory.mktemp("ogcdr_chain")
    mesh = str(base / "mesh_root")
    out = {"mesh": mesh, "plain": str(base / "plain"), "background": str(base / "background"), "again": str(base / "again"),
           "seed1": str(base / "seed1"), "single": str(base / "single")}
    sample_pointcloud.main([mesh, "--save_root", out["plain"], "--synthetic", "2"] + SIZES)
    sample_pointcloud.main([mesh, "--save_root", out["background"], "--keep_background"] + SIZES)
    sample_pointcloud.main([mesh, "--save_root", out["again"], "--keep_background"] + SIZES)
    sample_pointcloud.main([mesh, "--save_root", out["seed1"], "--keep_background", "--seed", "1"] + SIZES)
    out["ids"] = sorted(os.listdir(os.path.join(mesh, "mesh")))
    out["views"] = synthetic.write_ogcdr_singleview_root(out["single"], out["background"])
    collect_segm.main(["--src_root", out["background"], "--dest_root", out["single"], "--n_sample_point", str(N_SINGLE)])
    return out


def frame_meshes(mesh_root, name, frame_id, background):
    d = os.path.join(mesh_root, "mesh", name)
    meshes = [mesh_io.read_obj(os.path.join(d, "object_%02d_%02d.obj" % (frame_id, k))) for k in range(int(name[:2]))]
    if background:
        meshes += [mesh_io.read_obj(os.path.join(d, "ground.obj"))] + [mesh_io.read_obj(os.path.join(d, "wall_%02d.obj" % w)) for w in range(4)]
    return meshes


def xz_range(mesh_root, name):
    with open(os.path.join(mesh_root, "mesh", name, "meta.pkl"), "rb") as f:
        return pickle.load(f)["xz_ground_range"]


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


ON_MESH = 2e-7      # float32 coordinates of magnitude < 0.5: half an ulp is 1.5e-8 per coordinate, 2.6e-8 in norm; the rest is slack


def load(root, name, frame_id):
    d = os.path.join(root, "data", name)
    return tuple(np.load(os.path.join(d, "%s_%02d.npy" % (what, frame_id))) for what in ("pc", "segm", "pose"))


@pytest.mark.parametrize("which", ["plain", "background"])
def test_files_points_on_their_meshes_and_outside_the_thickness(roots, which):
    background = which == "background"
    for name in roots["ids"]:
        xz = xz_range(roots["mesh"], name)
        for t in range(4):
            pc, segm, pose = load(roots[which], name, t)
            assert pc.dtype == np.float32 and pc.shape == (N_FPS, 3) and segm.dtype == np.int16 and segm.shape == (N_FPS,)
            assert np.array_equal(pose, np.load(os.path.join(roots["mesh"], "data", name, "pose_%02d.npy" % t)))
            meshes = frame_meshes(roots["mesh"], name, t, background)
            assert set(np.unique(segm)) == set(range(0 if background else 1, 4))
            for label in np.unique(segm):
                parts = [meshes[label - 1]] if label > 0 else meshes[3:]
                dist = np.min([distance_to_mesh(pc[segm == label], *part) for part in parts], 0)
                assert dist.max() < ON_MESH, (name, t, label, dist.max())
            assert cases.crop_mask_reference(pc, xz).all()
            assert len(np.unique(pc, axis=0)) == N_FPS
    assert sorted(os.listdir(os.path.join(roots[which], "data"))) == roots["ids"] + ["test.lst", "train.lst", "val.lst"]
    assert open(os.path.join(roots[which], "data", "val.lst")).read().split() == roots["ids"]


@pytest.mark.parametrize("which", ["plain", "background"])
def test_written_clouds_equal_the_mirror_pipeline(roots, which):
    """Candidate mirror, thinning mirror, the first `count` survivors, the cast, the reference's crop expression in numpy — and the
    package's own FPS on what is left."""
    background = which == "background"
    removed = 0
    for scene_index, name in enumerate(roots["ids"]):
        for t in (0, 3):
            meshes = frame_meshes(roots["mesh"], name, t, background)
            vertices, faces, face_offsets = sample_pointcloud.concat_meshes(meshes)
            cum = cases.cumulative_areas(vertices, faces, face_offsets)
            area = np.array([cum[face_offsets[m + 1] - 1] for m in range(len(meshes))])
            counts = np.array(sample_pointcloud.point_counts(area, N_SAMPLE_POINT))
            cand_offsets = np.concatenate([[0], np.cumsum(3 * counts)])
            points, _, _ = cases.candidates_mirror(vertices, faces, cum, face_offsets, cand_offsets, sample_pointcloud.frame_seed(0, scene_index, t))
            keep = cases.greedy_thin_reference(points, cand_offsets, np.sqrt(area / (3 * counts)))
            chosen, labels = [], []
            for m in range(len(meshes)):
                survivors = cand_offsets[m] + np.nonzero(keep[cand_offsets[m]:cand_offsets[m + 1]])[0]
                assert len(survivors) >= counts[m]
                chosen.append(survivors[:counts[m]])
                labels.append(np.full(counts[m], m + 1 if m < 3 else 0, dtype=np.int16))
            pts, labels = points[np.concatenate(chosen)].astype(np.float32), np.concatenate(labels)
            mask = cases.crop_mask_reference(pts, xz_range(roots["mesh"], name))
            removed += int((~mask).sum())
            pts, labels = pts[mask], labels[mask]
            fps_idx = fps_downsample(pts, n_sample_point=N_FPS)
            pc, segm, _ = load(roots[which], name, t)
            assert np.array_equal(pc.view(np.uint32), pts[fps_idx].view(np.uint32)), (name, t)
            assert np.array_equal(segm, labels[fps_idx]), (name, t)
    assert (removed > 0) == background          # the thickness of ground and walls is there to be cut, the objects are not touched


def test_crop_on_the_device_equals_numpy_on_and_next_to_every_bound():
    """Points at the float32 nearest each bound and one float32 to either side, for ranges whose bounds round up and down: the y
    test is decided in float32, the x and z tests in float64."""
    for xz in (np.array([0.4, 0.3]), np.array([1.0, 0.6123]), np.array([0.77, 1.0])):
        bounds = [(1, cases.GROUND_LEVEL - 1e-4)]
        for column, extent in ((0, xz[0]), (2, xz[1])):
            bounds += [(column, -extent / 2. + cases.WALL_THICKNESS - 1e-4), (column, extent / 2. - cases.WALL_THICKNESS + 1e-4)]
        pts = []
        for column, bound in bounds:
            at = np.float32(bound)
            for value in (np.nextafter(at, np.float32(-9)), at, np.nextafter(at, np.float32(9))):
                p = np.array([0.0, 0.0, 0.0], dtype=np.float32)
                p[column] = value
                pts.append(p)
        pts = np.stack(pts)
        want = cases.crop_mask_reference(pts, xz)
        got = sample_pointcloud.crop_mask(torch.from_numpy(pts).cuda(), xz).cpu().numpy()
        assert np.array_equal(got, want), xz
        assert 0 < want.sum() < len(want)


def test_one_seed_one_result_another_seed_another(roots):
    differ = 0
    for name in roots["ids"]:
        for t in range(4):
            for what in ("pc", "segm", "pose"):
                path = os.path.join("data", name, "%s_%02d.npy" % (what, t))
                a, b, c = (open(os.path.join(roots[k], path), "rb").read() for k in ("background", "again", "seed1"))
                assert a == b, path
                differ += int(what == "pc" and a != c)
    assert differ == 4 * len(roots["ids"])


def test_reader_loads_the_root_and_its_flow_lands_on_the_next_mesh(roots):
    dataset = OGCDynamicRoomDataset(roots["plain"], "val", view_sels=[[0, 1], [2, 3]])
    assert len(dataset) == 2 * len(roots["ids"])
    for sid in range(len(dataset)):
        pcs, segms, flows, valids = dataset[sid]
        name, (t1, t2) = roots["ids"][sid // 2], dataset.view_sels[sid % 2]
        assert pcs.shape == (2, N_FPS, 3) and flows.shape == (2, N_FPS, 3) and segms.shape == (2, N_FPS) and valids.all()
        pc1, segm1, _ = load(roots["plain"], name, t1)
        assert np.array_equal(pcs[0], pc1) and np.abs(flows[0]).max() > 1e-3
        target = frame_meshes(roots["mesh"], name, t2, False)
        for label in (1, 2, 3):
            moved = (pcs[0] + flows[0])[segm1 == label]
            assert distance_to_mesh(moved, *target[label - 1]).max() < 4 * ON_MESH, (name, label)


def test_collect_segm_labels_equal_cdist_and_files(roots):
    for name in roots["ids"]:
        for t in range(4):
            pc, segm, pose = load(roots["single"], name, t)
            src_pc, src_segm, src_pose = load(roots["background"], name, t)
            view = mesh_io.read_pcd(os.path.join(roots["single"], "pcd", name, "pc_%02d.pcd" % t))
            assert view.shape == (roots["views"][name][t], 3) and N_SINGLE <= len(view) < N_FPS
            assert pc.dtype == np.float32 and np.array_equal(pc, view[fps_downsample(view, n_sample_point=N_SINGLE)])
            want, _ = cases.nearest_label_reference(pc[None], src_pc[None], src_segm[None])
            assert segm.dtype == src_segm.dtype == np.int16 and np.array_equal(segm, want[0])
            assert len(np.unique(segm)) > 1 and np.array_equal(pose, src_pose)
    for split in ("train", "val", "test"):
        assert open(os.path.join(roots["single"], "data", split + ".lst")).read() == open(os.path.join(roots["background"], "data", split + ".lst")).read()


def test_errors_name_what_is_wrong(roots, tmp_path):
    first = roots["ids"][0]
    with pytest.raises(ValueError, match=r"pcd.%s.pc_00\.pcd holds \d+ points, fewer than the 1000" % first):
        collect_segm.main(["--src_root", roots["background"], "--dest_root", roots["single"], "--n_sample_point", "1000"])
    with pytest.raises(ValueError, match="scene %s, frame 0 keeps" % first):
        sample_pointcloud.main([roots["mesh"], "--save_root", str(tmp_path / "few"), "--n_sample_point", "200", "--n_sample_point_fps", "256"])
    other = str(tmp_path / "other_key")
    synthetic.write_ogcdr_mesh_root(other, 1, meta_key="xz_groundplane_range")          # the key the reference reads
    assert sample_pointcloud.main([other, "--save_root", str(tmp_path / "other_out")] + SIZES)["lists"] == ["train", "val", "test"]
    missing = str(tmp_path / "missing_key")
    synthetic.write_ogcdr_mesh_root(missing, 1, meta_key="xz_range")
    with pytest.raises(KeyError, match=r"meta\.pkl holds neither"):
        sample_pointcloud.main([missing, "--save_root", str(tmp_path / "missing_out")] + SIZES)
    packed = str(tmp_path / "packed")
    os.makedirs(os.path.join(packed, "pcd", first))
    with open(os.path.join(packed, "pcd", first, "pc_00.pcd"), "wb") as f:
        f.write(b"VERSION 0.7\nFIELDS x y z\nSIZE 4 4 4\nTYPE F F F\nCOUNT 1 1 1\nWIDTH 1\nHEIGHT 1\nPOINTS 1\nDATA binary_compressed\n\0\0\0\0")
    with pytest.raises(ValueError, match="binary_compressed"):
        collect_segm.main(["--src_root", roots["background"], "--dest_root", packed])


def test_sample_surface_even_returns_the_first_count_survivors_in_order(roots):
    """mesh_ops.sample_surface_even against the mirrors, with a mesh of count 0 and one that keeps fewer than its count: a slab."""
    meshes = frame_meshes(roots["mesh"], roots["ids"][0], 2, False) + [cases.cube_mesh((0.1, 0.1, 1e-7))]
    vertices, faces, face_offsets = sample_pointcloud.concat_meshes(meshes)
    counts = np.array([500, 0, 40, 300])
    got_points, got_mesh = mesh_ops.sample_surface_even(vertices, faces, face_offsets, counts, 123)
    cum = cases.cumulative_areas(vertices, faces, face_offsets)
    area = np.array([cum[face_offsets[m + 1] - 1] for m in range(4)])
    cand_offsets = np.concatenate([[0], np.cumsum(3 * counts)])
    points, _, _ = cases.candidates_mirror(vertices, faces, cum, face_offsets, cand_offsets, 123)
    radius = np.sqrt(area / np.maximum(3 * counts, 1))        # (the mesh without candidates: any radius)
    keep = cases.greedy_thin_reference(points, cand_offsets, radius)
    want_points, want_mesh = [], []
    for m in range(4):
        survivors = cand_offsets[m] + np.nonzero(keep[cand_offsets[m]:cand_offsets[m + 1]])[0][:counts[m]]
        want_points.append(points[survivors])
        want_mesh += [m] * len(survivors)
    assert got_points.dtype == torch.float64 and got_mesh.dtype == torch.int32
    assert np.array_equal(got_mesh.cpu().numpy(), want_mesh) and np.array_equal(got_points.cpu().numpy(), np.concatenate(want_points))
    per_mesh = np.bincount(want_mesh, minlength=4)
    assert per_mesh[0] == 500 and per_mesh[1] == 0 and per_mesh[2] == 40
    assert 100 < per_mesh[3] < 300          # a slab thinner than the radius: its two sides thin each other, fewer than `count` are left

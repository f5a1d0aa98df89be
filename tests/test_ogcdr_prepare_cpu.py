"""The device-free side of the OGC-DR preparation: the .obj and .pcd readers, the numpy mirrors of
tests/ogcdr_prepare_cases.py against each other and against what they stand for, the point counts, the layout
write_ogcdr_mesh_root leaves, and the refusals of mesh_ops that need no device."""
import os
import pickle
import struct
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ogcdr_prepare_cases as cases  # noqa: E402

from ogc_amd.data_prepare import mesh_io, mesh_ops  # noqa: E402
from ogc_amd.utils import synthetic  # noqa: E402

N_SAMPLE_POINT, N_FPS = 6000, 256       # the sizes of tests/test_ogcdr_prepare_drivers_gpu.py


def test_obj_round_trip_with_slashes_negative_indices_and_a_quad(tmp_path):
    path = str(tmp_path / "mesh.obj")
    with open(path, "w") as f:
        f.write("# a comment\nmtllib none.mtl\nv 0 0 0\nv 1 0 0 0.5 0.5 0.5\nv 1 1 0\nvn 0 0 1\nvt 0 0\nv 0 1 0\n"
                "f 1/1/1 2/1/1 3/1/1\nf 1//1 3//1 4//1\nv 0.1 0.2 1e-3\nf -1 -5 -4\nf 1 2 3 4\nf 2/1 3/1 5/1 4/1 1/1\ng group\n")
    v, f = mesh_io.read_obj(path)
    assert v.dtype == np.float64 and f.dtype == np.int32
    assert np.array_equal(v, [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.1, 0.2, 1e-3]])
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [4, 0, 1], [0, 1, 2], [0, 2, 3], [1, 2, 4], [1, 4, 3], [1, 3, 0]]
    rs = np.random.RandomState(0)
    vertices = rs.randn(9, 3) * np.array([1e-3, 1.0, 1e3])
    out = str(tmp_path / "out.obj")
    mesh_io.write_obj(out, vertices, [[0, 1, 2], [3, 4, 5, 6], [6, 7, 8]])
    v2, f2 = mesh_io.read_obj(out)
    assert np.array_equal(v2, vertices)            # every float64 bit survives the text
    assert f2.tolist() == [[0, 1, 2], [3, 4, 5], [3, 5, 6], [6, 7, 8]]
    with open(path, "a") as f:
        f.write("f 1 2 9\n")
    with pytest.raises(ValueError, match="mesh.obj:16"):
        mesh_io.read_obj(path)


def _pcd_header(fields, sizes, types, n, data):
    return ("# .PCD v0.7\nVERSION 0.7\nFIELDS %s\nSIZE %s\nTYPE %s\nCOUNT %s\nWIDTH %d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA %s\n"
            % (fields, sizes, types, " ".join("1" for _ in fields.split()), n, n, data)).encode("ascii")


def test_read_pcd_ascii_binary_and_the_refusal_of_compressed(tmp_path):
    pts = np.array([[0.5, -1.25, 3.0], [1e-3, 2.0, -7.5], [4.0, 5.0, 6.0]], dtype=np.float32)
    ascii_path = str(tmp_path / "a.pcd")
    with open(ascii_path, "wb") as f:
        f.write(_pcd_header("x y z rgb", "4 4 4 4", "F F F U", 3, "ascii"))
        f.write(b"".join(("%r %r %r 255\n" % tuple(float(c) for c in p)).encode("ascii") for p in pts))
    got = mesh_io.read_pcd(ascii_path)
    assert got.dtype == np.float32 and np.array_equal(got, pts)
    binary_path = str(tmp_path / "b.pcd")
    with open(binary_path, "wb") as f:      # an intensity byte between y and z, a double behind: fields of other sizes are skipped
        f.write(_pcd_header("x y i z t", "4 4 1 4 8", "F F U F F", 3, "binary"))
        for p in pts:
            f.write(struct.pack("<ffBfd", float(p[0]), float(p[1]), 7, float(p[2]), 0.25))
    got = mesh_io.read_pcd(binary_path)
    assert got.dtype == np.float32 and np.array_equal(got, pts)
    round_trip = str(tmp_path / "c.pcd")
    mesh_io.write_pcd(round_trip, pts)
    assert np.array_equal(mesh_io.read_pcd(round_trip), pts)
    packed = str(tmp_path / "d.pcd")
    with open(packed, "wb") as f:
        f.write(_pcd_header("x y z", "4 4 4", "F F F", 3, "binary_compressed") + b"\0" * 16)
    with pytest.raises(ValueError, match="binary_compressed"):
        mesh_io.read_pcd(packed)
    doubles = str(tmp_path / "e.pcd")
    with open(doubles, "wb") as f:
        f.write(_pcd_header("x y z", "8 8 8", "F F F", 0, "binary"))
    with pytest.raises(ValueError, match="float32"):
        mesh_io.read_pcd(doubles)
    short = str(tmp_path / "f.pcd")
    with open(short, "wb") as f:
        f.write(_pcd_header("x y z", "4 4 4", "F F F", 3, "binary") + pts[:2].tobytes())
    with pytest.raises(ValueError, match="bytes of data"):
        mesh_io.read_pcd(short)


def test_philox_known_answers():
    """Philox4x32-10 against the known-answer vectors of the Random123 distribution (kat_vectors)."""
    def run(counter, key):
        return [int(w[0]) for w in cases.philox4x32_10([np.array([c], dtype=np.uint64) for c in counter], key)]
    assert run((0, 0, 0, 0), (0, 0)) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert run((0xffffffff,) * 4, (0xffffffff, 0xffffffff)) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert run((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)) == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_thinning_mirrors_agree_and_the_round_form_gives_the_same():
    for n, seed in ((300, 1), (1500, 2), (5000, 3)):
        pts = cases.cube_surface_points(n, seed)
        r = float(np.sqrt(6.0 / n))
        loop = cases.greedy_thin_reference(pts, [0, n], [r], method="loop")
        tree = cases.greedy_thin_reference(pts, [0, n], [r], method="tree")
        assert np.array_equal(loop, tree), n
        assert n // 3 < loop.sum() < n         # more survivors than the wanted third of the candidates
    pts = cases.cube_surface_points(1500, 2)
    r = float(np.sqrt(6.0 / 1500))
    want = cases.greedy_thin_reference(pts, [0, 1500], [r])
    keep, rounds = cases.thin_rounds_simulation(pts, r)
    assert np.array_equal(keep, want) and 2 <= rounds <= 40
    for seed, stale in ((5, 0.0), (6, 0.3), (7, 0.9)):       # any order inside a round, any amount of stale reads: the same result
        keep, more = cases.thin_rounds_simulation(pts, r, rs=np.random.RandomState(seed), stale=stale)
        assert np.array_equal(keep, want), (seed, stale)
    # the bound is inclusive and exact on small integers / 8; different meshes never interact
    lattice = np.array([[0, 0, 0], [0.375, 0.5, 0], [0.75, 1.0, 0.0], [0.375, 0.5, 0.0]])
    assert cases.greedy_thin_reference(lattice, [0, 4], [0.625]).tolist() == [1, 0, 1, 0]
    assert cases.greedy_thin_reference(lattice, [0, 4], [0.62]).tolist() == [1, 1, 1, 0]
    assert cases.greedy_thin_reference(lattice, [0, 2, 4], [0.625, 0.625]).tolist() == [1, 0, 1, 0]
    assert cases.greedy_thin_reference(lattice, [0, 1, 4], [9.0, 0.0]).tolist() == [1, 1, 1, 0]


def _three_faces():
    """Triangles of areas 1 : 2 : 4 with zero-area faces in front of, between and behind them."""
    vertices = np.array([[0, 0, 0], [2, 0, 0], [0, 1, 0],   [5, 0, 0], [7, 0, 0], [5, 2, 0],   [0, 5, 1], [4, 5, 1], [0, 7, 1]], dtype=np.float64)
    faces = np.array([[0, 0, 1], [0, 1, 2], [3, 3, 3], [3, 4, 5], [1, 2, 1], [6, 7, 8], [8, 8, 6]], dtype=np.int32)
    return vertices, faces


def test_candidate_mirror_points_lie_in_their_triangles_with_the_right_shares():
    vertices, faces = _three_faces()
    offsets = [0, len(faces)]
    cum = cases.cumulative_areas(vertices, faces, offsets)
    assert cum.tolist() == [0.0, 1.0, 1.0, 3.0, 3.0, 7.0, 7.0]
    n = 70000
    points, face_idx, bary = cases.candidates_mirror(vertices, faces, cum, offsets, [0, n], seed=20261020)
    assert set(np.unique(face_idx)) == {1, 3, 5}                        # a zero-area face is never picked
    o, e1, e2 = vertices[faces[face_idx, 0]], vertices[faces[face_idx, 1]] - vertices[faces[face_idx, 0]], vertices[faces[face_idx, 2]] - vertices[faces[face_idx, 0]]
    # barycentric coordinates recovered from the point itself, by least squares in the triangle's plane
    d = points - o
    g11, g12, g22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
    b1, b2 = (d * e1).sum(1), (d * e2).sum(1)
    det = g11 * g22 - g12 * g12
    s, t = (g22 * b1 - g12 * b2) / det, (g11 * b2 - g12 * b1) / det
    assert np.abs(d - (s[:, None] * e1 + t[:, None] * e2)).max() < 1e-12      # in the plane
    assert s.min() > -1e-12 and t.min() > -1e-12 and (s + t).max() < 1 + 1e-12
    assert np.abs(s - bary[:, 0]).max() < 1e-12 and np.abs(t - bary[:, 1]).max() < 1e-12
    for face, share in ((1, 1 / 7), (3, 2 / 7), (5, 4 / 7)):
        got, sigma = int((face_idx == face).sum()), np.sqrt(n * share * (1 - share))
        assert abs(got - n * share) < 4 * sigma, (face, got, n * share, sigma)
    # a candidate depends on (seed, mesh, index) alone: a prefix of a longer draw, whatever else the call holds
    again = cases.candidates_mirror(vertices, faces, cum, offsets, [0, 100], seed=20261020)
    assert np.array_equal(again[0], points[:100]) and np.array_equal(again[1], face_idx[:100])
    other = cases.candidates_mirror(vertices, faces, cum, offsets, [0, 100], seed=20261021)
    assert not np.array_equal(other[0], points[:100])
    u = cases.candidate_uniforms(3, 1, 50000)
    assert u.min() >= 0.0 and u.max() < 1.0 and np.abs(u.mean(0) - 0.5).max() < 0.01
    assert np.array_equal(u * 2.0 ** 53, np.floor(u * 2.0 ** 53))           # 53-bit integers times 2^-53
    # pick on the last face, and beyond every running sum: clamped to the last face that adds area
    assert np.minimum(np.searchsorted(cum, 7.0, side="right"), np.searchsorted(cum, cum[-1], side="left")) == 5


def test_point_counts_are_cut_not_rounded():
    from ogc_amd.data_prepare.sample_pointcloud import frame_seed, point_counts
    assert point_counts([1.0, 2.0, 4.0], 70) == [10, 20, 40]
    assert point_counts([1.0, 1.0, 1.0], 100) == [33, 33, 33]
    assert point_counts([0.0, 3.0], 10) == [0, 10]
    areas = [0.3, 0.2, 0.123]
    c = np.array(areas)
    c /= sum(c)
    assert point_counts(areas, 100000) == [int(v * 100000) for v in c]
    seeds = {frame_seed(s, i, t) for s in (0, 1, 2 ** 31) for i in (0, 1, 300) for t in range(4)}
    assert len(seeds) == 36 and all(0 <= s < 2 ** 64 for s in seeds)


@pytest.fixture(scope="module")
def mesh_root(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("ogcdr_meshes"))
    return root, synthetic.write_ogcdr_mesh_root(root, 2)


def _frame_meshes(root, name, frame_id, background):
    d = os.path.join(root, "mesh", name)
    meshes = [mesh_io.read_obj(os.path.join(d, "object_%02d_%02d.obj" % (frame_id, k))) for k in range(int(name[:2]))]
    if background:
        meshes += [mesh_io.read_obj(os.path.join(d, "ground.obj"))] + [mesh_io.read_obj(os.path.join(d, "wall_%02d.obj" % w)) for w in range(4)]
    return meshes


def test_mesh_root_layout_loads(mesh_root):
    root, ids = mesh_root
    assert ids == ["03_000000", "03_000001"] and sorted(os.listdir(os.path.join(root, "mesh"))) == ids
    assert open(os.path.join(root, "data", "val.lst")).read().split() == ids
    assert open(os.path.join(root, "data", "train.lst")).read() == "" and os.path.exists(os.path.join(root, "data", "test.lst"))
    for name in ids:
        with open(os.path.join(root, "mesh", name, "meta.pkl"), "rb") as f:
            meta = pickle.load(f)
        xr = meta["xz_ground_range"]
        assert xr.dtype == np.float64 and xr.shape == (2,) and meta["n_object"] == 3
        ground, *walls = _frame_meshes(root, name, 0, True)[3:]
        assert np.allclose(ground[0].min(0), [-xr[0] / 2, -0.5, -xr[1] / 2]) and np.allclose(ground[0].max(0), [xr[0] / 2, -0.49, xr[1] / 2])
        for w, (axis, side) in enumerate(((2, -1), (0, -1), (2, 1), (0, 1))):       # build_ogcdr.py:370-396
            lo, hi = walls[w][0].min(0), walls[w][0].max(0)
            assert np.isclose(lo[1], -0.49) and np.isclose(hi[1] - lo[1], meta["wall_height"]) and np.isclose(hi[axis] - lo[axis], 0.01)
            assert np.isclose((lo if side < 0 else hi)[axis], side * xr[(0, None, 1)[axis]] / 2)
        canon = None
        for t in range(4):
            poses = np.load(os.path.join(root, "data", name, "pose_%02d.npy" % t))
            assert poses.shape == (3, 4, 4) and poses.dtype == np.float64
            objects = _frame_meshes(root, name, t, False)
            sizes = [len(f) for _, f in objects]
            assert sizes == [52, 80, 108]            # 48 + 4 zero-area faces; the ellipsoid; 106 triangles + the quad's two
            areas = cases.face_areas(*objects[0])
            assert (areas == 0).sum() == 4 and areas[0] == 0 and areas[-1] == 0
            for k, (v, f) in enumerate(objects):
                assert v.min(0)[1] > -0.49 and np.abs(v[:, 0]).max() < xr[0] / 2 - 0.01 and np.abs(v[:, 2]).max() < xr[1] / 2 - 0.01
                back = (v - poses[k, :3, 3]) @ poses[k, :3, :3]          # the rigid motion undone: the same canonical mesh every frame
                if t == 0:
                    canon = (canon or []) + [back]
                else:
                    assert np.abs(back - canon[k]).max() < 1e-12


def test_the_mirror_leaves_at_least_count_survivors_for_every_synthetic_mesh(mesh_root):
    """The condition under which sample_surface_even's "first `count` survivors" is exercised, not "all of them", at the sizes of
    the driver test: every mesh of the synthetic root, with and without the background."""
    from ogc_amd.data_prepare.sample_pointcloud import concat_meshes, frame_seed, point_counts
    root, ids = mesh_root
    for scene_index, name in enumerate(ids):
        for background in (False, True):
            meshes = _frame_meshes(root, name, 1, background)
            vertices, faces, face_offsets = concat_meshes(meshes)
            cum, area = mesh_ops.cumulative_areas(vertices, faces, face_offsets)
            assert np.array_equal(cum, cases.cumulative_areas(vertices, faces, face_offsets))
            counts = np.array(point_counts(area, N_SAMPLE_POINT))
            assert counts.min() > 0 and N_SAMPLE_POINT - len(meshes) <= counts.sum() <= N_SAMPLE_POINT
            cand_offsets = np.concatenate([[0], np.cumsum(3 * counts)])
            points, _, _ = cases.candidates_mirror(vertices, faces, cum, face_offsets, cand_offsets, frame_seed(0, scene_index, 1))
            radius = mesh_ops.even_radius(area, counts)
            keep = cases.greedy_thin_reference(points, cand_offsets, radius)
            survivors = np.add.reduceat(keep, cand_offsets[:-1])
            assert (survivors >= counts).all(), (name, background, survivors.tolist(), counts.tolist())
            if background:
                assert radius.max() < 0.01          # below the thickness of ground and walls: their two sides do not thin each other


def test_crop_expression_compares_y_in_float32_and_x_z_in_float64():
    xz = np.array([0.4, 0.3])
    y_bound, x_bound = np.float32(cases.GROUND_LEVEL - 1e-4), -xz[0] / 2. + cases.WALL_THICKNESS - 1e-4
    pts = np.zeros((4, 3), dtype=np.float32)
    pts[0, 1] = y_bound                                                 # equal in float32, above the float64 bound or not: removed
    pts[1, 1] = np.nextafter(y_bound, np.float32(1))
    pts[2, 0] = np.float32(x_bound)                                     # the float32 nearest the bound, compared as a double
    pts[3, 0] = np.nextafter(np.float32(x_bound), np.float32(1))
    want = [False, True, bool(np.float64(np.float32(x_bound)) > x_bound), True]
    assert cases.crop_mask_reference(pts, xz).tolist() == want


def test_operators_refuse_before_they_touch_a_device():
    f64, i32 = torch.zeros(4, 3, dtype=torch.float64), torch.zeros(3, dtype=torch.int32)
    with pytest.raises(TypeError):
        mesh_ops.surface_thin(f64.float(), i32, torch.zeros(2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh_ops.surface_thin(f64, i32, torch.zeros(2, dtype=torch.float64))
    with pytest.raises(TypeError):
        mesh_ops.nearest_label(torch.zeros(1, 4, 3, dtype=torch.float64), torch.zeros(1, 4, 3), torch.zeros(1, 4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh_ops.nearest_label(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3), torch.zeros(1, 4, dtype=torch.int32))
    with pytest.raises(TypeError):
        mesh_ops.surface_candidates(f64, torch.zeros(2, 3, dtype=torch.int64), torch.zeros(2, dtype=torch.float64), i32, i32, 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh_ops.surface_candidates(f64, torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, dtype=torch.float64), i32, i32, 0)
    assert mesh_ops.face_areas([[0, 0, 0], [2, 0, 0], [0, 1, 0]], np.array([[0, 1, 2], [0, 0, 1]])).tolist() == [1.0, 0.0]

"""The three operators of the OGC-DR preparation on the device (csrc/surface_candidates.hip, surface_thin.hip,
nearest_label.hip) against the numpy mirrors of tests/ogcdr_prepare_cases.py: every bit of the candidates, every keep flag of the
thinning and every index of the label transfer, at the launch edges and on the inputs built to break them."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ogcdr_prepare_cases as cases  # noqa: E402

from ogc_amd import pointnet2_cuda as native  # noqa: E402
from ogc_amd.data_prepare import mesh_ops  # noqa: E402
from ogc_amd.utils import synthetic  # noqa: E402


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


# ---- candidates ------------------------------------------------------------------------------------------------------------------

def three_faces():
    vertices = np.array([[0, 0, 0], [2, 0, 0], [0, 1, 0], [5, 0, 0], [7, 0, 0], [5, 2, 0], [0, 5, 1], [4, 5, 1], [0, 7, 1]], dtype=np.float64)
    faces = np.array([[0, 0, 1], [0, 1, 2], [3, 3, 3], [3, 4, 5], [1, 2, 1], [6, 7, 8], [8, 8, 6]], dtype=np.int32)
    return vertices, faces


def triangulated(mesh):
    """(vertices, faces as lists, a quad among them) -> (vertices, (F, 3) int32) by the fan of mesh_io.read_obj."""
    vertices, faces = mesh
    return vertices, np.array([[f[0], f[k], f[k + 1]] for f in faces for k in range(1, len(f) - 1)], dtype=np.int32)


def five_meshes():
    rs = np.random.RandomState(11)
    single = (np.array([[0.1, 0.2, 0.3], [1.5, -0.25, 0.75], [-0.5, 2.0, 1.0]]), np.array([[0, 1, 2]], dtype=np.int32))
    return [cases.cube_mesh(1.0), three_faces(), single, triangulated(synthetic.ogcdr_object_mesh(0, rs)),
            triangulated(synthetic.ogcdr_object_mesh(1, rs))]


def concat(meshes):
    vertices = np.concatenate([v for v, _ in meshes])
    shift = np.cumsum([0] + [len(v) for v, _ in meshes])
    faces = np.concatenate([f + shift[m] for m, (_, f) in enumerate(meshes)]).astype(np.int32)
    return vertices, faces, np.cumsum([0] + [len(f) for _, f in meshes]).astype(np.int32)


def draw(meshes, counts, seed):
    vertices, faces, face_offsets = concat(meshes)
    cum = cases.cumulative_areas(vertices, faces, face_offsets)
    cand_offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    got = mesh_ops.surface_candidates(dev(vertices, np.float64), dev(faces, np.int32), dev(cum, np.float64), dev(face_offsets, np.int32),
                                      dev(cand_offsets, np.int32), seed)
    want = cases.candidates_mirror(vertices, faces, cum, face_offsets, cand_offsets, seed)
    return got[0].cpu().numpy(), got[1].cpu().numpy(), want


@pytest.mark.parametrize("total", [1, 63, 64, 65, 255, 256, 257, 4099])
def test_candidates_equal_the_mirror_in_every_bit(total):
    meshes = five_meshes()
    for which, seed in (([1], 5), ([2], 2 ** 63 + 12345), ([0, 1, 2, 3, 4], -7)):        # interleaved zero-area faces; one face; five
        share = np.array([3, 1, 2, 4, 5][:len(which)], dtype=np.float64)
        counts = np.floor(share / share.sum() * total).astype(np.int64)
        counts[0] += total - counts.sum()
        points, face_idx, want = draw([meshes[m] for m in which], counts, seed)
        assert points.shape == (total, 3) and points.dtype == np.float64 and face_idx.dtype == np.int32
        assert np.array_equal(points.view(np.uint64), want[0].view(np.uint64)), (total, which)
        assert np.array_equal(face_idx, want[1]), (total, which)
    vertices, faces, _ = concat(meshes)
    assert (cases.face_areas(vertices, faces)[face_idx] > 0).all()          # the five meshes: no zero-area face chosen anywhere
    assert counts.min() > 0 or total < 15


def test_candidates_pick_on_the_last_face_and_zero_area_in_front():
    """A mesh whose last face of area is followed by zero-area faces and takes almost all the area: most picks land on it, none
    behind it; and a leading zero-area face is never the pick, whatever u0 is."""
    vertices = np.array([[0, 0, 0], [1e-3, 0, 0], [0, 1e-3, 0], [0, 0, 0], [10, 0, 0], [0, 10, 0]], dtype=np.float64)
    faces = np.array([[0, 0, 0], [0, 1, 2], [3, 4, 5], [5, 5, 3], [4, 4, 4]], dtype=np.int32)
    points, face_idx, want = draw([(vertices, faces)], [3000], 99)
    assert np.array_equal(points.view(np.uint64), want[0].view(np.uint64)) and np.array_equal(face_idx, want[1])
    assert set(np.unique(face_idx)) <= {1, 2} and (face_idx == 2).sum() > 2900


def test_candidates_of_a_mesh_do_not_depend_on_the_rest_of_the_call():
    meshes = five_meshes()
    alone = draw([meshes[3]], [700], 31)
    first_of_many = draw([meshes[3], meshes[0], meshes[1]], [300, 4099, 12], 31)
    assert np.array_equal(alone[0][:300].view(np.uint64), first_of_many[0][:300].view(np.uint64))
    assert np.array_equal(alone[1][:300], first_of_many[1][:300])
    other_seed = draw([meshes[3]], [300], 32)
    assert not np.array_equal(alone[0][:300], other_seed[0])
    empty = draw([meshes[0], meshes[1]], [0, 0], 1)
    assert empty[0].shape == (0, 3)


def test_candidates_refusals_by_status():
    vertices, faces = cases.cube_mesh()
    cum = cases.cumulative_areas(vertices, faces, [0, 12])
    good = dict(vertices=vertices, faces=faces, cum=cum, face_offsets=[0, 12], cand_offsets=[0, 100])

    def call(raw=False, **change):
        a = dict(good, **change)
        args = [dev(a["vertices"], np.float64), dev(a["faces"], np.int32), dev(a["cum"], np.float64), dev(a["face_offsets"], np.int32),
                dev(a["cand_offsets"], np.int32)]
        if not raw:
            return mesh_ops.surface_candidates(*args, 3)
        total = int(a["cand_offsets"][-1])
        points = torch.full((total, 3), 7.0, dtype=torch.float64, device="cuda")
        face_idx = torch.full((total,), 7, dtype=torch.int32, device="cuda")
        status = torch.full((1,), 7, dtype=torch.int32, device="cuda")
        native.surface_candidates_wrapper(total, len(a["face_offsets"]) - 1, len(a["vertices"]), len(a["faces"]), *args, 3, points, face_idx, status)
        return int(status.item()), bool((points == 7.0).all()) and bool((face_idx == 7).all())

    assert call(raw=True) [0] == 0
    bad_face = faces.copy()
    bad_face[5, 1] = 8
    negative = faces.copy()
    negative[11, 2] = -1
    flat = np.zeros_like(vertices)
    changes = ((1, dict(faces=bad_face)), (1, dict(faces=negative)),
               (2, dict(face_offsets=[0, 8, 4, 12], cand_offsets=[0, 10, 50, 100])), (2, dict(cand_offsets=[0, 60, 40, 100], face_offsets=[0, 4, 8, 12])),
               (2, dict(face_offsets=[1, 12])), (2, dict(face_offsets=[0, 11])),
               (3, dict(vertices=flat, cum=cases.cumulative_areas(flat, faces, [0, 12]))),
               (3, dict(face_offsets=[0, 12, 12], cand_offsets=[0, 50, 100])))
    for code, change in changes:
        assert call(raw=True, **change) == (code, True), change.keys()
        with pytest.raises(ValueError, match="surface_candidates"):
            call(**change)
    # a mesh without area is fine as long as nothing is drawn from it
    points, _ = call(face_offsets=[0, 12, 12], cand_offsets=[0, 100, 100])
    assert points.shape == (100, 3)


# ---- thinning --------------------------------------------------------------------------------------------------------------------

def thin(points, cand_offsets, radius):
    keep, rounds = mesh_ops.surface_thin(dev(points, np.float64).reshape(-1, 3), dev(cand_offsets, np.int32), dev(radius, np.float64),
                                         return_rounds=True)
    return keep.cpu().numpy(), rounds


def check_independently(points, cand_offsets, radius, keep):
    """Without the mirror: no two kept points of a mesh within r of each other, and every removed point has a kept point of lower
    index within r."""
    from scipy.spatial import cKDTree
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    assert set(np.unique(keep)) <= {0, 1}
    for m in range(len(cand_offsets) - 1):
        lo, hi = cand_offsets[m], cand_offsets[m + 1]
        p, k, r = points[lo:hi], keep[lo:hi], radius[m]
        if hi == lo:
            continue
        pairs = cKDTree(p).query_pairs(float(r) * (1 + 1e-9) + 1e-300, output_type="ndarray")
        pairs = pairs[cases.within(p[pairs[:, 0]], p[pairs[:, 1]], r)]
        a, b = pairs.min(1), pairs.max(1)
        assert not (k[a] & k[b]).any(), "two kept points within the radius"
        covered = np.zeros(hi - lo, dtype=bool)
        covered[b[k[a] == 1]] = True
        assert np.array_equal(covered, k == 0), "a removed point without a kept point of lower index within the radius"


def check_thin(points, cand_offsets, radius):
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    keep, rounds = thin(points, cand_offsets, radius)
    assert keep.dtype == np.int32 and keep.shape == (len(points),)
    want = cases.greedy_thin_reference(points, cand_offsets, radius)
    assert np.array_equal(keep, want), "%d of %d flags differ" % ((keep != want).sum(), len(keep))
    check_independently(points, cand_offsets, radius, keep)
    return keep, rounds


def test_thin_one_and_two_points():
    assert check_thin([[0.5, 1.0, -2.0]], [0, 1], [0.3])[0].tolist() == [1]
    assert check_thin([[0, 0, 0], [0.1, 0.2, 0.2]], [0, 2], [0.31])[0].tolist() == [1, 0]         # distance 0.3
    assert check_thin([[0, 0, 0], [0.1, 0.2, 0.2]], [0, 2], [0.29])[0].tolist() == [1, 1]
    assert thin(np.zeros((0, 3)), [0, 0], [1.0])[0].shape == (0,)


def test_thin_lattice_points_at_exactly_the_radius():
    """Coordinates are integers / 8: every difference, square and sum is exact, so d == r is decided by the inclusive bound alone."""
    rs = np.random.RandomState(21)
    grid = np.stack(np.meshgrid(*[np.arange(6)] * 3, indexing="ij"), -1).reshape(-1, 3) / 8.0 - 0.25
    grid = grid[rs.permutation(len(grid))]
    for r in (0.125, 0.25, 0.125 * np.sqrt(2.0), 0.1249999):
        check_thin(grid, [0, len(grid)], [r])
    keep, _ = check_thin([[0, 0, 0], [0.375, 0.5, 0], [0.75, 1.0, 0.0], [0.375, 0.5, 0.0]], [0, 4], [0.625])       # 3-4-5: d == r
    assert keep.tolist() == [1, 0, 1, 0]
    on_axis, _ = check_thin(grid[np.argsort(grid @ [36, 6, 1], kind="stable")], [0, len(grid)], [0.125])
    assert 0 < on_axis.sum() < len(grid)


def test_thin_duplicates_and_a_zero_radius():
    rs = np.random.RandomState(22)
    base = rs.rand(90, 3)
    pts = base[rs.randint(0, 90, size=400)]
    keep, _ = check_thin(pts, [0, 400], [0.0])                              # only the later copies go
    first = np.zeros(400, dtype=bool)
    first[np.unique(pts, axis=0, return_index=True)[1]] = True
    assert np.array_equal(keep == 1, first)
    check_thin(pts, [0, 400], [0.15])
    same = np.tile([[0.25, -1.0, 3.0]], (70, 1))
    assert check_thin(same, [0, 70], [0.0])[0].tolist() == [1] + [0] * 69       # a box without extent and no radius: one cell


def test_thin_chain_that_needs_a_round_per_link():
    """257 points on a line, each within r of its neighbours on the line and of no other: the kept ones alternate, and point i
    waits for point i - 1.  A wavefront decides at most one of its links per launch, so the 64 links inside one take 64 rounds at
    least: beyond the 32 rounds of the first call, and the chain crosses the edge of a workgroup."""
    pts = np.stack([np.arange(257) * 1.0, np.zeros(257), np.zeros(257)], 1)
    keep, rounds = check_thin(pts, [0, 257], [1.5])
    assert keep.tolist() == [1, 0] * 128 + [1]
    print("chain of 257: %d rounds" % rounds)
    assert 64 <= rounds <= 257


def test_thin_everything_in_one_cell():
    """A second mesh of one point with a huge radius makes the cell edge larger than the box: all 300 points share a cell."""
    rs = np.random.RandomState(23)
    pts = np.concatenate([rs.rand(300, 3), [[0.5, 0.5, 0.5]]])
    keep, _ = check_thin(pts, [0, 300, 301], [0.12, 50.0])
    assert 20 < keep[:300].sum() < 300 and keep[300] == 1


def test_thin_points_on_cell_edges_at_negative_coordinates():
    rs = np.random.RandomState(24)
    lattice = -rs.randint(0, 20, size=(500, 3)) / 8.0                       # multiples of the radius: on the faces of the cells
    check_thin(lattice, [0, 500], [0.25])
    check_thin(lattice - 1e-9 * rs.rand(500, 3), [0, 500], [0.25])
    check_thin(-rs.rand(777, 3) * np.array([3.0, 0.01, 1.0]) - 5.0, [0, 777], [0.11])


def test_thin_meshes_do_not_interact():
    rs = np.random.RandomState(25)
    pts = rs.rand(300, 3)
    both = np.concatenate([pts, pts, pts])
    keep, _ = check_thin(both, [0, 300, 600, 900], [0.2, 0.05, 0.0])
    alone = [thin(pts, [0, 300], [r])[0] for r in (0.2, 0.05, 0.0)]
    assert np.array_equal(keep, np.concatenate(alone))
    assert keep[:300].sum() < keep[300:600].sum() < keep[600:].sum() == 300
    empty_between, _ = check_thin(both[:600], [0, 300, 300, 600], [0.2, 1.0, 0.2])
    assert np.array_equal(empty_between[:300], empty_between[300:])


@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257])
def test_thin_at_the_launch_edges(n):
    pts = cases.cube_surface_points(n, 40 + n)
    keep, _ = check_thin(pts, [0, n], [np.sqrt(6.0 / n)])
    assert keep[0] == 1


def test_thin_with_coarsened_cells():
    """Two clusters a million apart and a small radius: cells of the radius would be far more than the table holds."""
    rs = np.random.RandomState(26)
    pts = np.concatenate([rs.rand(400, 3), rs.rand(400, 3) + np.array([1e6, -2e5, 3e3])])[rs.permutation(800)]
    keep, _ = check_thin(pts, [0, 800], [0.05])
    assert 100 < keep.sum() < 800
    check_thin(pts, [0, 800], [0.0])


def test_thin_60000_cube_candidates():
    n = 60000
    pts = cases.cube_surface_points(n, 77)
    keep, rounds = check_thin(pts, [0, n], [np.sqrt(6.0 / n)])
    print("cube, %d candidates: %d kept, %d rounds" % (n, keep.sum(), rounds))
    assert keep.sum() > n // 3


def test_thin_refusals():
    pts = np.random.RandomState(27).rand(100, 3)
    for bad in (np.nan, np.inf, -np.inf):
        broken = pts.copy()
        broken[63, 1] = bad
        keep = torch.full((100,), 7, dtype=torch.int32, device="cuda")
        status = torch.full((3,), 7, dtype=torch.int32, device="cuda")
        ws = torch.empty(native.surface_thin_ws_bytes(100, 1), dtype=torch.uint8, device="cuda")
        native.surface_thin_wrapper(100, 1, dev(broken, np.float64), dev([0, 100], np.int32), dev([0.1], np.float64), 4, 0, keep, status, ws)
        assert status.tolist() == [1, 0, 0] and bool((keep == 7).all())         # the status set, keep untouched
        with pytest.raises(ValueError, match="not finite"):
            thin(broken, [0, 100], [0.1])
    for radius in ([-0.1], [np.nan], [np.inf]):
        with pytest.raises(ValueError, match="radius"):
            thin(pts, [0, 100], radius)
    with pytest.raises(ValueError, match="radius"):
        thin(pts, [0, 50, 100], [0.1, -1e-300])
    for offsets in ([0, 60, 40, 100], [0, 50, 99], [1, 50, 100]):
        with pytest.raises(ValueError, match="cand_offsets"):
            thin(pts, offsets, [0.1] * (len(offsets) - 1))
    with pytest.raises(ValueError):
        native.surface_thin_ws_bytes(2 ** 26 + 1, 1)
    assert native.surface_thin_ws_bytes(2 ** 26, 1) > 2 ** 26 * 8


# ---- nearest label ---------------------------------------------------------------------------------------------------------------

def check_nearest(query, source, labels):
    got_label, got_idx = mesh_ops.nearest_label(dev(query, np.float32), dev(source, np.float32), dev(labels, np.int32))
    want_label, want_idx = cases.nearest_label_reference(query, source, labels)
    assert got_idx.dtype == torch.int32 and got_label.dtype == torch.int32
    assert np.array_equal(got_idx.cpu().numpy(), want_idx)
    assert np.array_equal(got_label.cpu().numpy(), want_label)
    return want_idx


@pytest.mark.parametrize("ns", [1, 63, 64, 65, 2047, 2048, 2049])
def test_nearest_label_equals_cdist_argmin(ns):
    rs = np.random.RandomState(300 + ns)
    for batch in (1, 4):
        for nq in (1, 255, 257):
            source = rs.randn(batch, ns, 3).astype(np.float32)
            query = rs.randn(batch, nq, 3).astype(np.float32)
            query[:, 0] = source[:, ns // 2]                            # a query on a source point
            labels = rs.randint(0, 32768, size=(batch, ns))
            labels[:, -1] = 32767
            idx = check_nearest(query, source, labels)
            assert (idx[:, 0] == ns // 2).all()


def test_nearest_label_ties_take_the_first_index():
    """Lattice clouds: most queries have several nearest source points, many of them at distances whose squares differ and whose
    roots do not."""
    rs = np.random.RandomState(31)
    tied = 0
    for batch, nq, ns in ((1, 257, 2049), (4, 255, 700)):
        source = (rs.randint(-4, 5, size=(batch, ns, 3)) * 2).astype(np.float32) / 4
        query = (rs.randint(-4, 5, size=(batch, nq, 3)) * 2 + 1).astype(np.float32) / 4
        idx = check_nearest(query, source, rs.randint(0, 32768, size=(batch, ns)))
        from scipy.spatial.distance import cdist
        for b in range(batch):
            d = cdist(query[b], source[b])
            tied += int(((d == d.min(1, keepdims=True)).sum(1) > 1).sum())
            assert (idx[b] == np.argmax(d == d.min(1, keepdims=True), 1)).all()
    assert tied > (257 + 4 * 255) // 2
    big = (rs.rand(1, 300, 3) * 1000).astype(np.float32)             # large coordinates: squares that differ in the last bits only
    check_nearest(big + rs.randn(1, 300, 3).astype(np.float32) * 1e-3, np.concatenate([big, big], 1), rs.randint(0, 9, size=(1, 600)))


def test_nearest_label_shapes_and_refusals():
    q, s, l = torch.zeros(2, 0, 3, device="cuda"), torch.zeros(2, 5, 3, device="cuda"), torch.zeros(2, 5, dtype=torch.int32, device="cuda")
    label, idx = mesh_ops.nearest_label(q, s, l)
    assert label.shape == (2, 0) and idx.shape == (2, 0)
    with pytest.raises(ValueError):
        mesh_ops.nearest_label(torch.zeros(2, 4, 3, device="cuda"), s, l[:1])
    with pytest.raises(ValueError):
        mesh_ops.nearest_label(torch.zeros(2, 4, 3, device="cuda"), s[:, :0], l[:, :0])
    with pytest.raises(TypeError):
        mesh_ops.nearest_label(torch.zeros(2, 4, 3, device="cuda"), s, l.long())

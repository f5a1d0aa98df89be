"""ogc_depth_render / ogc_depth_points (csrc/depth_render.hip) through mesh_ops.depth_render and render_points against the
numpy float64 mirror of tests/depth_render_cases.py: the depth image equal in every bit, the face image in every entry, the cloud, its
pixels and its size likewise.  Images of 1 x 1, 7 x 5, 64 x 64 and 65 x 33; views whose projections are exact dyadic numbers for the
decided cases, and views where nothing is dyadic; small and large faces in one launch; the refusals; determinism."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import depth_render_cases as cases  # noqa: E402

from ogc_amd import pointnet2_cuda as native  # noqa: E402
from ogc_amd.data_prepare import mesh_ops  # noqa: E402


def two_planes_1024():
    """Two faces that fill 1024 x 768 and pass through each other: 2 x 12 288 blocks, more than the wavefronts of one launch."""
    view = cases.axis_view(512.0, 512.0, 384.0, 0.5, 64.0)
    return cases.scene(view, 1024, 768, [((-3000.0, -2000.0, 2.0), (5000.0, -1000.0, 8.0), (400.0, 6000.0, 4.0)),
                                         ((-3000.0, -1000.0, 8.0), (5000.0, -2000.0, 2.0), (600.0, 6000.0, 4.0))])


SCENES = {
    "no_centre": cases.no_centre, "no_centre_1x1": cases.no_centre_1x1, "one_centre": cases.one_centre, "vertex_on_centre": cases.vertex_on_centre,
    "shared_edge": cases.shared_edge, "shared_edge_swapped": lambda: cases.shared_edge(True), "coincident": cases.coincident,
    "crossing": cases.crossing, "degenerate": cases.degenerate, "far_outside_vertices": cases.far_outside_vertices,
    "far_outside_vertices_1x1": lambda: cases.far_outside_vertices(1, 1), "far_outside_vertices_64": lambda: cases.far_outside_vertices(64, 64),
    "wholly_outside": cases.wholly_outside, "behind_near": cases.behind_near, "empty": cases.empty_scene,
    "sphere_and_backdrop": cases.sphere_and_backdrop, "far_cut": cases.far_cut, "random": cases.random_scene,
    "random_64": lambda: cases.random_scene(seed=12, n_faces=500, width=64, height=64), "box_and_sphere": cases.box_and_sphere,
    "two_planes_1024": two_planes_1024,
}
_cache = {}


def scene_and_mirror(name):
    """The mirror of a scene, computed once and shared."""
    if name not in _cache:
        s = SCENES[name]()
        _cache[name] = (s, cases.mirror_render(s["vertices"], s["faces"], s["view"], s["width"], s["height"]))
    return _cache[name]


def as_view(doubles):
    return mesh_ops.View(tuple(doubles[0:3]), tuple(doubles[3:6]), tuple(doubles[6:9]), tuple(doubles[9:12]), *doubles[12:])


def upload(s):
    return torch.from_numpy(np.ascontiguousarray(s["vertices"], dtype=np.float64)).cuda(), torch.from_numpy(np.ascontiguousarray(s["faces"], dtype=np.int32)).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_images_and_cloud_equal_the_mirror(name):
    s, want = scene_and_mirror(name)
    vertices, faces = upload(s)
    view, width, height = as_view(s["view"]), s["width"], s["height"]
    depth, face, dropped = mesh_ops.depth_render(vertices, faces, view, width, height, return_dropped=True)
    assert depth.dtype == torch.float64 and face.dtype == torch.int32 and depth.shape == face.shape == (height, width) and depth.is_cuda
    depth, face = depth.cpu().numpy(), face.cpu().numpy()
    print(name, "covered", int((face >= 0).sum()), "depth bits differing", int((bits(depth) != bits(want["depth"])).sum()),
          "faces differing", int((face != want["face"]).sum()))
    assert np.array_equal(bits(depth), bits(want["depth"]))
    assert np.array_equal(face, want["face"])
    assert dropped == want["dropped_near"]
    points, pixel, face_of_point = mesh_ops.render_points(vertices, faces, view, width, height)
    assert points.dtype == torch.float32 and pixel.dtype == torch.int32 and face_of_point.dtype == torch.int32 and points.is_cuda
    assert points.shape == (len(want["pixel"]), 3) and pixel.shape == face_of_point.shape == (len(want["pixel"]),)
    assert np.array_equal(pixel.cpu().numpy(), want["pixel"]) and np.array_equal(face_of_point.cpu().numpy(), want["face_of_point"])
    assert np.array_equal(bits(points.cpu().numpy()), bits(want["points"]))


def test_the_decided_cases_are_what_they_claim():
    """What the mirror gives on the small scenes is pinned by hand in the CPU file; here: the scenes hold the work they are meant to."""
    assert len(scene_and_mirror("no_centre")[1]["pixel"]) == 0 and len(scene_and_mirror("one_centre")[1]["pixel"]) == 1
    edge = scene_and_mirror("shared_edge")[1]
    assert (edge["face"][2] == 0).all() and (edge["hits_per_pixel"][2] == 2).all() and (edge["face"] >= 0).all()
    assert (scene_and_mirror("far_outside_vertices")[1]["face"] == 0).all()
    assert scene_and_mirror("behind_near")[1]["dropped_near"] == 1
    sphere_scene, sphere = scene_and_mirror("sphere_and_backdrop")
    assert len(sphere_scene["faces"]) == 20001 and (sphere["face"] >= 0).all()
    assert 500 < (sphere["face"] < 20000).sum() < 1200 and len(np.unique(sphere["face"])) > 400        # a disc of small faces on the backdrop
    planes = scene_and_mirror("two_planes_1024")[1]
    assert (planes["hits_per_pixel"] == 2).all() and 0.1 < (planes["face"] == 0).mean() < 0.9


def test_mesh_idx_follows_face_offsets():
    s, want = scene_and_mirror("box_and_sphere")
    vertices, faces = upload(s)
    offsets = torch.from_numpy(s["face_offsets"]).cuda()
    points, pixel, face_of_point, mesh_idx = mesh_ops.render_points(vertices, faces, as_view(s["view"]), s["width"], s["height"], offsets)
    assert mesh_idx.dtype == torch.int32 and np.array_equal(mesh_idx.cpu().numpy(), (want["face_of_point"] >= s["face_offsets"][1]).astype(np.int32))
    assert set(mesh_idx.cpu().tolist()) == {0, 1} and np.array_equal(bits(points.cpu().numpy()), bits(want["points"]))


@pytest.mark.parametrize("name", ["sphere_and_backdrop", "crossing", "random"])
def test_two_calls_give_identical_bits(name):
    s, _ = scene_and_mirror(name)
    vertices, faces = upload(s)
    view = as_view(s["view"])
    first = [a.cpu().numpy() for a in mesh_ops.depth_render(vertices, faces, view, s["width"], s["height"])]
    first += [a.cpu().numpy() for a in mesh_ops.render_points(vertices, faces, view, s["width"], s["height"])]
    again = [a.cpu().numpy() for a in mesh_ops.depth_render(vertices, faces, view, s["width"], s["height"])]
    again += [a.cpu().numpy() for a in mesh_ops.render_points(vertices, faces, view, s["width"], s["height"])]
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()


def test_device_side_refusals_write_nothing():
    s, _ = scene_and_mirror("crossing")
    view, width, height = as_view(s["view"]), s["width"], s["height"]
    vertices, faces = upload(s)
    outside = faces.clone()
    outside[1, 2] = vertices.shape[0]
    negative = faces.clone()
    negative[0, 0] = -1
    nan, inf = vertices.clone(), vertices.clone()
    nan[4, 1] = float("nan")
    inf[0, 0] = float("-inf")
    for v, f, text, code in ((vertices, outside, "a face index outside the vertices", 1), (vertices, negative, "a face index outside the vertices", 1),
                             (nan, faces, "not finite", 2), (inf, faces, "not finite", 2), (nan, negative, "not finite", 2)):
        for fn in (mesh_ops.depth_render, mesh_ops.render_points):
            with pytest.raises(ValueError, match=text):
                fn(v, f, view, width, height)
        # the library itself: a code in the status, and not one word of the outputs touched
        depth = torch.full((height, width), -7.0, dtype=torch.float64, device="cuda")
        face = torch.full((height, width), -7, dtype=torch.int32, device="cuda")
        points = torch.full((height * width, 3), -7.0, dtype=torch.float32, device="cuda")
        pixel = torch.full((height * width,), -7, dtype=torch.int32, device="cuda")
        face_out = torch.full((height * width,), -7, dtype=torch.int32, device="cuda")
        status = torch.full((3,), -7, dtype=torch.int32, device="cuda")
        ws = torch.empty(native.depth_render_ws_bytes(f.shape[0]), dtype=torch.uint8, device="cuda")
        doubles = mesh_ops.view_doubles(view)
        native.depth_render_wrapper(v.shape[0], f.shape[0], v, f, doubles, width, height, depth, face, status, ws)
        native.depth_points_wrapper(width, height, doubles, depth, face, points, pixel, face_out, status)
        assert status.cpu().tolist()[0] == code and status.cpu().tolist()[1] == 0
        for t in (depth, face, points, pixel, face_out):
            assert (t == -7).all()
    # an unreferenced vertex is not looked at
    spare = torch.cat([vertices, torch.full((1, 3), float("nan"), dtype=torch.float64, device="cuda")])
    assert torch.equal(mesh_ops.depth_render(spare, faces, view, width, height)[1], mesh_ops.depth_render(vertices, faces, view, width, height)[1])


def test_host_side_refusals():
    s, _ = scene_and_mirror("crossing")
    view, width, height = as_view(s["view"]), s["width"], s["height"]
    vertices, faces = upload(s)
    offsets = torch.tensor([0, 2], dtype=torch.int32, device="cuda")
    for fn in (mesh_ops.depth_render, mesh_ops.render_points):
        with pytest.raises(TypeError, match="vertices must be torch.float64"):
            fn(vertices.float(), faces, view, width, height)
        with pytest.raises(TypeError, match="faces must be torch.int32"):
            fn(vertices, faces.long(), view, width, height)
        with pytest.raises(TypeError):
            fn(vertices.cpu().float(), faces, view, width, height)          # the type first, wherever the tensor lives
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            fn(vertices.cpu(), faces, view, width, height)
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            fn(vertices, faces.cpu(), view, width, height)
        with pytest.raises(RuntimeError, match="contiguous"):
            fn(vertices.t().contiguous().t(), faces, view, width, height)
        with pytest.raises(RuntimeError, match="contiguous"):
            fn(vertices, faces.t().contiguous().t(), view, width, height)
        with pytest.raises(ValueError, match=r"\(V, 3\)"):
            fn(vertices.reshape(-1), faces, view, width, height)
        with pytest.raises(ValueError, match=r"\(F, 3\)"):
            fn(vertices, faces.reshape(-1, 2), view, width, height)
        with pytest.raises(ValueError, match="1..16384"):
            fn(vertices, faces, view, 0, height)
        with pytest.raises(ValueError, match="1..16384"):
            fn(vertices, faces, view, width, 16385)
        for bad in (view._replace(f=0.0), view._replace(near=0.0), view._replace(far=view.near / 2), view._replace(cx=float("nan"))):
            with pytest.raises(native._lib.OgcOpsError, match="view"):
                fn(vertices, faces, bad, width, height)
        with pytest.raises(ValueError, match="3 numbers each"):
            fn(vertices, faces, view._replace(up=(0.0, 1.0)), width, height)
    with pytest.raises(TypeError, match="face_offsets must be torch.int32"):
        mesh_ops.render_points(vertices, faces, view, width, height, offsets.long())
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        mesh_ops.render_points(vertices, faces, view, width, height, offsets.cpu())
    with pytest.raises(RuntimeError, match="workspace"):
        native.depth_render_wrapper(vertices.shape[0], faces.shape[0], vertices, faces, mesh_ops.view_doubles(view), width, height,
                                    torch.empty(height, width, dtype=torch.float64, device="cuda"), torch.empty(height, width, dtype=torch.int32, device="cuda"),
                                    torch.empty(3, dtype=torch.int32, device="cuda"), torch.empty(64, dtype=torch.uint8, device="cuda"))


def test_timed_form_gives_the_same_images_and_three_times():
    s, want = scene_and_mirror("sphere_and_backdrop")
    vertices, faces = upload(s)
    width, height = s["width"], s["height"]
    depth = torch.empty(height, width, dtype=torch.float64, device="cuda")
    face = torch.empty(height, width, dtype=torch.int32, device="cuda")
    status = torch.empty(3, dtype=torch.int32, device="cuda")
    ws = torch.empty(native.depth_render_ws_bytes(faces.shape[0]), dtype=torch.uint8, device="cuda")
    ms = native.depth_render_timed_wrapper(vertices.shape[0], faces.shape[0], vertices, faces, s["view"].tolist(), width, height, depth, face, status, ws)
    assert len(ms) == 3 and all(0.0 <= m < 1000.0 for m in ms)
    assert status.cpu().tolist() == [0, 0, 0]
    assert np.array_equal(bits(depth.cpu().numpy()), bits(want["depth"])) and np.array_equal(face.cpu().numpy(), want["face"])


def test_runs_on_the_current_stream_and_waits_for_nothing():
    """Queued behind an upload on a side stream, read after that stream alone is synchronised."""
    s, want = scene_and_mirror("random")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        vertices, faces = upload(s)
        depth, face = mesh_ops.depth_render(vertices, faces, as_view(s["view"]), s["width"], s["height"])
    stream.synchronize()
    assert np.array_equal(bits(depth.cpu().numpy()), bits(want["depth"])) and np.array_equal(face.cpu().numpy(), want["face"])

"""The depth render of the OGC-DRSV preparation without a device: the numpy mirror of tests/depth_render_cases.py against
properties that do not depend on it — a plain Möller–Trumbore ray caster written here —, default_view against hand-computed values,
the ABI wiring of the new entry points, their host-side refusals, and the driver's argument errors."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import depth_render_cases as cases  # noqa: E402

INTERIOR = 1e-9         # barycentric coordinates at least this large: the ray hits the face's interior
REL = 1e-9


def ray_directions(view, width, height):
    """Per pixel the ray e + t * direction through its centre, t the depth along -back: (H * W, 3)."""
    _, right, up, back, f, cx, cy, _, _ = cases.split_view(view)
    py, px = np.divmod(np.arange(width * height), width)
    gx, gy = (px + 0.5 - cx) / f, -(py + 0.5 - cy) / f
    return gx[:, None] * right + gy[:, None] * up - back


def moller_trumbore(origin, directions, v0, v1, v2):
    """Rays against triangles, all (..., 3) and broadcast against each other -> t, u, v; nan where a ray is parallel to the plane."""
    e1, e2 = v1 - v0, v2 - v0
    pvec = np.cross(directions, e2)
    with np.errstate(all="ignore"):
        inv = 1.0 / (e1 * pvec).sum(-1)
        inv = np.where(np.isfinite(inv), inv, np.nan)
        tvec = origin - v0
        u = (tvec * pvec).sum(-1) * inv
        qvec = np.cross(tvec, e1)
        v = (directions * qvec).sum(-1) * inv
        t = (e2 * qvec).sum(-1) * inv
    return t, u, v


SCENES = {"random": cases.random_scene, "crossing": cases.crossing, "box_and_sphere": cases.box_and_sphere, "far_cut": cases.far_cut,
          "behind_near": cases.behind_near, "sphere_and_backdrop": lambda: cases.sphere_and_backdrop(n_around=30, n_rings=21)}


@pytest.fixture(scope="module")
def rendered():
    out = {}
    for name, make in SCENES.items():
        s = make()
        out[name] = (s, cases.mirror_render(s["vertices"], s["faces"], s["view"], s["width"], s["height"]))
    return out


@pytest.mark.parametrize("name", sorted(SCENES))
def test_mirror_against_a_ray_caster(rendered, name):
    s, got = rendered[name]
    view, width, height = s["view"], s["width"], s["height"]
    e, _, _, _, f, cx, cy, near, far = cases.split_view(view)
    assert got["code"] == 0
    tri = s["vertices"][s["faces"]]
    directions = ray_directions(view, width, height)
    depth, face = got["depth"].reshape(-1), got["face"].reshape(-1)
    pixel = got["pixel"]
    assert len(pixel) > 20 and np.array_equal(pixel, np.nonzero(face >= 0)[0]) and np.array_equal(got["face_of_point"], face[pixel])
    assert np.isinf(depth[face < 0]).all() and (depth[pixel] >= near).all() and (depth[pixel] <= far).all()

    # every produced point lies on the plane of its named face and inside it
    named = tri[face[pixel]]
    t, u, v = moller_trumbore(e, directions[pixel], named[:, 0], named[:, 1], named[:, 2])
    assert np.abs(t - depth[pixel]).max() <= REL * depth[pixel].max(), np.abs(t - depth[pixel]).max()
    assert min(u.min(), v.min(), (1 - u - v).min()) >= -REL

    # every produced point re-projects to its pixel centre, in float64 and, within the cast, as the float32 that is written
    py, px = np.divmod(pixel, width)
    for points, tol in ((e + depth[pixel, None] * directions[pixel], REL * max(width, height)),
                        (got["points"].astype(np.float64), 2.0 ** -22 * f * (np.abs(got["points"]).max() + np.abs(e).max()) / depth[pixel].min())):
        xc, yc, zc = cases.camera_coordinates(points, view)
        assert np.abs(cx + f * xc / zc - (px + 0.5)).max() <= tol and np.abs(cy - f * yc / zc - (py + 0.5)).max() <= tol
    assert got["points"].dtype == np.float32

    # no other face is hit nearer along the ray, and every centre whose ray hits an interior has a point
    _, _, zc = cases.camera_coordinates(tri, view)
    usable = ~(zc < near).any(1)                            # the near rule drops the others whole
    has_interior = np.zeros(width * height, dtype=bool)
    step = max(1, (1 << 20) // max(1, len(tri)))
    for lo in range(0, width * height, step):
        t, u, v = moller_trumbore(e, directions[lo:lo + step, None, :], tri[None, :, 0], tri[None, :, 1], tri[None, :, 2])
        with np.errstate(invalid="ignore"):
            interior = (u >= INTERIOR) & (v >= INTERIOR) & (1 - u - v >= INTERIOR) & usable[None]
            interior &= (t >= near * (1 + REL)) & (t <= far * (1 - REL))
        nearest = np.where(interior, t, np.inf).min(1)
        hit = np.isfinite(nearest)
        assert (depth[lo:lo + step][hit] <= nearest[hit] * (1 + REL)).all()
        assert np.isfinite(depth[lo:lo + step][hit]).all()
        has_interior[lo:lo + step] = hit
    only_the_mirror = int((~has_interior[pixel]).sum())      # covered centres on an edge, a vertex or a cut: not checked above
    assert only_the_mirror <= 0.02 * len(pixel), (only_the_mirror, len(pixel))


def test_mirror_on_the_decided_cases():
    """What the small scenes must give, stated by hand."""
    def render(s):
        return cases.mirror_render(s["vertices"], s["faces"], s["view"], s["width"], s["height"])
    assert len(render(cases.no_centre())["pixel"]) == 0 and len(render(cases.no_centre_1x1())["pixel"]) == 0
    one = render(cases.one_centre())
    assert one["pixel"].tolist() == [2 * 7 + 3] and one["depth"][2, 3] == 4.0 and one["points"].tolist() == [[0.0, 0.0, -4.0]]
    assert render(cases.vertex_on_centre())["pixel"].tolist() == [2 * 7 + 3]
    for swap in (False, True):
        edge = render(cases.shared_edge(swap))
        assert (edge["face"] >= 0).all() and (edge["depth"] == 4.0).all()          # no gaps
        assert (edge["hits_per_pixel"][2] == 2).all() and (edge["face"][2] == 0).all()          # the row on the edge: both, the lower wins
        assert (edge["hits_per_pixel"][[0, 1, 3, 4]] == 1).all() and len(edge["pixel"]) == 35
        assert (edge["face"][:2] == (1 if swap else 0)).all() and (edge["face"][3:] == (0 if swap else 1)).all()
    both = render(cases.coincident())
    assert (both["face"].max() == 0) and (both["hits_per_pixel"][both["face"] == 0] == 2).all() and (both["face"] == 0).sum() > 5
    cross = render(cases.crossing())
    assert {0, 1} <= set(np.unique(cross["face"])) and (cross["hits_per_pixel"] == 2).sum() > 500
    flat = render(cases.degenerate())
    assert set(np.unique(flat["face"])) == {-1, 2}
    full = render(cases.far_outside_vertices())
    assert (full["face"] == 0).all() and (full["depth"] == 4.0).all()
    assert (render(cases.far_outside_vertices(1, 1))["face"] == 0).all()
    assert len(render(cases.wholly_outside())["pixel"]) == 0
    near = render(cases.behind_near())
    assert near["dropped_near"] == 1 and set(np.unique(near["face"])) == {-1, 1}
    cut = render(cases.far_cut())
    assert 50 < len(cut["pixel"]) and cut["depth"][np.isfinite(cut["depth"])].max() <= 6.0
    uncut = dict(cases.far_cut(), view=cases.dyadic_view(65, 33, far=64.0))
    assert len(render(uncut)["pixel"]) > len(cut["pixel"]) + 50
    none = render(cases.empty_scene())
    assert len(none["pixel"]) == 0 and np.isinf(none["depth"]).all() and none["points"].shape == (0, 3)
    big = cases.sphere_and_backdrop()
    assert len(big["faces"]) == 20001
    bad = cases.one_centre()
    assert cases.mirror_render(bad["vertices"], [[0, 1, 3]], bad["view"], 7, 5) == {"code": 1}
    bad["vertices"][1, 2] = np.nan
    assert cases.mirror_render(bad["vertices"], bad["faces"], bad["view"], 7, 5) == {"code": 2}


def test_default_view_on_a_known_box():
    from ogc_amd.data_prepare.mesh_ops import default_view, view_doubles
    view = default_view((-1.0, -2.0, -3.0), (3.0, 0.0, -2.0))            # ext = 4, centre (1, -1, -2.5)
    distance = 0.7 * 4.0 / math.tan(math.radians(30.0))
    assert distance == pytest.approx(2.8 * math.sqrt(3.0), rel=1e-14)
    assert view.e[0] == 1.0 and view.e[1] == -1.0 and view.e[2] == pytest.approx(-2.5 + distance, rel=1e-14)      # on +z of the centre
    assert view.right == (1.0, 0.0, 0.0) and view.up == (0.0, 1.0, 0.0) and view.back == (0.0, 0.0, 1.0)
    assert view.f == pytest.approx(540.0 * math.sqrt(3.0), rel=1e-14) and (view.cx, view.cy) == (960.0, 540.0)
    assert view.near == pytest.approx(0.04, rel=1e-14) and view.far == pytest.approx(distance + 12.0, rel=1e-14)
    assert np.array_equal(view_doubles(view), cases.default_view_mirror((-1.0, -2.0, -3.0), (3.0, 0.0, -2.0)))
    # a zoom that puts the eye further away than 3 ext: near follows the distance; other sizes, explicit fields
    far = default_view((0, 0, 0), (1, 2, 1), width=160, height=90, fov_deg=20, zoom=1.0)
    distance = 2.0 / math.tan(math.radians(10.0))
    assert far.near == pytest.approx(distance - 6.0, rel=1e-14) and far.f == pytest.approx(45.0 / math.tan(math.radians(10.0)), rel=1e-14)
    assert np.array_equal(view_doubles(far), cases.default_view_mirror((0, 0, 0), (1, 2, 1), 160, 90, 20, 1.0))
    assert default_view((0, 0, 0), (1, 1, 1), near=0.5, cx=3.25)._replace(near=0, cx=0) == default_view((0, 0, 0), (1, 1, 1))._replace(near=0, cx=0)
    assert default_view((0, 0, 0), (1, 1, 1), near=0.5).near == 0.5
    # the box lies wholly in front of near and of far: the default view never drops a face
    for v, (lo, hi) in ((view, (-3.0, -2.0)), (far, (0.0, 1.0))):
        assert v.e[2] - hi >= v.near and v.e[2] - lo <= v.far
    for lo, hi, kw in (((0, 0, 0), (0, 0, 0), {}), ((0, 0, 1), (1, 1, 0), {}), ((0, 0, 0), (1, 1, float("inf")), {}),
                       ((0, 0, 0), (1, 1, 1), {"fov_deg": 180}), ((0, 0, 0), (1, 1, 1), {"zoom": 0}), ((0, 0, 0), (1, 1, 1), {"width": 0})):
        with pytest.raises(ValueError):
            default_view(lo, hi, **kw)
    with pytest.raises(TypeError):
        default_view((0, 0, 0), (1, 1, 1), focal=3.0)


@pytest.fixture(scope="module")
def lib():
    from ogc_amd.csrc import build as b
    L = ctypes.CDLL(b.build())
    L.ogc_last_error.restype = ctypes.c_char_p
    return L


def test_library_exports_the_entry_points(lib):
    from ogc_amd import _lib
    from ogc_amd import pointnet2_cuda as nat
    for name in ("ogc_depth_render", "ogc_depth_render_ws_bytes", "ogc_depth_points", "ogc_depth_render_timed"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    timed = _lib.SIGNATURES["ogc_depth_render_timed"]           # the same arguments and, in front of the stream, the host floats
    assert timed[:-2] == _lib.SIGNATURES["ogc_depth_render"][:-1] and timed[-2:] == [ctypes.c_void_p, ctypes.c_void_p]
    assert _lib.SIGNATURES["ogc_depth_render"][-1] is ctypes.c_void_p and len(_lib.SIGNATURES["ogc_depth_render"]) == 13
    assert _lib.SIGNATURES["ogc_depth_render"][-2] is ctypes.c_longlong
    assert _lib.SIGNATURES["ogc_depth_points"][-1] is ctypes.c_void_p and len(_lib.SIGNATURES["ogc_depth_points"]) == 10
    assert _lib.SIGNATURES["ogc_depth_render_ws_bytes"] == [ctypes.c_int]
    header = open(os.path.join(os.path.dirname(HERE), "include", "ogc_ops.h")).read()
    assert "int ogc_depth_render(int V, int F, const double *vertices, const int *faces, const double *view," in header
    assert "int ogc_depth_points(int width, int height, const double *view," in header
    assert "long long ogc_depth_render_ws_bytes(int F);" in header
    assert "#define OGC_DEPTH_VIEW_DOUBLES %d" % nat.DEPTH_VIEW_DOUBLES in header and nat.DEPTH_VIEW_DOUBLES == cases.VIEW_DOUBLES
    assert "int ogc_depth_render_timed(int V, int F, const double *vertices," in header
    assert all(callable(getattr(nat, n)) for n in ("depth_render_wrapper", "depth_points_wrapper", "depth_render_ws_bytes", "depth_render_timed_wrapper"))
    lib.ogc_depth_render_ws_bytes.restype = ctypes.c_longlong
    assert lib.ogc_depth_render_ws_bytes(-1) == -1 and lib.ogc_depth_render_ws_bytes((1 << 24) + 1) == -1
    sizes = [lib.ogc_depth_render_ws_bytes(f) for f in (0, 1, 256, 257, 100000)]
    assert sizes == sorted(sizes) and sizes[0] >= 0 and sizes[-1] >= 100000 * 128 and all(s % 256 == 0 for s in sizes)
    assert nat.depth_render_ws_bytes(257) == sizes[3]
    with pytest.raises(ValueError):
        nat.depth_render_ws_bytes((1 << 24) + 1)


def test_host_side_refusals_launch_nothing(lib):
    """Every argument check of the two entry points that needs no look at device memory: status and message, without a device."""
    from ogc_amd import _lib
    for name in ("ogc_depth_render", "ogc_depth_points"):
        getattr(lib, name).argtypes = _lib.SIGNATURES[name]
        getattr(lib, name).restype = ctypes.c_int
    good = cases.dyadic_view(7, 5)
    fake = ctypes.c_void_p(256)             # never dereferenced: every call below is refused before anything is queued

    def render(view=good, v=3, f=1, width=7, height=5, ws_bytes=1 << 20, ws=fake, depth=fake):
        arr = None if view is None else (ctypes.c_double * len(view))(*view)
        rc = lib.ogc_depth_render(v, f, fake, fake, arr, width, height, depth, fake, fake, ws, ws_bytes, None)
        return rc, lib.ogc_last_error().decode()

    def points(view=good, width=7, height=5, out=fake):
        arr = None if view is None else (ctypes.c_double * len(view))(*view)
        rc = lib.ogc_depth_points(width, height, arr, fake, fake, out, fake, fake, fake, None)
        return rc, lib.ogc_last_error().decode()

    def changed(index, value):
        view = good.copy()
        view[index] = value
        return view

    for call in (render, points):
        for kwargs, text in (({"width": 0}, "image"), ({"height": 16385}, "image"), ({"view": None}, "view"),
                             ({"view": changed(12, 0.0)}, "f > 0"), ({"view": changed(15, 0.0)}, "near"), ({"view": changed(16, 0.25)}, "near <= far"),
                             ({"view": changed(4, float("nan"))}, "view[4] is not finite"), ({"view": changed(0, float("inf"))}, "view[0]")):
            rc, message = call(**kwargs)
            assert rc == -1 and text in message, (call.__name__, kwargs, message)
    assert points(out=None)[0] == -1
    for kwargs, rc_want, text in (({"v": -1}, -1, "negative"), ({"f": -1}, -1, "negative"), ({"f": (1 << 24) + 1}, -3, "at most"),
                                  ({"ws_bytes": 128}, -1, "workspace"), ({"ws": ctypes.c_void_p(264)}, -1, "aligned"),
                                  ({"ws": None}, -1, "workspace"), ({"depth": None}, -1, "null")):
        rc, message = render(**kwargs)
        assert rc == rc_want and text in message, (kwargs, message)


def test_operators_have_no_cpu_path_and_check_types_first():
    from ogc_amd.data_prepare import mesh_ops
    s = cases.one_centre()
    view = mesh_ops.View(*np.split(s["view"][:12], 4), *s["view"][12:])
    vertices, faces = torch.from_numpy(s["vertices"]), torch.from_numpy(s["faces"])
    for fn in (mesh_ops.depth_render, mesh_ops.render_points):
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            fn(vertices, faces, view, 7, 5)
        with pytest.raises(TypeError, match="vertices must be torch.float64"):
            fn(vertices.float(), faces, view, 7, 5)
        with pytest.raises(TypeError, match="faces must be torch.int32"):
            fn(vertices, faces.long(), view, 7, 5)
        with pytest.raises(TypeError, match="must be a torch.Tensor"):
            fn(s["vertices"], faces, view, 7, 5)
    assert mesh_ops.view_doubles(view) == s["view"].tolist()
    from ogc_amd import data_prepare
    assert data_prepare.render_points is mesh_ops.render_points and data_prepare.default_view is mesh_ops.default_view


def test_driver_argument_errors(tmp_path):
    from ogc_amd.data_prepare import build_ogcdrsv
    roots = ["--src_root", str(tmp_path / "src"), "--dest_root", str(tmp_path / "dest")]
    for extra, text in ((["--width", "0"], "--width and --height"), (["--height", "20000"], "--width and --height"), (["--fov", "180"], "--fov"),
                        (["--fov", "0"], "--fov"), (["--zoom", "0"], "--zoom"), (["--synthetic", "-1"], "--synthetic")):
        with pytest.raises(ValueError, match=text):
            build_ogcdrsv.main(roots + extra)
    with pytest.raises(FileNotFoundError, match="mesh"):
        build_ogcdrsv.main(roots)
    with pytest.raises(SystemExit):
        build_ogcdrsv.main(["--src_root", str(tmp_path / "src")])
    assert not os.path.exists(str(tmp_path / "dest"))
    if not torch.cuda.is_available():
        os.makedirs(str(tmp_path / "src" / "mesh"))
        with pytest.raises(RuntimeError, match="no CPU path"):
            build_ogcdrsv.main(roots)

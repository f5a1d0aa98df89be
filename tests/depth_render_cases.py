"""Helpers of the depth-render tests (no tests here): a numpy float64 mirror of the contract of ogc_depth_render / ogc_depth_points
(include/ogc_ops.h), default_view's expression, and the scenes the CPU and the GPU files share.

The mirror repeats the contract's sequence operation by operation: numpy rounds every operation once and fuses nothing.  It is a
brute force over faces x pixel centres for small images.  One shortcut, inside the contract: a centre outside the closed bounding
interval of a face's screen vertices is not covered, so a face whose interval, widened by a pixel on every side, fits a window of
one of the PATCHES sizes is evaluated on that window only; every other face meets every centre of the image."""
import math

import numpy as np

VIEW_DOUBLES = 17
PATCHES = (6, 16, 48)
CHUNK = 1 << 22     # face x centre pairs evaluated at once


def view_array(e, right, up, back, f, cx, cy, near, far):
    return np.array([*e, *right, *up, *back, f, cx, cy, near, far], dtype=np.float64)


def axis_view(f, cx, cy, near, far, e=(0.0, 0.0, 0.0)):
    """The axis-aligned view: right = x, up = y, the camera looks along -z."""
    return view_array(e, (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), f, cx, cy, near, far)


def default_view_mirror(lo, hi, width=1920, height=1080, fov_deg=60, zoom=0.7):
    lo, hi = [float(x) for x in lo], [float(x) for x in hi]
    ext = max(h - l for l, h in zip(lo, hi))
    tan_half = math.tan(math.radians(fov_deg) / 2.0)
    distance = zoom * ext / tan_half
    lookat = [(l + h) / 2.0 for l, h in zip(lo, hi)]
    return view_array((lookat[0], lookat[1], lookat[2] + distance), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0),
                      (height / 2.0) / tan_half, width / 2.0, height / 2.0, max(0.01 * ext, distance - 3.0 * ext), distance + 3.0 * ext)


def split_view(view):
    view = np.asarray(view, dtype=np.float64)
    assert view.shape == (VIEW_DOUBLES,)
    return view[0:3], view[3:6], view[6:9], view[9:12], view[12], view[13], view[14], view[15], view[16]


def camera_coordinates(points, view):
    """(..., 3) world -> xc, yc, zc, the contract's sums left to right."""
    e, right, up, back = split_view(view)[:4]
    d0, d1, d2 = points[..., 0] - e[0], points[..., 1] - e[1], points[..., 2] - e[2]
    xc = (right[0] * d0 + right[1] * d1) + right[2] * d2
    yc = (up[0] * d0 + up[1] * d1) + up[2] * d2
    zc = -((back[0] * d0 + back[1] * d1) + back[2] * d2)
    return xc, yc, zc


def face_setup(vertices, faces, view):
    """-> (code, dict of per-face arrays).  code as status[0]; with a code set the dict is None."""
    vertices = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    _, _, _, _, f, cx, cy, near, far = split_view(view)
    bad_index = ((faces < 0) | (faces >= len(vertices))).any(1)
    safe = np.where(bad_index[:, None], 0, faces) if len(vertices) else np.zeros_like(faces)
    tri = vertices[safe] if len(vertices) else np.zeros((len(faces), 3, 3))
    not_finite = ~bad_index & ~np.isfinite(tri).all((1, 2))
    code = 2 if not_finite.any() else 1 if bad_index.any() else 0
    if code:
        return code, None
    with np.errstate(all="ignore"):
        xc, yc, zc = camera_coordinates(tri, view)                  # (F, 3) each
        dropped = (zc < near).any(1)
        sx = cx + f * (xc / zc)
        sy = cy - f * (yc / zc)
        finite = np.isfinite(xc).all(1) & np.isfinite(yc).all(1) & np.isfinite(zc).all(1) & np.isfinite(sx).all(1) & np.isfinite(sy).all(1)
        area = (sx[:, 1] - sx[:, 0]) * (sy[:, 2] - sy[:, 0]) - (sy[:, 1] - sy[:, 0]) * (sx[:, 2] - sx[:, 0])
        ux, uy, uz = xc[:, 1] - xc[:, 0], yc[:, 1] - yc[:, 0], zc[:, 1] - zc[:, 0]
        wx, wy, wz = xc[:, 2] - xc[:, 0], yc[:, 2] - yc[:, 0], zc[:, 2] - zc[:, 0]
        nx = uy * wz - uz * wy
        ny = uz * wx - ux * wz
        nz = ux * wy - uy * wx
        nc0 = (nx * xc[:, 0] + ny * yc[:, 0]) + nz * zc[:, 0]
    active = ~dropped & finite & ~(area == 0.0)
    return 0, {"sx": sx, "sy": sy, "n": np.stack([nx, ny, nz], 1), "nc0": nc0, "zmin": zc.min(1), "zmax": zc.max(1), "active": active,
               "dropped": dropped, "xc": xc, "yc": yc, "zc": zc}


def hits(rec, idx, qx, qy, view):
    """Faces idx (k,) against centres: qx, qy broadcastable to (k, m) -> (hit (k, m) bool, t (k, m))."""
    _, _, _, _, f, cx, cy, near, far = split_view(view)
    sx, sy = rec["sx"][idx], rec["sy"][idx]
    ax, ay, bx, by, c_x, c_y = (a[:, None] for a in (sx[:, 0], sy[:, 0], sx[:, 1], sy[:, 1], sx[:, 2], sy[:, 2]))
    with np.errstate(all="ignore"):
        inside = (qx >= sx.min(1)[:, None]) & (qx <= sx.max(1)[:, None]) & (qy >= sy.min(1)[:, None]) & (qy <= sy.max(1)[:, None])
        e0 = (bx - ax) * (qy - ay) - (by - ay) * (qx - ax)
        e1 = (c_x - bx) * (qy - by) - (c_y - by) * (qx - bx)
        e2 = (ax - c_x) * (qy - c_y) - (ay - c_y) * (qx - c_x)
        covered = ((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0))
        gx = (qx - cx) / f
        gy = -((qy - cy) / f)
        n = rec["n"][idx]
        ng = (n[:, 0:1] * gx + n[:, 1:2] * gy) + n[:, 2:3]
        t = rec["nc0"][idx][:, None] / ng
        ok = inside & covered & ~(ng == 0.0) & np.isfinite(t)
        t = np.minimum(np.maximum(t, rec["zmin"][idx][:, None]), rec["zmax"][idx][:, None])
        ok &= (t >= near) & (t <= far)
    return ok, t


def mirror_render(vertices, faces, view, width, height):
    """-> dict: code, dropped_near, depth (H, W) float64 (+inf: no hit), face (H, W) int32 (-1), and the cloud of the covered pixels
    in row-major order: points (P, 3) float32, pixel (P,) int32, face_of_point (P,) int32.  With a code set only code is there."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    code, rec = face_setup(vertices, faces, view)
    if code:
        return {"code": code}
    n_pixel = width * height
    found = [np.zeros((0,), np.int64)], [np.zeros((0,), np.float64)], [np.zeros((0,), np.int64)]     # pixel, t, face

    def collect(idx, px, py, ok, t):
        k, m = np.nonzero(ok)
        found[0].append((np.broadcast_to(py, ok.shape)[k, m] * width + np.broadcast_to(px, ok.shape)[k, m]).astype(np.int64))
        found[1].append(t[k, m])
        found[2].append(idx[k])

    active = np.nonzero(rec["active"])[0]
    if len(active):
        sx, sy = rec["sx"][active], rec["sy"][active]
        x0, y0 = np.floor(sx.min(1) - 0.5) - 1, np.floor(sy.min(1) - 0.5) - 1
        x1, y1 = np.ceil(sx.max(1) - 0.5) + 1, np.ceil(sy.max(1) - 0.5) + 1
        extent = np.maximum(x1 - x0, y1 - y0) + 1
        rest = np.ones(len(active), dtype=bool)
        for patch in PATCHES:
            small = rest & (extent <= patch)
            rest &= ~small
            idx = active[small]
            if len(idx) == 0:
                continue
            oy, ox = np.divmod(np.arange(patch * patch), patch)
            # the window may lie anywhere, also far outside the image: clip before the cast
            px = np.clip(x0[small], -2 - patch, width + 1)[:, None].astype(np.int64) + ox[None]
            py = np.clip(y0[small], -2 - patch, height + 1)[:, None].astype(np.int64) + oy[None]
            for lo in range(0, len(idx), CHUNK // (patch * patch)):
                part = slice(lo, lo + CHUNK // (patch * patch))
                ok, t = hits(rec, idx[part], px[part] + 0.5, py[part] + 0.5, view)
                ok &= (px[part] >= 0) & (px[part] < width) & (py[part] >= 0) & (py[part] < height)
                collect(idx[part], px[part], py[part], ok, t)
        idx = active[rest]
        py, px = np.divmod(np.arange(n_pixel), width)
        step = max(1, CHUNK // n_pixel)
        for lo in range(0, len(idx), step):
            ok, t = hits(rec, idx[lo:lo + step], (px + 0.5)[None], (py + 0.5)[None], view)
            collect(idx[lo:lo + step], px[None], py[None], ok, t)
    pix, t, fid = (np.concatenate(a) for a in found)
    order = np.lexsort((fid, t, pix))                      # by pixel, then depth, then face index
    pix, t, fid = pix[order], t[order], fid[order]
    first = np.ones(len(pix), dtype=bool)
    first[1:] = pix[1:] != pix[:-1]
    depth = np.full(n_pixel, np.inf)
    face = np.full(n_pixel, -1, dtype=np.int32)
    depth[pix[first]] = t[first]
    face[pix[first]] = fid[first]
    out = {"code": 0, "dropped_near": int(rec["dropped"].sum()), "depth": depth.reshape(height, width), "face": face.reshape(height, width),
           "hits_per_pixel": np.bincount(pix, minlength=n_pixel).reshape(height, width)}
    out["points"], out["pixel"], out["face_of_point"] = mirror_points(depth, face, view, width)
    return out


def mirror_points(depth, face, view, width):
    e, right, up, back, f, cx, cy, _, _ = split_view(view)
    pixel = np.nonzero(face.reshape(-1) >= 0)[0]
    py, px = np.divmod(pixel, width)
    qx, qy = px + 0.5, py + 0.5
    gx = (qx - cx) / f
    gy = -((qy - cy) / f)
    t = depth.reshape(-1)[pixel]
    points = np.stack([e[k] + t * ((gx * right[k] + gy * up[k]) - back[k]) for k in range(3)], 1).astype(np.float32)
    return points.reshape(-1, 3), pixel.astype(np.int32), face.reshape(-1)[pixel].astype(np.int32)


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
def world(view, sx, sy, zc):
    """The world point that projects to (sx, sy) at depth zc.  Exact for an axis-aligned view with dyadic numbers."""
    e, right, up, back, f, cx, cy, _, _ = split_view(view)
    xc, yc = (sx - cx) * zc / f, -(sy - cy) * zc / f
    return e + xc * right + yc * up - zc * back


def scene(view, width, height, triangles):
    """triangles: [((sx, sy, zc), (sx, sy, zc), (sx, sy, zc))] in screen coordinates and depth -> a scene with its own vertices."""
    vertices = np.array([world(view, *corner) for tri in triangles for corner in tri], dtype=np.float64).reshape(-1, 3)
    faces = np.arange(len(vertices), dtype=np.int32).reshape(-1, 3)
    return {"vertices": vertices, "faces": faces, "view": view, "width": width, "height": height}


def dyadic_view(width, height, near=0.5, far=64.0):
    """f = 8 and geometry at zc = 4: sx = cx + 2 xc exactly."""
    return axis_view(8.0, width / 2.0, height / 2.0, near, far)


def no_centre(width=7, height=5):
    return scene(dyadic_view(width, height), width, height, [((3.625, 2.625, 4.0), (3.875, 2.625, 4.0), (3.75, 2.875, 4.0))])


def no_centre_1x1():
    return scene(dyadic_view(1, 1), 1, 1, [((0.625, 0.125, 4.0), (0.875, 0.125, 4.0), (0.75, 0.375, 4.0))])


def one_centre():
    return scene(dyadic_view(7, 5), 7, 5, [((3.0, 2.0, 4.0), (4.0, 2.25, 4.0), (3.5, 3.0, 4.0))])


def vertex_on_centre():
    return scene(dyadic_view(7, 5), 7, 5, [((3.5, 2.5, 4.0), (3.875, 2.625, 4.0), (3.625, 2.875, 4.0))])


def shared_edge(swap=False):
    """Two faces of one plane that share the edge sy = 2.5, which runs through the centres of row 2."""
    upper = ((-20.0, 2.5, 4.0), (27.0, 2.5, 4.0), (3.5, -30.0, 4.0))
    lower = ((27.0, 2.5, 4.0), (-20.0, 2.5, 4.0), (3.5, 35.0, 4.0))
    return scene(dyadic_view(7, 5), 7, 5, [lower, upper] if swap else [upper, lower])


def coincident():
    tri = ((1.0, 0.25, 4.0), (6.5, 1.0, 4.0), (2.25, 4.75, 4.0))
    return scene(dyadic_view(7, 5), 7, 5, [tri, tri])


def crossing():
    """Two faces that pass through each other: one recedes to the right, the other to the left."""
    a = ((2.0, 2.0, 2.0), (62.0, 3.0, 8.0), (30.0, 61.0, 5.0))
    b = ((2.0, 3.0, 8.0), (62.0, 2.0, 2.0), (34.0, 60.0, 5.0))
    return scene(dyadic_view(64, 64), 64, 64, [a, b])


def degenerate():
    """A face with zero screen area (collinear), one with two equal vertices, one seen edge-on (its plane holds the eye), and an
    ordinary one so that the image is not empty."""
    view = dyadic_view(7, 5)
    s = scene(view, 7, 5, [((0.5, 0.5, 4.0), (3.5, 2.5, 4.0), (6.5, 4.5, 4.0)), ((1.5, 1.5, 4.0), (1.5, 1.5, 4.0), (5.5, 3.5, 4.0)),
                           ((5.0, 0.25, 4.0), (6.25, 0.5, 4.0), (5.5, 1.75, 4.0))])
    edge_on = np.array([[0.0, -1.0, -2.0], [0.0, 1.0, -4.0], [0.0, 0.5, -8.0]])        # xc = 0 everywhere: the column sx = cx
    s["vertices"] = np.concatenate([s["vertices"], edge_on])
    s["faces"] = np.concatenate([s["faces"], [[9, 10, 11]]]).astype(np.int32)
    return s


def far_outside_vertices(width=65, height=33):
    """One face whose vertices lie far outside the image on every side: every centre is covered."""
    return scene(dyadic_view(width, height), width, height, [((-4096.0, -2048.0, 4.0), (8192.0, -1024.0, 4.0), (32.0, 16384.0, 4.0))])


def wholly_outside():
    return scene(dyadic_view(64, 64), 64, 64, [((100.0, 10.0, 4.0), (120.0, 12.0, 4.0), (110.0, 40.0, 4.0)),
                                               ((-50.0, -20.0, 4.0), (-10.0, -30.0, 4.0), (-20.0, -2.0, 4.0)),
                                               ((10.0, 70.0, 4.0), (50.0, 80.0, 4.0), (20.0, 90.0, 4.0))])


def behind_near():
    """Face 0 has one vertex behind near = 1 and is dropped whole; face 1 is ordinary."""
    view = dyadic_view(65, 33, near=1.0)
    s = scene(view, 65, 33, [((10.0, 4.0, 4.0), (50.0, 6.0, 4.0), (30.0, 30.0, 4.0)), ((20.0, 8.0, 8.0), (60.0, 10.0, 8.0), (41.0, 28.0, 8.0))])
    s["vertices"][2] = [0.0, -1.0, -0.5]       # zc = 0.5 < near
    return s


def far_cut():
    """A face that recedes from zc = 2 to zc = 16 under far = 6: its far part is cut pixel by pixel."""
    view = dyadic_view(65, 33, far=6.0)
    return scene(view, 65, 33, [((1.0, 1.0, 2.0), (64.0, 2.0, 16.0), (30.0, 32.0, 8.0))])


def empty_scene():
    return {"vertices": np.zeros((0, 3)), "faces": np.zeros((0, 3), dtype=np.int32), "view": dyadic_view(7, 5), "width": 7, "height": 5}


def uv_sphere(centre, radius, n_around, n_rings):
    """A closed sphere of 2 n_around (n_rings - 1) triangles."""
    vertices = [[0.0, 1.0, 0.0]]
    for r in range(1, n_rings):
        polar = math.pi * r / n_rings
        vertices += [[math.sin(polar) * math.cos(2 * math.pi * s / n_around), math.cos(polar), math.sin(polar) * math.sin(2 * math.pi * s / n_around)]
                     for s in range(n_around)]
    vertices.append([0.0, -1.0, 0.0])
    last = len(vertices) - 1
    faces = []
    for s in range(n_around):
        t = (s + 1) % n_around
        faces.append([0, 1 + t, 1 + s])
        for r in range(n_rings - 2):
            u, v = 1 + r * n_around, 1 + (r + 1) * n_around
            faces += [[u + s, u + t, v + t], [u + s, v + t, v + s]]
        faces.append([last, last - n_around + s, last - n_around + t])
    return np.asarray(vertices) * radius + np.asarray(centre, dtype=np.float64), np.asarray(faces, dtype=np.int32)


def sphere_and_backdrop(width=128, height=96, n_around=100, n_rings=101):
    """A sphere of 2 n_around (n_rings - 1) faces, each smaller than a pixel, in front of one face that fills the screen: small and
    large work in one launch.  The default sizes give 20 000 + 1 faces."""
    view = axis_view(64.0, width / 2.0 + 0.25, height / 2.0 - 0.125, 0.5, 64.0)
    vertices, faces = uv_sphere((0.0625, -0.03125, -4.0), 1.0, n_around, n_rings)      # 32 pixels across: 100 faces around
    back = scene(view, width, height, [((-300.0, -200.0, 16.0), (700.0, -100.0, 16.0), (50.0, 900.0, 16.0))])
    return {"vertices": np.concatenate([vertices, back["vertices"]]), "faces": np.concatenate([faces, back["faces"] + len(vertices)]).astype(np.int32),
            "view": view, "width": width, "height": height}


def random_scene(seed=11, n_faces=300, width=65, height=33):
    """Triangles of every size under a turned view with a focal length that is no power of two: nothing here is dyadic."""
    rs = np.random.RandomState(seed)
    a, b = 0.3, -0.2
    ry = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    rx = np.array([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
    frame = ry @ rx                                       # columns: right, up, back (orthonormal up to rounding)
    e = np.array([0.3, -0.2, 5.0])
    view = view_array(e, frame[:, 0], frame[:, 1], frame[:, 2], 37.3, width / 2.0 - 0.3, height / 2.0 + 0.7, 0.25, 9.0)
    centres = world(view, rs.rand(n_faces, 1) * (width + 20) - 10, rs.rand(n_faces, 1) * (height + 20) - 10, 1.0 + rs.rand(n_faces, 1) * 9.0)
    size = np.where(rs.rand(n_faces, 1, 1) < 0.7, 0.05, 1.5)
    vertices = (centres[:, None, :] + (rs.rand(n_faces, 3, 3) - 0.5) * size).reshape(-1, 3)
    return {"vertices": vertices, "faces": np.arange(3 * n_faces, dtype=np.int32).reshape(-1, 3), "view": view, "width": width, "height": height}


def box_and_sphere(width=48, height=40):
    """Two closed meshes, one partly hidden behind the other, under the default view of their bounding box."""
    sphere, sphere_faces = uv_sphere((0.02, 0.01, 0.05), 0.06, 12, 8)
    lo, hi = np.array([-0.09, -0.05, -0.08]), np.array([0.03, 0.06, 0.0])
    corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    box_faces = np.array([t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], dtype=np.int32)
    vertices = np.concatenate([sphere, corners])
    view = default_view_mirror(vertices.min(0), vertices.max(0), width, height)
    return {"vertices": vertices, "faces": np.concatenate([sphere_faces, box_faces + len(sphere)]).astype(np.int32), "view": view, "width": width,
            "height": height, "face_offsets": np.array([0, len(sphere_faces), len(sphere_faces) + len(box_faces)], dtype=np.int32)}

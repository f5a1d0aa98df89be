"""The device operators of the OGC-DR preparation (csrc/surface_candidates.hip, csrc/surface_thin.hip, csrc/nearest_label.hip;
DESIGN §4m): random points on mesh surfaces, their thinning to an even sampling, and the label transfer of the single-view set.
Inputs are CUDA tensors and results stay on the device; the host reads a status word per call (and, in sample_surface_even, the
areas it needs for the radii, which it computes itself).  There is no CPU path.
The depth render of the OGC-DRSV preparation (csrc/depth_render.hip) is here too: default_view, depth_render and
render_points.  So is the scene composition of build_ogcdr (csrc/room_compose.hip): compose_rooms and apply_poses."""
import collections
import math

import numpy as np
import torch

from .. import pointnet2_cuda as _native

CANDIDATE_STATUS = {1: "a face index outside the vertices", 2: "offsets that do not start at 0, descend or do not end at the array sizes",
                    3: "a mesh with candidates whose area is not a positive finite number"}
THIN_STATUS = {1: "a coordinate that is not finite", 2: "a radius that is negative or not finite",
               3: "cand_offsets that do not start at 0, descend or do not end at the number of points"}
THIN_FIRST_ROUNDS = 32      # rounds queued before the first read of the status
THIN_MAX_ROUNDS = 1024      # per call afterwards; every continuation doubles up to here


def _check_tensors(tensors):
    """tensors: (tensor, name, dtype).  Types first, so that a wrong dtype is a TypeError wherever the tensors live."""
    for t, name, dtype in tensors:
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor" % name)
        if t.dtype != dtype:
            raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    for t, name, _ in tensors:
        if t.device.type != "cuda":
            raise RuntimeError("%s must be a CUDA tensor (HIP device); ogc_amd has no CPU path" % name)


def _check_contiguous(tensors):
    for t, name, _ in tensors:
        if not t.is_contiguous():
            raise RuntimeError("%s must be contiguous" % name)


def face_areas(vertices, faces):
    """numpy: vertices (V, 3) float64, faces (F, 3) integers -> (F,) float64, 0.5 * |cross(v1 - v0, v2 - v0)|: the definition of the
    areas behind cum_area."""
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces)
    return 0.5 * np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1)


def cumulative_areas(vertices, faces, face_offsets):
    """numpy: the running sum of the face areas per mesh, restarting at every mesh -> (cum_area (F,) float64, area (M,) float64)."""
    areas = face_areas(vertices, faces)
    cum = np.zeros(areas.shape[0], dtype=np.float64)
    total = np.zeros(len(face_offsets) - 1, dtype=np.float64)
    for m in range(len(face_offsets) - 1):
        lo, hi = int(face_offsets[m]), int(face_offsets[m + 1])
        if hi > lo:
            cum[lo:hi] = np.cumsum(areas[lo:hi])
            total[m] = cum[hi - 1]
    return cum, total


def surface_candidates(vertices, faces, cum_area, face_offsets, cand_offsets, seed):
    """Area-weighted random points on the triangles of M concatenated meshes: vertices (V, 3) fp64, faces (F, 3) int32 indexing
    them, cum_area (F,) fp64 (cumulative_areas), face_offsets and cand_offsets (M + 1,) int32, CUDA tensors; seed an integer
    -> (points (C, 3) fp64, face_idx (C,) int32) on the device, C = cand_offsets[-1].  Candidate j of mesh m depends on
    (seed, m, j) and on its mesh alone (include/ogc_ops.h: ogc_surface_candidates).  One host read: the status word."""
    tensors = ((vertices, "vertices", torch.float64), (faces, "faces", torch.int32), (cum_area, "cum_area", torch.float64),
               (face_offsets, "face_offsets", torch.int32), (cand_offsets, "cand_offsets", torch.int32))
    _check_tensors(tensors)
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError("vertices must be (V, 3), got %s" % (tuple(vertices.shape),))
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError("faces must be (F, 3), got %s" % (tuple(faces.shape),))
    if tuple(cum_area.shape) != (faces.shape[0],):
        raise ValueError("cum_area must be (%d,), got %s" % (faces.shape[0], tuple(cum_area.shape)))
    if face_offsets.dim() != 1 or face_offsets.shape[0] < 1 or tuple(cand_offsets.shape) != tuple(face_offsets.shape):
        raise ValueError("face_offsets and cand_offsets must both be (M + 1,), got %s and %s"
                         % (tuple(face_offsets.shape), tuple(cand_offsets.shape)))
    _check_contiguous(tensors)
    n_mesh = face_offsets.shape[0] - 1
    total = int(cand_offsets[-1].item())
    if total < 0:
        raise ValueError("cand_offsets ends at %d" % total)
    points = torch.empty(total, 3, dtype=torch.float64, device=vertices.device)
    face_idx = torch.empty(total, dtype=torch.int32, device=vertices.device)
    if total == 0:
        return points, face_idx
    status = torch.empty(1, dtype=torch.int32, device=vertices.device)
    _native.surface_candidates_wrapper(total, n_mesh, vertices.shape[0], faces.shape[0], vertices, faces, cum_area, face_offsets,
                                       cand_offsets, seed, points, face_idx, status)
    code = int(status.item())
    if code:
        raise ValueError("surface_candidates: " + CANDIDATE_STATUS.get(code, "status %d" % code))
    return points, face_idx


def surface_thin(points, cand_offsets, radius, return_rounds=False):
    """First-come greedy thinning, exact: points (C, 3) fp64, cand_offsets (M + 1,) int32, radius (M,) fp64, CUDA tensors
    -> keep (C,) int32 on the device (with return_rounds: and the number of rounds that decided something).

    The definition is sequential and is this package's contract: walking a mesh's candidates in index order, candidate i is kept
    iff no KEPT candidate j < i of the same mesh has ((dx*dx) + (dy*dy)) + (dz*dz) <= r * r in fp64, the bound inclusive as in
    cKDTree.query_pairs(r).  It is the rule trimesh.sample.sample_surface_even documents as rejection sampling; trimesh itself is
    not what the result is pinned to.  Candidates of different meshes never interact.  The device evaluates it in rounds
    (csrc/surface_thin.hip); the host reads the status once per 32 rounds, then per doubling batch, and continues while
    candidates are undecided."""
    tensors = ((points, "points", torch.float64), (cand_offsets, "cand_offsets", torch.int32), (radius, "radius", torch.float64))
    _check_tensors(tensors)
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("points must be (C, 3), got %s" % (tuple(points.shape),))
    if cand_offsets.dim() != 1 or cand_offsets.shape[0] < 1:
        raise ValueError("cand_offsets must be (M + 1,), got %s" % (tuple(cand_offsets.shape),))
    n_mesh = cand_offsets.shape[0] - 1
    if tuple(radius.shape) != (n_mesh,):
        raise ValueError("radius must be (%d,), got %s" % (n_mesh, tuple(radius.shape)))
    _check_contiguous(tensors)
    total = points.shape[0]
    keep = torch.empty(total, dtype=torch.int32, device=points.device)
    if total == 0:
        return (keep, 0) if return_rounds else keep
    ws = torch.empty(_native.surface_thin_ws_bytes(total, n_mesh), dtype=torch.uint8, device=points.device)
    status = torch.empty(3, dtype=torch.int32, device=points.device)
    rounds, done = THIN_FIRST_ROUNDS, 0
    while True:
        _native.surface_thin_wrapper(total, n_mesh, points, cand_offsets, radius, rounds, done, keep, status, ws)
        done += rounds
        code, left, used = (int(v) for v in status.cpu())
        if code:
            raise ValueError("surface_thin: " + THIN_STATUS.get(code, "status %d" % code))
        if left == 0:
            return (keep, used) if return_rounds else keep
        rounds = min(2 * rounds, THIN_MAX_ROUNDS)


def nearest_label(query, source, labels):
    """Per query point the label and the index of its nearest source point, `labels[cdist(query, source).argmin(1)]`
    (collect_segm.py:59-61): query (B, Nq, 3), source (B, Ns, 3) fp32, labels (B, Ns) int32, CUDA tensors
    -> (out_label (B, Nq) int32, out_idx (B, Nq) int32) on the device.  Distances are cdist's fp64 expression; the first index
    among equal minima wins."""
    tensors = ((query, "query", torch.float32), (source, "source", torch.float32), (labels, "labels", torch.int32))
    _check_tensors(tensors)
    if query.dim() != 3 or query.shape[2] != 3:
        raise ValueError("query must be (B, Nq, 3), got %s" % (tuple(query.shape),))
    batch, nq = query.shape[0], query.shape[1]
    if source.dim() != 3 or source.shape[0] != batch or source.shape[2] != 3:
        raise ValueError("source must be (%d, Ns, 3), got %s" % (batch, tuple(source.shape)))
    ns = source.shape[1]
    if tuple(labels.shape) != (batch, ns):
        raise ValueError("labels must be (%d, %d), got %s" % (batch, ns, tuple(labels.shape)))
    if ns < 1 and batch * nq > 0:
        raise ValueError("source holds no points")
    _check_contiguous(tensors)
    out_label = torch.empty(batch, nq, dtype=torch.int32, device=query.device)
    out_idx = torch.empty(batch, nq, dtype=torch.int32, device=query.device)
    if batch * nq > 0:
        _native.nearest_label_wrapper(batch, nq, ns, query, source, labels, out_label, out_idx)
    return out_label, out_idx


RENDER_STATUS = {1: "a face index outside the vertices", 2: "a vertex coordinate that is not finite"}

View = collections.namedtuple("View", "e right up back f cx cy near far")
View.__doc__ = """A pinhole view (include/ogc_ops.h: ogc_depth_render): eye e, the orthonormal right, up and back (the camera looks along
-back), focal length f in pixels, principal point (cx, cy), near and far.  Plain Python floats; the library receives doubles."""


def view_doubles(view):
    """The 17 doubles of a View in the order the library takes them."""
    vals = [float(x) for x in (*view.e, *view.right, *view.up, *view.back, view.f, view.cx, view.cy, view.near, view.far)]
    if len(vals) != _native.DEPTH_VIEW_DOUBLES:
        raise ValueError("e, right, up and back are 3 numbers each")
    return vals


def default_view(lo, hi, width=1920, height=1080, fov_deg=60, zoom=0.7, **fields):
    """The view build_ogcdrsv renders a frame with, from the bounding box [lo, hi] of the rendered vertices: lookat the centre of the
    box, front (0, 0, 1), up (0, 1, 0), ext the longest edge, distance = zoom * ext / tan(fov / 2), the eye at lookat + front *
    distance, the field of view vertical: f = (height / 2) / tan(fov / 2), the principal point the image centre,
    near = max(0.01 * ext, distance - 3 * ext), far = distance + 3 * ext.  It restates open3d's ViewControl defaults as far as they
    are known and has NOT been compared with open3d.  Any field of View can be given by keyword and then replaces the default.  The
    trigonometry runs here, in Python floats."""
    lo = [float(x) for x in lo]
    hi = [float(x) for x in hi]
    if len(lo) != 3 or len(hi) != 3 or not all(math.isfinite(a) and math.isfinite(b) and a <= b for a, b in zip(lo, hi)):
        raise ValueError("lo and hi must be 3 finite numbers each with lo <= hi, got %s and %s" % (lo, hi))
    if width < 1 or height < 1 or not 0.0 < fov_deg < 180.0 or not zoom > 0.0:
        raise ValueError("width and height must be >= 1, fov_deg in (0, 180) and zoom > 0")
    ext = max(h - l for l, h in zip(lo, hi))
    if not ext > 0.0:
        raise ValueError("the bounding box has no extent")
    tan_half = math.tan(math.radians(fov_deg) / 2.0)
    distance = zoom * ext / tan_half
    lookat = [(l + h) / 2.0 for l, h in zip(lo, hi)]
    view = View(e=(lookat[0], lookat[1], lookat[2] + distance), right=(1.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), back=(0.0, 0.0, 1.0),
                f=(height / 2.0) / tan_half, cx=width / 2.0, cy=height / 2.0, near=max(0.01 * ext, distance - 3.0 * ext),
                far=distance + 3.0 * ext)
    unknown = set(fields) - set(View._fields)
    if unknown:
        raise TypeError("default_view: unknown fields %s" % sorted(unknown))
    return view._replace(**fields)


def _check_mesh(vertices, faces):
    tensors = ((vertices, "vertices", torch.float64), (faces, "faces", torch.int32))
    _check_tensors(tensors)
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError("vertices must be (V, 3), got %s" % (tuple(vertices.shape),))
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError("faces must be (F, 3), got %s" % (tuple(faces.shape),))
    _check_contiguous(tensors)


def _check_image(width, height):
    if not (1 <= int(width) <= 16384 and 1 <= int(height) <= 16384):
        raise ValueError("width and height must be in 1..16384, got %s x %s" % (width, height))
    return int(width), int(height)


def _render(vertices, faces, doubles, width, height):
    depth = torch.empty(height, width, dtype=torch.float64, device=vertices.device)
    face = torch.empty(height, width, dtype=torch.int32, device=vertices.device)
    status = torch.empty(3, dtype=torch.int32, device=vertices.device)
    ws = torch.empty(_native.depth_render_ws_bytes(faces.shape[0]), dtype=torch.uint8, device=vertices.device)
    _native.depth_render_wrapper(vertices.shape[0], faces.shape[0], vertices, faces, doubles, width, height, depth, face, status, ws)
    return depth, face, status


def _render_status(name, status):
    code, count, dropped = (int(v) for v in status.cpu())
    if code:
        raise ValueError("%s: %s" % (name, RENDER_STATUS.get(code, "status %d" % code)))
    return count, dropped


def depth_render(vertices, faces, view, width, height, return_dropped=False):
    """The depth image of triangle meshes through a View (include/ogc_ops.h: ogc_depth_render): vertices (V, 3) fp64, faces (F, 3)
    int32, CUDA tensors -> (depth (height, width) fp64, +inf where nothing is hit, face (height, width) int32, -1 there) on the device;
    with return_dropped also the number of faces the near rule dropped.  The nearest hit wins a pixel, the lowest face index among
    equal depths.  One host read: the status."""
    _check_mesh(vertices, faces)
    width, height = _check_image(width, height)
    depth, face, status = _render(vertices, faces, view_doubles(view), width, height)
    _, dropped = _render_status("depth_render", status)
    return (depth, face, dropped) if return_dropped else (depth, face)


def render_points(vertices, faces, view, width, height, face_offsets=None):
    """The cloud a depth render sees: the hit points of the covered pixels in row-major pixel order (ogc_depth_render, then
    ogc_depth_points) -> (points (P, 3) fp32, pixel (P,) int32 = y * width + x, face (P,) int32) on the device, and with
    face_offsets ((M + 1,) int32 CUDA tensor, ascending from 0 to F) also mesh_idx (P,) int32, the mesh of each point's face.
    One host read for both stages: the status, which carries P."""
    _check_mesh(vertices, faces)
    if face_offsets is not None:
        _check_tensors(((face_offsets, "face_offsets", torch.int32),))
        if face_offsets.dim() != 1 or face_offsets.shape[0] < 1:
            raise ValueError("face_offsets must be (M + 1,), got %s" % (tuple(face_offsets.shape),))
        _check_contiguous(((face_offsets, "face_offsets", torch.int32),))
    width, height = _check_image(width, height)
    doubles = view_doubles(view)
    depth, face, status = _render(vertices, faces, doubles, width, height)
    points = torch.empty(width * height, 3, dtype=torch.float32, device=vertices.device)
    pixel = torch.empty(width * height, dtype=torch.int32, device=vertices.device)
    face_out = torch.empty(width * height, dtype=torch.int32, device=vertices.device)
    _native.depth_points_wrapper(width, height, doubles, depth, face, points, pixel, face_out, status)
    count, _ = _render_status("render_points", status)
    points, pixel, face_out = points[:count], pixel[:count], face_out[:count]
    if face_offsets is None:
        return points, pixel, face_out
    mesh_idx = (torch.searchsorted(face_offsets, face_out, right=True) - 1).to(torch.int32)
    return points, pixel, face_out, mesh_idx


COMPOSE_STATUS = {3: "a vertex or room value that is not finite",
                  4: "offsets that do not start at 0, descend, do not end at the array sizes, delimit an object without vertices or give "
                     "a trial more than 32 objects"}
# the constants of ogc_room_compose in the order the library takes them, with the reference's values (build_ogcdr.py:51-67)
COMPOSE_DOUBLES = collections.OrderedDict((("ground_level", -0.5 + 0.01), ("wall_thickness", 0.01), ("y_angle_lo", 0.0), ("y_angle_hi", 360.0),
                                           ("mot_y_angle_lo", -10.0), ("mot_y_angle_hi", 10.0), ("mot_xz_angle_lo", -10.0),
                                           ("mot_xz_angle_hi", 10.0), ("prob_rotation_y", 0.6), ("mot_transl_lo", 0.02),
                                           ("mot_transl_hi", 0.04)))
COMPOSE_INTS = collections.OrderedDict((("n_frame", 4), ("max_iter", 1000), ("max_retry", 20)))
Composition = collections.namedtuple("Composition", "poses attempt fails status")


def compose_rooms(vertices, vert_offsets, obj_offsets, room, seeds, **constants):
    """T trial scenes composed in one launch (include/ogc_ops.h: ogc_room_compose): vertices (V, 3) fp64, the canonical meshes of all
    objects of all trials concatenated, vert_offsets (O + 1,) int32, obj_offsets (T + 1,) int32, room (T, 2) fp64 and seeds (T,)
    int64, CUDA tensors; the constants by keyword, any of COMPOSE_DOUBLES and COMPOSE_INTS, the reference's values otherwise
    -> Composition(poses (O, n_frame, 4, 4) fp64, attempt (O, n_frame) int32, fails (T, n_frame) int32, status (T, 2) int32) on the
    device.  status[t] = {code, frame}: 0 composed, 1 frame 0 found no place, 2 the dynamics used up its retries; these are results
    and the caller reads them with the poses.  One host read here: whether any code is 3 or 4, which raise."""
    unknown = set(constants) - set(COMPOSE_DOUBLES) - set(COMPOSE_INTS)
    if unknown:
        raise TypeError("compose_rooms: unknown constants %s" % sorted(unknown))
    tensors = ((vertices, "vertices", torch.float64), (vert_offsets, "vert_offsets", torch.int32), (obj_offsets, "obj_offsets", torch.int32),
               (room, "room", torch.float64), (seeds, "seeds", torch.int64))
    _check_tensors(tensors)
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError("vertices must be (V, 3), got %s" % (tuple(vertices.shape),))
    if vert_offsets.dim() != 1 or vert_offsets.shape[0] < 1 or obj_offsets.dim() != 1 or obj_offsets.shape[0] < 1:
        raise ValueError("vert_offsets must be (O + 1,) and obj_offsets (T + 1,), got %s and %s"
                         % (tuple(vert_offsets.shape), tuple(obj_offsets.shape)))
    n_object, n_trial = vert_offsets.shape[0] - 1, obj_offsets.shape[0] - 1
    if tuple(room.shape) != (n_trial, 2) or tuple(seeds.shape) != (n_trial,):
        raise ValueError("room must be (%d, 2) and seeds (%d,), got %s and %s" % (n_trial, n_trial, tuple(room.shape), tuple(seeds.shape)))
    _check_contiguous(tensors)
    doubles = [float(constants.get(k, v)) for k, v in COMPOSE_DOUBLES.items()]
    n_frame, max_iter, max_retry = (int(constants.get(k, v)) for k, v in COMPOSE_INTS.items())
    dev = vertices.device
    # n_frame sizes the outputs: its range is asked for here as well as by the library, so that nothing absurd is allocated
    frames = n_frame if 1 <= n_frame <= 8 else 1
    out = Composition(torch.empty(n_object, frames, 4, 4, dtype=torch.float64, device=dev),
                      torch.empty(n_object, frames, dtype=torch.int32, device=dev),
                      torch.empty(n_trial, frames, dtype=torch.int32, device=dev), torch.empty(n_trial, 2, dtype=torch.int32, device=dev))
    _native.room_compose_wrapper(n_trial, n_object, vertices.shape[0], vertices, vert_offsets, obj_offsets, room, seeds, doubles,
                                 (n_frame, max_iter, max_retry), out.poses, out.attempt, out.fails, out.status)
    if n_trial:
        code = int(out.status[:, 0].max().item())
        if code >= 3:
            raise ValueError("compose_rooms: " + COMPOSE_STATUS.get(code, "status %d" % code))
    return out


def apply_poses(vertices, vert_offsets, poses):
    """Every object's vertices under its pose of every frame (ogc_mesh_apply_poses): vertices (V, 3) fp64, vert_offsets (O + 1,) int32
    ascending from 0 to V, poses (O, n_frame, 4, 4) fp64, CUDA tensors -> (n_frame, V, 3) fp64 on the device,
    ((R_i0 * x + R_i1 * y) + R_i2 * z) + t_i.  No host read."""
    tensors = ((vertices, "vertices", torch.float64), (vert_offsets, "vert_offsets", torch.int32), (poses, "poses", torch.float64))
    _check_tensors(tensors)
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError("vertices must be (V, 3), got %s" % (tuple(vertices.shape),))
    if vert_offsets.dim() != 1 or vert_offsets.shape[0] < 1:
        raise ValueError("vert_offsets must be (O + 1,), got %s" % (tuple(vert_offsets.shape),))
    n_object = vert_offsets.shape[0] - 1
    if poses.dim() != 4 or poses.shape[0] != n_object or tuple(poses.shape[2:]) != (4, 4):
        raise ValueError("poses must be (%d, n_frame, 4, 4), got %s" % (n_object, tuple(poses.shape)))
    _check_contiguous(tensors)
    out = torch.empty(poses.shape[1], vertices.shape[0], 3, dtype=torch.float64, device=vertices.device)
    _native.mesh_apply_poses_wrapper(vertices.shape[0], n_object, poses.shape[1], vertices, vert_offsets, poses, out)
    return out


def even_radius(area, count):
    """The radius sample_surface_even thins `3 * count` candidates with: sqrt(area / (3 * count)), float64."""
    return np.sqrt(np.float64(area) / np.float64(3 * count))


def sample_surface_even(vertices, faces, face_offsets, counts, seed):
    """An even sampling of M concatenated meshes, the package's form of trimesh.sample.sample_surface_even: for every mesh draw
    3 * count candidates, thin them with the radius sqrt(area / (3 * count)) and keep the first `count` survivors in index order,
    or all of them if there are fewer.  vertices (V, 3) float64 and faces (F, 3) int32 numpy arrays (the faces index the
    concatenated vertices), face_offsets (M + 1) and counts (M) integers; seed an integer.
    -> (points (P, 3) fp64, mesh_idx (P,) int32) CUDA tensors, in mesh order and, inside a mesh, in candidate order.  A mesh whose
    count is 0 contributes nothing.  One upload of the meshes; the areas are computed on the host (cumulative_areas)."""
    vertices = np.ascontiguousarray(vertices, dtype=np.float64)
    faces = np.ascontiguousarray(faces, dtype=np.int32)
    face_offsets = np.asarray(face_offsets, dtype=np.int64)
    counts = np.asarray(counts, dtype=np.int64)
    if vertices.ndim != 2 or vertices.shape[1] != 3 or faces.ndim != 2 or faces.shape[1] != 3:
        raise ValueError("vertices must be (V, 3) and faces (F, 3), got %s and %s" % (vertices.shape, faces.shape))
    if face_offsets.ndim != 1 or counts.shape != (face_offsets.shape[0] - 1,):
        raise ValueError("face_offsets must be (M + 1,) and counts (M,), got %s and %s" % (face_offsets.shape, counts.shape))
    if (counts < 0).any() or 3 * int(counts.sum()) > 1 << 26:
        raise ValueError("counts must be >= 0 and sum to at most 2**26 / 3")
    cum, area = cumulative_areas(vertices, faces, face_offsets)
    cand_offsets = np.concatenate([[0], np.cumsum(3 * counts)]).astype(np.int32)
    with np.errstate(divide="ignore", invalid="ignore"):
        radius = np.where(counts > 0, even_radius(area, np.maximum(counts, 1)), 0.0)
    dev = "cuda"
    cand_dev = torch.from_numpy(cand_offsets).to(dev)
    points, _ = surface_candidates(torch.from_numpy(vertices).to(dev), torch.from_numpy(faces).to(dev), torch.from_numpy(cum).to(dev),
                                   torch.from_numpy(face_offsets.astype(np.int32)).to(dev), cand_dev, seed)
    keep = surface_thin(points, cand_dev, torch.from_numpy(radius).to(dev))
    # the first `count` survivors of every mesh: a survivor's rank inside its mesh from one running sum
    mesh_idx = torch.repeat_interleave(torch.arange(counts.shape[0], device=dev, dtype=torch.int32),
                                       torch.from_numpy(3 * counts).to(dev))
    running = torch.cumsum(keep, 0, dtype=torch.int64)
    before = torch.cat([running.new_zeros(1), running])[cand_dev[:-1].long()]       # survivors ahead of each mesh
    rank = running - before[mesh_idx.long()]                                        # 1-based among the mesh's survivors
    chosen = (keep == 1) & (rank <= torch.from_numpy(counts).to(dev)[mesh_idx.long()])
    return points[chosen], mesh_idx[chosen]

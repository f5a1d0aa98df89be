"""OGC-DR preparation, the single-view clouds (reference: data_prepare/ogcdrsv/build_ogcdrsv.py): the object meshes of
<src_root>/mesh/<id>/ rendered frame by frame -> <dest_root>/pcd/<id>/pc_%02d.pcd, what collect_segm reads.

    python -m ogc_amd.data_prepare.build_ogcdrsv --src_root <OGC-DR root> --dest_root <OGC-DRSV root>
                                                 [--width 1920 --height 1080 --fov 60 --zoom 0.7] [--synthetic N]

Per frame: the object_FF_OO.obj files of the int(id[:2]) objects are read on the host (mesh_io.read_obj) and uploaded once; ground
and walls are not rendered, as in the reference.  One render (mesh_ops.render_points: DESIGN §4n) through the default view of the
frame's bounding box (mesh_ops.default_view) gives the hit points of the covered pixels in row-major order, which are written as
binary PCD.  The reference renders through open3d's visualiser and saves its depth image as a cloud; the view and the rasteriser
here are this package's own definition (include/ogc_ops.h: ogc_depth_render) and have not been compared with open3d.  A frame that
renders no point is an error that names scene and frame.  `--synthetic N` first writes N synthetic scenes into SRC_ROOT
(ogc_amd/utils/synthetic.py::write_ogcdr_mesh_root).
"""
import argparse
import os

import numpy as np
import torch

from .mesh_io import read_obj, write_pcd
from .mesh_ops import default_view, render_points
from .sample_pointcloud import N_FRAME, concat_meshes


def frame_view(vertices, width, height, fov_deg, zoom):
    """The default view of the bounding box of a frame's vertices (numpy (V, 3) float64)."""
    return default_view(vertices.min(0), vertices.max(0), width=width, height=height, fov_deg=fov_deg, zoom=zoom)


def render_frame(meshes, width, height, fov_deg, zoom, where="the frame", device="cuda"):
    """meshes: [(vertices, faces)] of a frame's objects -> (points (P, 3) float32, mesh_idx (P,) int32), numpy, in row-major pixel
    order."""
    vertices, faces, face_offsets = concat_meshes(meshes)
    vertices = np.ascontiguousarray(vertices, dtype=np.float64)
    if vertices.shape[0] == 0 or faces.shape[0] == 0:
        raise ValueError("%s holds no triangle" % where)
    if not np.isfinite(vertices).all():
        raise ValueError("%s holds a vertex coordinate that is not finite" % where)
    view = frame_view(vertices, width, height, fov_deg, zoom)
    points, _, _, mesh_idx = render_points(torch.from_numpy(vertices).to(device), torch.from_numpy(np.ascontiguousarray(faces)).to(device),
                                           view, width, height, torch.from_numpy(face_offsets.astype(np.int32)).to(device))
    if points.shape[0] == 0:
        raise ValueError("%s renders no point at %d x %d" % (where, width, height))
    return points.cpu().numpy(), mesh_idx.cpu().numpy()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--src_root", type=str, required=True, help="Root path for the OGC-DR dataset: mesh/ below it")
    ap.add_argument("--dest_root", type=str, required=True, help="Root path for the OGC-DRSV dataset: pcd/ is written below it")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--fov", type=float, default=60.0, help="vertical field of view in degrees")
    ap.add_argument("--zoom", type=float, default=0.7)
    ap.add_argument("--synthetic", type=int, default=0, help="write this many synthetic scenes into src_root first")
    args = ap.parse_args(argv)
    if not (1 <= args.width <= 16384 and 1 <= args.height <= 16384):
        raise ValueError("--width and --height must be in 1..16384, got %d x %d" % (args.width, args.height))
    if not 0.0 < args.fov < 180.0:
        raise ValueError("--fov must be inside (0, 180) degrees, got %r" % args.fov)
    if not args.zoom > 0.0:
        raise ValueError("--zoom must be positive, got %r" % args.zoom)
    if args.synthetic < 0:
        raise ValueError("--synthetic must not be negative")
    mesh_root = os.path.join(args.src_root, "mesh")
    if args.synthetic == 0 and not os.path.isdir(mesh_root):
        raise FileNotFoundError("%s is no directory: --src_root must hold mesh/<id>/object_FF_OO.obj" % mesh_root)
    if not torch.cuda.is_available():
        raise RuntimeError("build_ogcdrsv needs a HIP device; ogc_amd has no CPU path")
    if args.synthetic > 0:
        from ..utils.synthetic import write_ogcdr_mesh_root
        write_ogcdr_mesh_root(args.src_root, args.synthetic)
    save_root = os.path.join(args.dest_root, "pcd")
    os.makedirs(save_root, exist_ok=True)
    data_ids = sorted(os.listdir(mesh_root))
    n_points = 0
    for data_id in data_ids:
        n_object = int(data_id[:2])
        data_path, save_path = os.path.join(mesh_root, data_id), os.path.join(save_root, data_id)
        os.makedirs(save_path, exist_ok=True)
        for frame_id in range(N_FRAME):
            meshes = [read_obj(os.path.join(data_path, "object_%02d_%02d.obj" % (frame_id, k))) for k in range(n_object)]
            points, _ = render_frame(meshes, args.width, args.height, args.fov, args.zoom, where="scene %s, frame %d" % (data_id, frame_id))
            write_pcd(os.path.join(save_path, "pc_%02d.pcd" % frame_id), points)
            n_points += points.shape[0]
    print("build_ogcdrsv: %d scenes of %d frames written to %s (%d points in all)" % (len(data_ids), N_FRAME, save_root, n_points))
    return {"scenes": data_ids, "save_root": save_root, "points": n_points}


if __name__ == "__main__":
    main()

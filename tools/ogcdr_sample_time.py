"""Time of the OGC-DR surface sampling (ogc_amd/data_prepare/sample_pointcloud.py) on one frame at the size it runs at —
eight objects, ground and walls, 100 000 wanted points, about 300 000 candidates:

  candidates  HIP-event time of ogc_surface_candidates (its check and its draw), on tensors that are on the device already
  thinning    wall time of mesh_ops.surface_thin: the grid, the rounds and the reads of the status word; the number of rounds
  fps         HIP-event time of furthest point sampling, the kept points after the crop -> 2048
  labels      HIP-event time of ogc_nearest_label at collect_segm's size, 4 x 2048 queries against 4 x 2048 source points
  frame       wall time of sample_pointcloud.sample_frame: areas on the host, one upload, everything above, the copy back
  host        wall time of the thinning mirror (cKDTree.query_pairs and one ordered pass, tests/ogcdr_prepare_cases.py) on the same
              candidates — for orientation only: the reference's trimesh path cannot run where trimesh is not installed

after warm-up and after a check that device and mirror give the same keep flags.  Needs the GPU.

    python tools/ogcdr_sample_time.py [--calls 20] [--warmup 3] [--out profiles/ogcdr_sample_time.txt]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ogcdr_prepare_cases as mirror  # noqa: E402
from ogc_amd.data_prepare import mesh_ops, sample_pointcloud  # noqa: E402
from ogc_amd.pointnet2.pointnet2 import furthest_point_sample  # noqa: E402
from ogc_amd.utils import synthetic  # noqa: E402

N_OBJECT, N_SAMPLE_POINT, N_FPS = 8, 100000, 2048
XZ_RANGE = np.array([1.0, 0.8])


def summary(ms):
    ms = sorted(ms)
    return "median %.3f ms, min %.3f, max %.3f over %d calls" % (statistics.median(ms), ms[0], ms[-1], len(ms))


def events(fn, calls, warmup):
    out = []
    for i in range(warmup + calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= warmup:
            out.append(e0.elapsed_time(e1))
    return out


def wall(fn, calls, warmup, device=True):
    out = []
    for i in range(warmup + calls):
        if device:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if device:
            torch.cuda.synchronize()
        if i >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return out


def frame_meshes():
    """Eight synthetic objects of 48 to 108 triangles, three times their usual size, in a room of 1.0 x 0.8 with ground and walls."""
    rs = np.random.RandomState(77)
    meshes = []
    for k in range(N_OBJECT):
        vertices, faces = synthetic.ogcdr_object_mesh(k, rs)
        faces = np.array([[f[0], f[j], f[j + 1]] for f in faces for j in range(1, len(f) - 1)], dtype=np.int32)
        meshes.append((vertices * 3.0 + np.array([(k % 4 - 1.5) * 0.2, -0.3, (k // 4 - 0.5) * 0.3]), faces))
    gl, wt, h = synthetic.OGCDR_GROUND_LEVEL, synthetic.OGCDR_WALL_THICKNESS, 0.2
    boxes = [([-0.5, -0.5, -0.4], [0.5, gl, 0.4]), ([-0.5, gl, -0.4], [0.5, gl + h, -0.4 + wt]), ([-0.5, gl, -0.4], [-0.5 + wt, gl + h, 0.4]),
             ([-0.5, gl, 0.4 - wt], [0.5, gl + h, 0.4]), ([0.5 - wt, gl, -0.4], [0.5, gl + h, 0.4])]
    for lo, hi in boxes:
        vertices, faces = synthetic.box_mesh_between(lo, hi)
        meshes.append((vertices, np.asarray(faces, dtype=np.int32)))
    return meshes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ogcdr_sample_time.py measures on the GPU"
    lines = ["device: %s" % torch.cuda.get_device_name(0)]
    meshes = frame_meshes()
    vertices, faces, face_offsets = sample_pointcloud.concat_meshes(meshes)
    cum, area = mesh_ops.cumulative_areas(vertices, faces, face_offsets)
    counts = np.array(sample_pointcloud.point_counts(area, N_SAMPLE_POINT))
    cand_offsets = np.concatenate([[0], np.cumsum(3 * counts)]).astype(np.int32)
    radius = mesh_ops.even_radius(area, counts)
    total = int(cand_offsets[-1])
    dev = [torch.from_numpy(a).cuda() for a in (vertices, faces, cum, face_offsets.astype(np.int32), cand_offsets)]
    radius_dev = torch.from_numpy(radius).cuda()

    points, _ = mesh_ops.surface_candidates(*dev, 5)
    keep, rounds = mesh_ops.surface_thin(points, dev[4], radius_dev, return_rounds=True)
    host_points = points.cpu().numpy()
    t0 = time.perf_counter()
    want = mirror.greedy_thin_reference(host_points, cand_offsets, radius)
    host_ms = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(keep.cpu().numpy(), want), "device and mirror differ"
    kept = int(want.sum())

    candidates = events(lambda: mesh_ops.surface_candidates(*dev, 5), args.calls, args.warmup)
    thinning = wall(lambda: mesh_ops.surface_thin(points, dev[4], radius_dev), args.calls, args.warmup)
    frame = wall(lambda: sample_pointcloud.sample_frame(meshes, N_OBJECT, XZ_RANGE, N_SAMPLE_POINT, N_FPS, 5), args.calls, args.warmup)
    cloud = points[keep == 1].float()
    cloud = cloud[sample_pointcloud.crop_mask(cloud, XZ_RANGE)][:N_SAMPLE_POINT].unsqueeze(0).contiguous()
    fps = events(lambda: furthest_point_sample(cloud, N_FPS), args.calls, args.warmup)
    rs = np.random.RandomState(3)
    query, source = (torch.from_numpy(rs.rand(4, N_FPS, 3).astype(np.float32)).cuda() for _ in range(2))
    labels = torch.from_numpy(rs.randint(0, 9, size=(4, N_FPS)).astype(np.int32)).cuda()
    nearest = events(lambda: mesh_ops.nearest_label(query, source, labels), args.calls, args.warmup)
    lines += ["OGC-DR surface sampling, one frame: %d meshes (%d objects), %d faces, %d wanted points, %d candidates, %d kept by the thinning"
              % (len(meshes), N_OBJECT, len(faces), N_SAMPLE_POINT, total, kept),
              "  device == mirror in every keep flag; thinning radius %.5f .. %.5f; rounds that decided something: %d" % (radius.min(), radius.max(), rounds),
              "  ogc_surface_candidates (check + draw, one status read), HIP events: %s" % summary(candidates),
              "  surface_thin (grid, %d rounds queued per status read, the reads), wall: %s" % (mesh_ops.THIN_FIRST_ROUNDS, summary(thinning)),
              "  furthest point sampling %d -> %d, HIP events: %s" % (cloud.shape[1], N_FPS, summary(fps)),
              "  ogc_nearest_label 4 x %d queries x %d source points, HIP events: %s" % (N_FPS, N_FPS, summary(nearest)),
              "  sample_frame (host areas, upload, candidates, thinning, crop, FPS, copy back), wall: %s" % summary(frame),
              "  thinning mirror on the host (cKDTree.query_pairs + one ordered pass), wall, one call, for orientation only: %.1f ms" % host_ms]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

"""Time of the OGC-DRSV depth render (ogc_amd/data_prepare/build_ogcdrsv.py) on one frame at the size it runs at —
1920 x 1080, eight synthetic objects (subdivided spheres and grid boxes) of about 100 000 triangles in all, the default view of their
bounding box:

  setup       HIP-event time of the status clear, the per-face records, the item offsets and the empty image
  depth pass  HIP-event time of the two launches that take the minimum depth per pixel (small faces, (face, block) items)
  face pass   HIP-event time of the two launches that take the lowest face index at that depth
              (the three from ogc_depth_render_timed, which records events between the stages of ogc_depth_render)
  render      HIP-event time of ogc_depth_render as the driver calls it
  compaction  HIP-event time of ogc_depth_points: count and scatter of the covered pixels
  frame       wall time of build_ogcdrsv.render_frame: concatenation and bounding box on the host, one upload, render, compaction,
              the status read, the copy back
  extreme     the three stage times again for two faces that each cover every centre of the image
  host        with --mirror: wall time of the numpy mirror (tests/depth_render_cases.py) on the same frame, after a check that device
              and mirror give the same depth bits, faces and points — for orientation only: open3d, which the reference renders
              with, is not installed where this runs, so there is no ratio against the reference

after warm-up.  Needs the GPU.

    python tools/ogcdrsv_render_time.py [--calls 20] [--warmup 3] [--mirror] [--out profiles/ogcdrsv_render_time.txt]"""
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
import depth_render_cases as mirror  # noqa: E402
from ogc_amd import pointnet2_cuda as native  # noqa: E402
from ogc_amd.data_prepare import build_ogcdrsv, mesh_ops, sample_pointcloud  # noqa: E402
from ogc_amd.utils import synthetic  # noqa: E402

WIDTH, HEIGHT, FOV, ZOOM = 1920, 1080, 60.0, 0.7


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


def wall(fn, calls, warmup):
    out = []
    for i in range(warmup + calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return out


def frame_meshes():
    """Eight objects in two rows: six spheres of 2 * 80 * 79 = 12 640 triangles and two grid boxes of 12 * 32^2 = 12 288."""
    meshes = []
    for k in range(8):
        centre = np.array([(k % 4 - 1.5) * 0.22, (k // 4 - 0.5) * 0.25, 0.05 * (k % 3)])
        if k % 3 == 2:
            vertices, faces = synthetic._grid_box([0.15, 0.12, 0.1], 32)
            meshes.append((np.asarray(vertices) + centre, np.asarray(faces, dtype=np.int32)))
        else:
            meshes.append(mirror.uv_sphere(centre, 0.08, 80, 80))
    return meshes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mirror", action="store_true", help="check against the numpy mirror and quote its time")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ogcdrsv_render_time.py measures on the GPU"
    lines = ["device: %s" % torch.cuda.get_device_name(0)]
    meshes = frame_meshes()
    vertices, faces, face_offsets = sample_pointcloud.concat_meshes(meshes)
    view = build_ogcdrsv.frame_view(vertices, WIDTH, HEIGHT, FOV, ZOOM)
    doubles = mesh_ops.view_doubles(view)
    v_dev, f_dev = torch.from_numpy(np.ascontiguousarray(vertices)).cuda(), torch.from_numpy(faces).cuda()
    n_vertex, n_face = v_dev.shape[0], f_dev.shape[0]
    depth = torch.empty(HEIGHT, WIDTH, dtype=torch.float64, device="cuda")
    face = torch.empty(HEIGHT, WIDTH, dtype=torch.int32, device="cuda")
    status = torch.empty(3, dtype=torch.int32, device="cuda")
    ws = torch.empty(native.depth_render_ws_bytes(n_face), dtype=torch.uint8, device="cuda")
    points = torch.empty(WIDTH * HEIGHT, 3, dtype=torch.float32, device="cuda")
    pixel = torch.empty(WIDTH * HEIGHT, dtype=torch.int32, device="cuda")
    face_out = torch.empty(WIDTH * HEIGHT, dtype=torch.int32, device="cuda")

    def render():
        native.depth_render_wrapper(n_vertex, n_face, v_dev, f_dev, doubles, WIDTH, HEIGHT, depth, face, status, ws)

    def compact():
        native.depth_points_wrapper(WIDTH, HEIGHT, doubles, depth, face, points, pixel, face_out, status)

    render()
    compact()
    code, count, dropped = status.cpu().tolist()
    assert code == 0 and dropped == 0 and count > 0, (code, count, dropped)
    lines.append("OGC-DRSV depth render, one frame: %d objects, %d faces, %d vertices, %d x %d pixels, %d covered (%.1f %%)"
                 % (len(meshes), n_face, n_vertex, WIDTH, HEIGHT, count, 100.0 * count / (WIDTH * HEIGHT)))
    if args.mirror:
        t0 = time.perf_counter()
        want = mirror.mirror_render(vertices, faces, np.array(doubles), WIDTH, HEIGHT)
        host_ms = (time.perf_counter() - t0) * 1e3
        assert np.array_equal(depth.cpu().numpy().view(np.uint64), want["depth"].view(np.uint64)), "device and mirror differ in the depth"
        assert np.array_equal(face.cpu().numpy(), want["face"]), "device and mirror differ in the faces"
        assert count == len(want["pixel"]) and np.array_equal(points[:count].cpu().numpy().view(np.uint32), want["points"].view(np.uint32))
        lines.append("  device == mirror in every bit of the depth image, every face and every point")

    stages = []
    for i in range(args.warmup + args.calls):
        ms = native.depth_render_timed_wrapper(n_vertex, n_face, v_dev, f_dev, doubles, WIDTH, HEIGHT, depth, face, status, ws)
        if i >= args.warmup:
            stages.append(ms)
    whole = events(render, args.calls, args.warmup)
    compaction = events(compact, args.calls, args.warmup)
    frame = wall(lambda: build_ogcdrsv.render_frame(meshes, WIDTH, HEIGHT, FOV, ZOOM), args.calls, args.warmup)
    lines += ["  setup (status, face records, item offsets, empty image), HIP events: %s" % summary([s[0] for s in stages]),
              "  depth pass (small faces + block items, 64-bit atomicMin), HIP events: %s" % summary([s[1] for s in stages]),
              "  face pass (same walk, 32-bit atomicMin where the depth is the stored one), HIP events: %s" % summary([s[2] for s in stages]),
              "  ogc_depth_render, all of the above in one call, HIP events: %s" % summary(whole),
              "  ogc_depth_points (count + scatter of the covered pixels), HIP events: %s" % summary(compaction),
              "  render_frame (host concatenation and box, upload, render, compaction, status read, copy back), wall: %s" % summary(frame)]
    if args.mirror:
        lines.append("  numpy mirror on the host, wall, one call, for orientation only (no open3d here: no ratio against the reference): %.0f ms" % host_ms)
    # the other extreme of the load: two faces that cover every centre, 2 x 32 400 block items
    big_view = mirror.axis_view(1024.0, WIDTH / 2.0, HEIGHT / 2.0, 0.5, 64.0)
    big = mirror.scene(big_view, WIDTH, HEIGHT, [((-6000.0, -4000.0, 2.0), (9000.0, -3000.0, 8.0), (900.0, 12000.0, 4.0)),
                                                 ((-6000.0, -3000.0, 8.0), (9000.0, -4000.0, 2.0), (1000.0, 12000.0, 4.0))])
    bv, bf = torch.from_numpy(big["vertices"]).cuda(), torch.from_numpy(big["faces"]).cuda()
    big_stages = []
    for i in range(args.warmup + args.calls):
        ms = native.depth_render_timed_wrapper(6, 2, bv, bf, big_view.tolist(), WIDTH, HEIGHT, depth, face, status, ws)
        if i >= args.warmup:
            big_stages.append(ms)
    native.depth_points_wrapper(WIDTH, HEIGHT, big_view.tolist(), depth, face, points, pixel, face_out, status)
    code, count, _ = status.cpu().tolist()
    assert code == 0 and count == WIDTH * HEIGHT, (code, count)
    lines += ["two faces that each cover all %d centres (2 x 32 400 items), every pixel hit twice:" % (WIDTH * HEIGHT),
              "  depth pass, HIP events: %s" % summary([s[1] for s in big_stages]),
              "  face pass, HIP events: %s" % summary([s[2] for s in big_stages]),
              "  setup + both passes, HIP events: %s" % summary([sum(s) for s in big_stages])]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

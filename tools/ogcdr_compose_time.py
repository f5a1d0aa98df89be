"""Time of the OGC-DR scene composition (ogc_amd/data_prepare/build_ogcdr.py) on one batch at the shape it runs at —
64 trial scenes x 8 objects, every object a slim grid box of about ten thousand vertices scaled into the reference's first scale
interval, rooms as the driver draws them:

  compose  HIP-event time of ogc_room_compose alone (the offsets check and the composition), on tensors that are on the device already
  apply    HIP-event time of ogc_mesh_apply_poses alone: the four frames of every vertex
  step     wall time of the device step of a batch as the driver runs it: one upload of the canonical meshes, the two launches, the
           status read, the copies back of poses, status and frame vertices
  host     with --mirror: wall time of the numpy mirror (tests/ogcdr_compose_cases.py) on the first trials of the batch, after a check
           that device and mirror agree in every bit there — for orientation only: the reference's loop runs trimesh on every try

after warm-up.  Reading and parsing the .obj files, which the driver does on the host, is not in any of these.  Needs the GPU.

    python tools/ogcdr_compose_time.py [--calls 50] [--warmup 5] [--mirror 4] [--out profiles/ogcdr_compose_time.txt]"""
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
import ogcdr_compose_cases as mirror  # noqa: E402
from ogc_amd.data_prepare import build_ogcdr, mesh_ops  # noqa: E402

TRIALS, OBJECTS, GRID = 64, 8, 41       # a grid box of 6 * (41 + 1)^2 = 10 584 vertices


def grid_box_vertices(size, k):
    t = np.linspace(-0.5, 0.5, k + 1)
    a, b = (g.ravel() for g in np.meshgrid(t, t, indexing="ij"))
    sides = []
    for axis in range(3):
        for sign in (-0.5, 0.5):
            p = np.zeros((a.size, 3))
            p[:, axis], p[:, (axis + 1) % 3], p[:, (axis + 2) % 3] = sign, a, b
            sides.append(p)
    return np.concatenate(sides) * np.asarray(size)


def summary(ms):
    ms = sorted(ms)
    return "median %.4f ms, min %.4f, p90 %.4f over %d calls" % (statistics.median(ms), ms[0], ms[int(0.9 * len(ms))], len(ms))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--mirror", type=int, default=0, help="compare and time the numpy mirror on this many trials")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ogcdr_compose_time.py measures on the GPU"
    rs = np.random.RandomState(700)
    lo, hi = build_ogcdr.SCALE_INTERVALS[0]
    trials = []
    for _ in range(TRIALS):
        meshes = [build_ogcdr.canonical_vertices(grid_box_vertices([1.0, 0.2 + 0.2 * rs.rand(), 0.3 + 0.5 * rs.rand()], GRID) + rs.rand(3), lo + rs.rand() * (hi - lo))
                  for _ in range(OBJECTS)]
        trials.append((meshes, mirror.draw_room(rs)))
    batch = mirror.pack(trials, 700)
    keys = ("vertices", "vert_offsets", "obj_offsets", "room", "seeds")
    dev = [torch.from_numpy(np.ascontiguousarray(batch[k])).cuda() for k in keys]
    out = mesh_ops.compose_rooms(*dev)
    status = out.status.cpu().numpy()
    good = status[:, 0] == 0
    lines = ["device: %s" % torch.cuda.get_device_name(0),
             "OGC-DR scene composition: %d trials x %d objects, %d vertices per object, %.1f MB of canonical vertices; codes 0 / 1 / 2: %s; "
             "largest accepted attempt %d, most failed tries of a composed scene %d"
             % (TRIALS, OBJECTS, len(trials[0][0][0]), batch["vertices"].nbytes / 1e6, " / ".join(str(int((status[:, 0] == c).sum())) for c in range(3)),
                int(out.attempt.cpu().numpy()[np.repeat(good, OBJECTS)].max(initial=0)), int(out.fails.cpu().numpy()[good].max(initial=0)))]
    lines.append("  ogc_room_compose, one call alone, HIP events: %s" % summary(events(lambda: mesh_ops.compose_rooms(*dev), args.calls, args.warmup)))
    lines.append("  ogc_mesh_apply_poses, one call alone, HIP events: %s"
                 % summary(events(lambda: mesh_ops.apply_poses(dev[0], dev[1], out.poses), args.calls, args.warmup)))

    def step():
        up = [torch.from_numpy(batch[k]).cuda() for k in keys]
        composed = mesh_ops.compose_rooms(*up)
        frames = mesh_ops.apply_poses(up[0], up[1], composed.poses).cpu()
        return composed.status.cpu(), composed.poses.cpu(), frames
    lines.append("  device step of a batch (upload, two launches, status read, copies back of %.1f MB), wall: %s"
                 % (4 * batch["vertices"].nbytes / 1e6, summary(wall(step, max(args.calls // 5, 3), 2))))
    if args.mirror > 0:
        n = min(args.mirror, TRIALS)
        part = mirror.pack(trials[:n], 700)
        t0 = time.perf_counter()
        want = mirror.compose_mirror(*[part[k] for k in keys])
        host_ms = (time.perf_counter() - t0) * 1e3
        want["obj_offsets"] = part["obj_offsets"]
        got = {k: getattr(out, k).cpu().numpy() for k in out._fields}
        mirror.compare_composed({"status": got["status"][:n], "fails": got["fails"][:n], "attempt": got["attempt"][:n * OBJECTS],
                                 "poses": got["poses"][:n * OBJECTS]}, want)
        lines.append("  numpy mirror on the host, first %d trials (equal to the device in every bit), wall: %.1f ms, %.1f ms per trial" % (n, host_ms, host_ms / n))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

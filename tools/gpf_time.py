"""Time of the ground-plane kernel (ogc_ground_plane_fit, launched through pointnet2_cuda.ground_plane_fit_wrapper on
preallocated outputs, after a check against ogc_amd.utils.gpf_util.ground_plane_fit_batch) on the data of
the fixture (tests/golden/gpf.npz): case g2048 at B = 2 — the Waymo flow-prediction driver's launch, the cloud twice, so both
workgroups do the same work — and case g8192 at B = 1, the function's defaults and the size limit.  HIP-event medians per call
after warm-up, every call timed on its own.  Beside them the time of `gpf_trace` (tests/golden/make_gpf_golden.py), the float64
numpy statement of the same loop, on the CPU of the machine this runs on and on the same data: the reference runs this step
in numpy on the CPU (utils/gpf_util.py), once per cloud.  Needs the GPU.

    python tools/gpf_time.py [--calls 200] [--warmup 20] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from make_gpf_golden import gpf_trace  # noqa: E402
from ogc_amd.pointnet2_cuda import ground_plane_fit_wrapper  # noqa: E402
from ogc_amd.utils.gpf_util import ground_plane_fit_batch  # noqa: E402

ARGS = ("n_iter", "n_lpr", "thresh_seed", "thresh_dist", "vertical_axis")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "gpf_time.py measures on the GPU"
    data = np.load(os.path.join(ROOT, "tests", "golden", "gpf.npz"))
    meta = json.loads(str(data["meta"]))
    lines = ["device: %s" % torch.cuda.get_device_name(0)]
    for name, B in (("g2048", 2), ("g8192", 1)):
        kw = {k: meta["cases"][name][k] for k in ARGS}
        cloud = data[name + "_pc"]
        pc = torch.from_numpy(cloud).cuda().repeat(B, 1, 1).contiguous()
        plane, mask, attempts = ground_plane_fit_batch(pc, **kw)
        # the timed call is the launch alone, on outputs allocated once: no allocation, no conversion of the mask to bool
        n = pc.shape[1]
        out = (torch.empty(B, 6, dtype=torch.float64, device="cuda"), torch.empty(B, n, dtype=torch.int32, device="cuda"),
               torch.empty(B, dtype=torch.int32, device="cuda"))

        def launch():
            ground_plane_fit_wrapper(B, n, pc, kw["n_iter"], kw["n_lpr"], kw["thresh_seed"], kw["thresh_dist"],
                                     kw["vertical_axis"], *out)

        for _ in range(args.warmup):
            launch()
        torch.cuda.synchronize()
        assert torch.equal(out[0], plane) and torch.equal(out[1].bool(), mask) and torch.equal(out[2], attempts)
        assert attempts.tolist() == data[name + "_attempts"].tolist() * B
        assert np.array_equal(mask.cpu().numpy(), np.repeat(data[name + "_is_ground"], B, 0))
        ms = []
        for _ in range(args.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms.sort()
        cpu = []
        for _ in range(max(3, args.calls // 20)):
            t0 = time.perf_counter()
            for _ in range(B):
                gpf_trace(cloud[0], **kw)
            cpu.append((time.perf_counter() - t0) * 1e3)
        lines.append("ogc_ground_plane_fit %s B=%d n=%d (%d fits): median %.4f ms, min %.4f, p90 %.4f over %d calls; "
                     "gpf_trace (numpy, float64, this CPU, the same %d cloud(s)): median %.3f ms"
                     % (name, B, cloud.shape[1], kw["n_iter"], statistics.median(ms), ms[0], ms[int(0.9 * len(ms))], len(ms), B,
                        statistics.median(cpu)))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

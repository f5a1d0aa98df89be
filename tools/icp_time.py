"""Time of the rigid-ICP kernel (ogc_rigid_icp through ogc_amd.utils.icp_util.icp_batch) on the data of fixture case c
(tests/golden/icp.npz: n = 1024, the flow-prediction driver's size; the reference needs 6 iterations there, i = 5):
HIP-event medians per call at (B, n) = (1, 1024) and (16, 1024) — the batch is the same pair 16 times, so every workgroup does
the same work — after warm-up, every call timed on its own.  Needs the GPU; prints one line per shape and the reference's CPU
time recorded in the fixture.

    python tools/icp_time.py [--calls 200] [--warmup 20] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ogc_amd.utils.icp_util import icp_batch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "icp_time.py measures on the GPU"
    data = np.load(os.path.join(ROOT, "tests", "golden", "icp.npz"))
    meta = json.loads(str(data["meta"]))
    lines = ["device: %s" % torch.cuda.get_device_name(0)]
    for B in (1, 16):
        src = torch.from_numpy(data["c_src"]).cuda().repeat(B, 1, 1).contiguous()
        dst = torch.from_numpy(data["c_dst"]).cuda().repeat(B, 1, 1).contiguous()
        for _ in range(args.warmup):
            T, dist, iters = icp_batch(src, dst)
        torch.cuda.synchronize()
        assert iters.tolist() == [int(data["c_iters"][0])] * B
        ms = []
        for _ in range(args.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            icp_batch(src, dst)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms.sort()
        lines.append("icp_batch B=%d n=1024 (%d iterations + final fit): median %.4f ms, min %.4f, p90 %.4f over %d calls; "
                     "%.4f ms per iteration and pair-batch" % (B, int(iters[0]) + 1, statistics.median(ms), ms[0],
                                                              ms[int(0.9 * len(ms))], len(ms),
                                                              statistics.median(ms) / (int(iters[0]) + 1)))
    lines.append("reference icp (sklearn kd-tree + numpy, CPU of the build machine, same pair): median %.2f ms"
                 % meta["reference_cpu_ms_case_c"])
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

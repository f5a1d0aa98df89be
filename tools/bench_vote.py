"""Times vote.vote_batch at the two shapes the evaluation runs it at (test_batch_size 64) and reports the peak of the caching
allocator:
    ogcdr     16 scenes x 4 frames x 4096 points, 8 slots
    kittisf   32 scenes x 2 frames x 8192 points, 10 slots
One JSON line per shape.  Uses only vote.vote_batch and utils.synthetic.make_sequence, so the same file times any revision of the
package: `--root DIR` names the tree whose ogc_amd is imported (default: the tree this file is in).  To compare two revisions run
them in separate processes, alternating, and look at the spread of the repeats before the difference.

    python tools/bench_vote.py [--root DIR] [--shapes ogcdr,kittisf] [--reps 5] [--warmup 2] [--save PREFIX]

`--save PREFIX` stores the voted masks of each shape as PREFIX_<shape>.pt, for comparing the results of two revisions.
"""
import argparse
import json
import os
import sys
import time

SHAPES = {"ogcdr": (16, 4, 4096, 8, False), "kittisf": (32, 2, 8192, 10, True)}   # scenes, frames, points, slots, outdoor


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--shapes", default="ogcdr,kittisf")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--time_window_size", type=int, default=3)
    ap.add_argument("--save", default=None)
    args = ap.parse_args(argv)
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import ogc_amd  # noqa: F401  (loads the native library)
    from ogc_amd import vote
    from ogc_amd.utils.synthetic import make_sequence
    if not torch.cuda.is_available():
        raise SystemExit("bench_vote.py needs the GPU: a timing taken elsewhere says nothing")
    for name in args.shapes.split(","):
        S, T, N, K, outdoor = SHAPES[name]
        pcs, masks, flows = [], [], []
        g = torch.Generator().manual_seed(99)
        for s in range(S):
            pc, segm, fl = make_sequence(T, N, K, seed=500 + s, outdoor=outdoor)
            m = (3.0 * torch.eye(K)[segm] + torch.randn(T, N, K, generator=g)).softmax(-1)
            m = torch.stack([m[t][:, torch.randperm(K, generator=g)] for t in range(T)])
            pcs.append(pc); masks.append(m)
            flows.append(torch.cat([fl, torch.zeros_like(fl[:1])]))             # the loader's redundant last entry
        pc, mask, flow = (torch.cat(x).cuda().contiguous() for x in (pcs, masks, flows))

        def run():
            with torch.no_grad():
                return vote.vote_batch(pc, mask, flow, T, args.time_window_size)
        for _ in range(args.warmup):
            run()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        times = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = run()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        peak = torch.cuda.max_memory_allocated()
        times.sort()
        print(json.dumps({"shape": name, "scenes": S, "frames": T, "points": N, "slots": K, "root": os.path.abspath(args.root),
                          "ms_median": round(times[len(times) // 2], 3), "ms_min": round(times[0], 3),
                          "ms_max": round(times[-1], 3), "reps": args.reps,
                          "peak_MiB": round(peak / 2 ** 20, 1), "peak_above_inputs_MiB": round((peak - base) / 2 ** 20, 1),
                          "rows_sum_to_one": bool(torch.allclose(out.sum(-1), torch.ones_like(out[..., 0]), atol=1e-5))}),
              flush=True)
        if args.save:
            torch.save(out.cpu(), "%s_%s.pt" % (args.save, name))
        del out, pc, mask, flow


if __name__ == "__main__":
    main()

"""Fixtures of the rigid point-to-point ICP (ogc_rigid_icp, ogc_amd/utils/icp_util.py) -> tests/golden/icp.npz.

    python tests/golden/make_icp_golden.py REFERENCE_ROOT          (CPU only, a few seconds; needs scikit-learn)

The expected values are what the reference's `icp` (utils/icp_util.py:73-124, imported by path from REFERENCE_ROOT at generation
time only) returns in float64 on the float32 inputs stored here.  `icp_trace` below is this repository's own float64 numpy
statement of the same algorithm with an exhaustive nearest-neighbour search; it records what the reference does not return —
the indices of the last search and, per iteration, the margins that make every discrete result (correspondences, iteration
count, reflection branch) independent of summation order:

    gap         second-nearest minus nearest distance, over all points               >= 1e-6
    tol margin  | |prev_error - mean_error| - tolerance |                            >= 1e-6
    sv ratio    smallest / largest singular value of the cross-covariance            >= 1e-4

The generator asserts the three thresholds on every iteration of every case, asserts that `icp_trace` and the reference agree
(same `i` and distances to 1e-9; T to 1e-9 once the last fit centres the float32 source in float32 as numpy does for the
reference, see icp_trace; the stored T is the reference's, and `f32_centring_effect` in the metadata says how far the all-float64
T lies from it), and stores the two smallest gaps / tolerance margins it saw.  Seeds are searched upwards
from 0 until a construction meets its conditions, so a rerun reproduces the file.

Cases (all with the reference's defaults max_iterations = 20, tolerance = 1e-3 unless noted):
    a5, a8, a16   unrelated uniform clouds in a flat 10 x 1 x 10 box; the `det R < 0` branch is taken in at least one iteration
                  with (s1 - s2) / s0 > 0.05, so that the reflection fix is well conditioned
    b             n = 200    less than one workgroup, not a multiple of 64
    c             n = 1024   the flow-prediction driver's size
    d             n = 1500   more points than threads, ragged tail
    e             three n = 256 pairs that stop at different iterations, the second with an initial pose
    f             the data of c with max_iterations = 3: the cap is hit, i == 2
b-e: points uniform in 40 x 4 x 40 m; the second frame is a window of the same set shifted by 20 %, rotated 0.03-0.05 rad about
y, translated by about 1 m, with 0.02 m noise, shuffled."""
import importlib.util
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GAP_MIN, TOL_MARGIN_MIN, SV_RATIO_MIN = 1e-6, 1e-6, 1e-4


def best_fit(A, B):
    """Least-squares rigid transform A -> B of corresponding (n, 3) float64 sets: (T (4, 4), singular values, reflected)."""
    ca, cb = A.mean(0), B.mean(0)
    H = (A - ca).T @ (B - cb)
    U, S, Vt = np.linalg.svd(H)
    R = Vt.T @ U.T
    reflected = bool(np.linalg.det(R) < 0)
    if reflected:
        Vt[2] *= -1
        R = Vt.T @ U.T
    T = np.identity(4)
    T[:3, :3] = R
    T[:3, 3] = cb - R @ ca
    return T, S, reflected


def nearest(src, dst):
    """Exhaustive float64 search: (distance, index, gap to the second nearest) per source point; lower index on ties."""
    d = np.sqrt(((src[:, None, :] - dst[None, :, :]) ** 2).sum(-1))
    idx = d.argmin(1)
    two = np.partition(d, 1, axis=1)[:, :2]
    return d[np.arange(len(src)), idx], idx, two[:, 1] - two[:, 0]


def icp_trace(A, B, init_pose=None, max_iterations=20, tolerance=0.001):
    """The algorithm of the issue in float64 numpy.  Returns (T, distances, i, indices, trace); trace holds, per iteration,
    gap / tol_margin / sv (singular values) / reflected."""
    A64, dst = np.asarray(A, np.float64), np.asarray(B, np.float64)
    src = np.concatenate([A64, np.ones((len(A64), 1))], 1).T                  # (4, n) homogeneous
    if init_pose is not None:
        src = np.asarray(init_pose, np.float64) @ src
    prev, trace = 0.0, []
    for i in range(max_iterations):
        dist, idx, gap = nearest(src[:3].T, dst)
        T, S, reflected = best_fit(src[:3].T, dst[idx])
        src = T @ src
        mean = dist.mean()
        trace.append({"gap": float(gap.min()), "tol_margin": float(abs(abs(prev - mean) - tolerance)), "sv": S.tolist(),
                      "reflected": reflected})
        if abs(prev - mean) < tolerance:
            break
        prev = mean
    T, S, _ = best_fit(A64, src[:3].T)
    # the reference hands its float32 input to this last fit, so numpy centres it in float32 (mean and difference both): kept
    # apart, as the kernel and the value returned here are float64 throughout
    trace.append({"sv": S.tolist(), "T_f32_centred": best_fit(np.asarray(A), src[:3].T)[0]})
    return T, dist, i, idx, trace


def margins(trace):
    gaps = [t["gap"] for t in trace if "gap" in t]
    tols = [t["tol_margin"] for t in trace if "tol_margin" in t]
    ratio = min(t["sv"][2] / t["sv"][0] for t in trace)
    return min(gaps), min(tols), ratio


def holds(trace):
    g, t, r = margins(trace)
    return g >= GAP_MIN and t >= TOL_MARGIN_MIN and r >= SV_RATIO_MIN


def rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def flat_pair(n, seed):
    rs = np.random.RandomState(seed)
    box = np.array([10.0, 1.0, 10.0])
    return (rs.rand(n, 3) * box).astype(np.float32), (rs.rand(n, 3) * box).astype(np.float32)


def window_pair(n, seed):
    """Frame 1: the first n of 1.2 n points; frame 2: the last n, moved rigidly, with noise, shuffled.  Also the motion."""
    rs = np.random.RandomState(seed)
    m = n + n // 5
    P = (rs.rand(m, 3) - 0.5) * np.array([40.0, 4.0, 40.0])
    R = rot_y(rs.uniform(0.03, 0.05) * rs.choice([-1.0, 1.0]))
    t = rs.uniform(-1.0, 1.0, 3) * np.array([0.7, 0.1, 0.7])
    Q = P[m - n:] @ R.T + t + rs.randn(n, 3) * 0.02
    return P[:n].astype(np.float32), Q[rs.permutation(n)].astype(np.float32), R, t


def search(make, accept, limit=200):
    for seed in range(limit):
        made = make(seed)
        out = icp_trace(*made[0], **made[1])
        if holds(out[4]) and accept(out):
            return seed, made, out
    raise RuntimeError("no seed below %d meets the conditions" % limit)


if __name__ == "__main__":
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("OGC_REFERENCE_ROOT")
    assert ref_root and os.path.isdir(ref_root), "give the checkout of the reference project: make_icp_golden.py REFERENCE_ROOT"
    spec = importlib.util.spec_from_file_location("reference_icp_util", os.path.join(ref_root, "utils", "icp_util.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    arrays, meta, all_traces = {}, {"cases": {}}, []
    centring = [0.0, 0.0]   # largest |T_reference - T_float64|: rotation entries, translation / largest |coordinate|

    def record(name, inputs_key, srcs, dsts, inits, kw, outs):
        """One (possibly batched) case: the reference's results per pair, checked against icp_trace's."""
        Ts, ds, its, idxs = [], [], [], []
        for b in range(len(srcs)):
            init = None if inits is None else inits[b]
            T, dist, i = ref.icp(srcs[b], dsts[b], init_pose=init, **kw)
            T2, dist2, i2, idx2, trace = outs[b]
            assert i == i2, (name, i, i2)
            assert np.abs(T - trace[-1]["T_f32_centred"]).max() < 1e-9 and np.abs(dist - dist2).max() < 1e-9, name
            assert holds(trace), (name, margins(trace))
            centring[0] = max(centring[0], float(np.abs(T[:3, :3] - T2[:3, :3]).max()))
            centring[1] = max(centring[1], float(np.abs(T[:3, 3] - T2[:3, 3]).max() / np.abs(dsts[b]).max()))
            all_traces.extend(trace[:-1] + [{"sv": trace[-1]["sv"]}])
            Ts.append(T); ds.append(dist); its.append(i); idxs.append(idx2)
        if inputs_key == name:
            arrays[name + "_src"], arrays[name + "_dst"] = np.stack(srcs), np.stack(dsts)
            if inits is not None:
                arrays[name + "_init"] = np.stack(inits)
        arrays[name + "_T"], arrays[name + "_distances"] = np.stack(Ts), np.stack(ds)
        arrays[name + "_iters"], arrays[name + "_indices"] = np.array(its, np.int32), np.stack(idxs).astype(np.int16)
        meta["cases"][name] = {"inputs": inputs_key, "has_init": inits is not None, "iters": [int(v) for v in its],
                               "max_iterations": kw.get("max_iterations", 20), "tolerance": kw.get("tolerance", 0.001)}

    for n in (5, 8, 16):
        seed, made, out = search(lambda s: (flat_pair(n, s), {}),
                                 lambda o: any(t.get("reflected") and (t["sv"][1] - t["sv"][2]) / t["sv"][0] > 0.05
                                               for t in o[4]))
        record("a%d" % n, "a%d" % n, [made[0][0]], [made[0][1]], None, {}, [out])
        meta["cases"]["a%d" % n]["seed"] = seed

    for name, n in (("b", 200), ("c", 1024), ("d", 1500)):
        seed, made, out = search(lambda s: (window_pair(n, s)[:2], {}), lambda o: 4 <= o[2] <= 9)
        record(name, name, [made[0][0]], [made[0][1]], None, {}, [out])
        meta["cases"][name]["seed"] = seed
        if name == "c":
            c_pair = made[0]
            reps = []
            for _ in range(5):
                t0 = time.perf_counter()
                ref.icp(*c_pair)
                reps.append((time.perf_counter() - t0) * 1e3)
            meta["reference_cpu_ms_case_c"] = round(float(np.median(reps)), 2)

    # e: three pairs with different iteration counts; the second starts from a pose close to its true motion
    srcs, dsts, inits, outs, seen, seed = [], [], [], [], set(), 0
    while len(srcs) < 3:
        A, B, R, t = window_pair(256, 1000 + seed)
        init = np.identity(4)
        if len(srcs) == 1:
            init[:3, :3], init[:3, 3] = rot_y(0.01) @ R, t + 0.2
        out = icp_trace(A, B, init_pose=init)
        if holds(out[4]) and out[2] not in seen and out[2] < 19:
            seen.add(out[2])
            srcs.append(A); dsts.append(B); inits.append(init); outs.append(out)
        seed += 1
        assert seed < 200
    record("e", "e", srcs, dsts, inits, {}, outs)

    out = icp_trace(*c_pair, max_iterations=3)
    assert out[2] == 2 and meta["cases"]["c"]["iters"][0] > 2       # the cap ends the loop, not the tolerance
    record("f", "c", [c_pair[0]], [c_pair[1]], None, {"max_iterations": 3}, [out])

    gaps = sorted(t["gap"] for t in all_traces if "gap" in t)
    tols = sorted(t["tol_margin"] for t in all_traces if "tol_margin" in t)
    meta["smallest_gaps"], meta["smallest_tol_margins"] = gaps[:2], tols[:2]
    meta["smallest_sv_ratio"] = min(t["sv"][2] / t["sv"][0] for t in all_traces)
    meta["f32_centring_effect"] = {"rotation": centring[0], "translation_rel": centring[1]}
    meta["thresholds"] = {"gap": GAP_MIN, "tol_margin": TOL_MARGIN_MIN, "sv_ratio": SV_RATIO_MIN}
    arrays["meta"] = np.array(json.dumps(meta, sort_keys=True))
    path = os.path.join(HERE, "icp.npz")
    np.savez_compressed(path, **arrays)
    print(json.dumps(meta, indent=1, sort_keys=True))
    print(path, os.path.getsize(path), "bytes")

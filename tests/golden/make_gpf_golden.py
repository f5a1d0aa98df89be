"""Writes tests/golden/gpf.npz: clouds and what ground-plane fitting makes of them, for ogc_ground_plane_fit
(ogc_amd/csrc/ground_plane.hip) and ogc_amd/utils/gpf_util.py.  CPU only, numpy only.

    python tests/golden/make_gpf_golden.py

The expected values come from `gpf_trace`, a float64 statement of the loop of the reference's `ground_plane_fitting`
(utils/gpf_util.py:45-66) written for this repository: the reference's own function needs scikit-spatial, which the build
machine lacks, and its CUDA FPS.  Of scikit-spatial it uses `Plane.best_fit`, which is the centroid plus the last left singular
vector of the centred points transposed, and which refuses fewer than 3 points and collinear points (`matrix_rank` of the
centred points below 2); any exception raises the seed threshold by 0.05 and starts the cloud again, until the threshold
exceeds 0.8.

What makes EQUAL masks and attempt counts a fair demand of another implementation is asserted here on every attempt and
iteration of every case (THRESHOLDS): no height within 1e-6 of a seed threshold, no distance within 1e-6 of thresh_dist, every
fitted selection either exactly degenerate by construction (points on a line whose coordinates have few mantissa bits: every
cross product of two centred points is an exact zero; for the axis-aligned line of cases retry, giveup and batch the centred
points are exact zeros in two columns, case tilted has a line across x and z) or with sigma2 / sigma1 >= 1e-3, and a last fit with sigma2 / sigma1 >= 0.05 and sigma3 / sigma2 <=
0.5, which conditions the plane.  The same mirror run in float32 — the reference computes in the dtype of its cloud — must
give identical masks and attempt counts.  Seeds are searched upwards from 0 until a construction meets all of that, so a rerun
reproduces the file.  The two smallest margins of each kind are recorded in the metadata.
"""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
THRESHOLDS = {"height": 1e-6, "dist": 1e-6, "rank": 1e-3, "final_s2_s1": 0.05, "final_s3_s2": 0.5}
SEED_STEP, SEED_GIVE_UP = 0.05, 0.8


class FitRefused(Exception):
    pass


def best_fit(pts, record=None):
    """Plane.best_fit: (centre, normal, singular values of the centred points)."""
    if pts.shape[0] < 3:
        raise FitRefused("fewer than 3 points")
    if not np.isfinite(pts).all():
        raise FitRefused("not finite")
    centre = pts.mean(0)
    centred = pts - centre
    s = np.linalg.svd(centred, compute_uv=False)
    if record is not None:
        # exactly collinear: the cross products with the longest centred point are exact zeros (exact for few-bit coordinates)
        longest = centred[np.abs(centred).sum(1).argmax()].astype(np.float64)
        degenerate = not np.cross(centred.astype(np.float64), longest).any()
        record["rank"].append(None if degenerate else float(s[1] / s[0]))
    if np.linalg.matrix_rank(centred) < 2:
        raise FitRefused("collinear")
    u = np.linalg.svd(centred.T)[0]
    return centre, u[:, 2], s


def gpf_trace(pc, n_iter=5, n_lpr=200, thresh_seed=0.4, thresh_dist=0.4, vertical_axis=1, dtype=np.float64, record=None):
    """pc (n, 3) -> (is_ground (n,) bool, plane (6,) float64: centre, unit normal with a vertical component >= 0, attempts).
    After giving up mask and plane are zero.  `record`, a dict, receives the margins (module docstring)."""
    pc = np.asarray(pc).astype(dtype)
    if record is not None:
        for k in ("height", "dist", "rank", "final"):
            record.setdefault(k, [])
    height = pc[:, vertical_axis]
    lpr = np.partition(height, n_lpr)[:n_lpr].mean()
    attempts = 0
    while True:
        attempts += 1
        try:
            limit = lpr + dtype(thresh_seed)
            if record is not None:
                record["height"].append(float(np.abs(height.astype(np.float64) - np.float64(limit)).min()))
            seed = pc[height < limit]
            for _ in range(n_iter):
                centre, normal, s = best_fit(seed, record)
                dist = np.abs(np.einsum("nj,j->n", pc - centre, normal))
                if record is not None:
                    record["dist"].append(float(np.abs(dist.astype(np.float64) - thresh_dist).min()))
                is_ground = dist < dtype(thresh_dist)
                seed = pc[is_ground]
            break
        except FitRefused:
            thresh_seed += SEED_STEP
            if thresh_seed > SEED_GIVE_UP:
                return np.zeros(pc.shape[0], dtype=bool), np.zeros(6), attempts
    if record is not None:
        record["final"].append((float(s[1] / s[0]), float(s[2] / s[1])))
    normal = normal.astype(np.float64) / np.linalg.norm(normal.astype(np.float64))
    if normal[vertical_axis] < 0:
        normal = -normal
    return is_ground, np.concatenate([centre.astype(np.float64), normal]), attempts


def final_mask(points, plane, thresh_dist=0.4):
    """The reference's last two lines on all points, float64; a plane of zeros labels nothing."""
    if not plane[3:].any():
        return np.zeros(points.shape[0], dtype=bool)
    return np.abs((points.astype(np.float64) - plane[:3]) @ plane[3:]) < thresh_dist


# ---- clouds ----------------------------------------------------------------------------------------------------------------
def sheet_cloud(n, rs, base=-1.7, ground_frac=0.6, quant=None, extent=20.0):
    """A tilted ground sheet (3 cm / m in x, 2 cm / m in z, sigma = 0.03 m) under uniform clutter 0.6 .. 3.6 m above it."""
    n_ground = max(3, int(n * ground_frac))
    xz = (rs.rand(n, 2) - 0.5) * 2 * extent
    sheet = base + 0.03 * xz[:, 0] + 0.02 * xz[:, 1]
    y = np.where(np.arange(n) < n_ground, sheet + 0.03 * rs.randn(n), sheet + 0.6 + 3.0 * rs.rand(n))
    if quant:
        y = np.round(y / quant) * quant
    pc = np.stack([xz[:, 0], y, xz[:, 1]], 1)
    return pc[rs.permutation(n)].astype(np.float32)


def line_cloud(n, rs, gap, slope=0.0):
    """The lowest 8 points on the line y = -2, z = 3 + slope * x (coordinates with few mantissa bits: their sums and means are
    exact in float32 too), the rest a sheet cloud whose lowest point lies `gap` above the line."""
    rest = sheet_cloud(n - 8, rs).astype(np.float64)
    rest[:, 1] += (-2.0 + gap) - rest[:, 1].min()
    x = -3.5 + np.arange(8)
    line = np.stack([x, np.full(8, -2.0), 3.0 + slope * x], 1)
    return np.concatenate([line, rest])[rs.permutation(n)].astype(np.float32)


def tiny_cloud(n, rs):
    """n = 5: two low points, the others about half a metre up, so that the first seed holds fewer than 3 points."""
    pc = (rs.rand(n, 3) - 0.5) * np.array([10.0, 0.0, 10.0])
    pc[:, 1] = np.where(np.arange(n) < 2, -2.0 + 0.05 * rs.rand(n), -1.5 + 0.3 * rs.rand(n))
    return pc[rs.permutation(n)].astype(np.float32)


def axis_cloud(n, rs):
    return np.ascontiguousarray(sheet_cloud(n, rs)[:, [0, 2, 1]])      # z is up


def _ties_straddle(height, n_lpr):
    """At least three copies of the n_lpr-th smallest height on either side of the partition."""
    h = np.sort(height)
    return (h[:n_lpr] == h[n_lpr - 1]).sum() >= 3 and (h[n_lpr:] == h[n_lpr - 1]).sum() >= 3


def _seed_signs(height, n_lpr):
    """Negative heights among the n_lpr smallest and on both sides of 0 inside the first seed."""
    h = np.sort(height.astype(np.float64))
    seed = h[h < h[:n_lpr].mean() + 0.4]
    return h[n_lpr - 1] < 0 and (seed < 0).sum() >= 10 and (seed > 0).sum() >= 10


# name -> (inputs key, builder(rs) -> (B, n, 3) or None when `inputs` names another case, arguments, accept(attempts, masks, clouds))
def _one(fn):
    return lambda rs: fn(rs)[None]


CASES = [
    ("g5", _one(lambda rs: tiny_cloud(5, rs)), {"n_lpr": 3}, lambda a, m, pc: a[0] >= 2 and m.any()),
    ("g64", _one(lambda rs: sheet_cloud(64, rs)), {"n_lpr": 10}, None),
    ("g200", _one(lambda rs: sheet_cloud(200, rs)), {"n_lpr": 20}, None),
    ("g2048", _one(lambda rs: sheet_cloud(2048, rs)), {"n_lpr": 50}, None),
    ("g3000", _one(lambda rs: sheet_cloud(3000, rs)), {"n_lpr": 50}, None),
    ("g8192", _one(lambda rs: sheet_cloud(8192, rs)), {"n_lpr": 200}, None),
    ("ties", _one(lambda rs: sheet_cloud(200, rs, quant=0.125)), {"n_lpr": 20}, lambda a, m, pc: _ties_straddle(pc[0, :, 1], 20)),
    ("neg", _one(lambda rs: sheet_cloud(200, rs, base=0.5)), {"n_lpr": 20}, lambda a, m, pc: _seed_signs(pc[0, :, 1], 20)),
    ("axis2", _one(lambda rs: axis_cloud(200, rs)), {"n_lpr": 20, "vertical_axis": 2}, None),
    ("iter1", "g200", {"n_lpr": 20, "n_iter": 1}, None),
    ("retry", _one(lambda rs: line_cloud(200, rs, 0.55 + 0.15 * rs.rand())), {"n_lpr": 8}, lambda a, m, pc: 4 <= a[0] <= 7 and m.any()),
    ("tilted", _one(lambda rs: line_cloud(200, rs, 0.55 + 0.15 * rs.rand(), slope=0.75)), {"n_lpr": 8},
     lambda a, m, pc: 4 <= a[0] <= 7 and m.any()),
    ("giveup", _one(lambda rs: line_cloud(200, rs, 1.25 + 0.1 * rs.rand())), {"n_lpr": 8}, lambda a, m, pc: a[0] == 8 and not m.any()),
    ("batch", lambda rs: np.stack([sheet_cloud(256, rs), line_cloud(256, rs, 0.55 + 0.15 * rs.rand()),
                                   line_cloud(256, rs, 1.25 + 0.1 * rs.rand()), sheet_cloud(256, rs, base=-1.2)]),
     {"n_lpr": 8}, lambda a, m, pc: a[0] == 1 and 4 <= a[1] <= 7 and a[2] == 8 and not m[2].any() and a[3] == 1),
]
DEFAULTS = {"n_iter": 5, "n_lpr": 200, "thresh_seed": 0.4, "thresh_dist": 0.4, "vertical_axis": 1}


def _meets(record):
    ranks = [r for r in record["rank"] if r is not None]
    return (min(record["height"]) >= THRESHOLDS["height"] and (not record["dist"] or min(record["dist"]) >= THRESHOLDS["dist"])
            and (not ranks or min(ranks) >= THRESHOLDS["rank"])
            and all(a >= THRESHOLDS["final_s2_s1"] and b <= THRESHOLDS["final_s3_s2"] for a, b in record["final"]))


def _solve(pcs, kw):
    """Both mirrors on every cloud of a case: (masks, planes, attempts, record) or None when a condition fails."""
    record, masks, planes, attempts = {}, [], [], []
    for pc in pcs:
        m, p, a = gpf_trace(pc, record=record, **kw)
        m32, _, a32 = gpf_trace(pc, dtype=np.float32, **kw)
        if not np.array_equal(m, m32) or a != a32:
            return None
        masks.append(m)
        planes.append(p)
        attempts.append(a)
    if not _meets(record):
        return None
    return np.stack(masks), np.stack(planes), np.asarray(attempts, dtype=np.int32), record


def build():
    out, meta = {}, {"thresholds": THRESHOLDS, "cases": {}}
    margins = {"height": [], "dist": [], "rank": [], "final_s2_s1": [], "final_s3_s2": []}
    for name, builder, args, accept in CASES:
        kw = dict(DEFAULTS, **args)
        if isinstance(builder, str):
            inputs, seeds = builder, [meta["cases"][builder]["seed"]]
        else:
            inputs, seeds = name, range(1000)
        for seed in seeds:
            pcs = out[inputs + "_pc"] if isinstance(builder, str) else builder(np.random.RandomState(seed))
            solved = _solve(pcs, kw)
            if solved is not None and (accept is None or accept(solved[2].tolist(), solved[0], pcs)):
                break
        else:
            raise RuntimeError("no seed gives case %s" % name)
        masks, planes, attempts, record = solved
        out[inputs + "_pc"] = pcs
        out[name + "_is_ground"], out[name + "_plane"], out[name + "_attempts"] = masks, planes, attempts
        meta["cases"][name] = dict(kw, inputs=inputs, seed=int(seed), B=int(pcs.shape[0]), n=int(pcs.shape[1]))
        margins["height"] += record["height"]
        margins["dist"] += record["dist"]
        margins["rank"] += [r for r in record["rank"] if r is not None]
        margins["final_s2_s1"] += [a for a, _ in record["final"]]
        margins["final_s3_s2"] += [b for _, b in record["final"]]
        print("%-7s seed %3d attempts %s ground %s" % (name, seed, attempts.tolist(), masks.sum(1).tolist()))
    meta["smallest_height_margins"] = sorted(margins["height"])[:2]
    meta["smallest_dist_margins"] = sorted(margins["dist"])[:2]
    meta["smallest_rank_ratios"] = sorted(margins["rank"])[:2]
    meta["smallest_final_s2_s1"] = sorted(margins["final_s2_s1"])[:2]
    meta["largest_final_s3_s2"] = sorted(margins["final_s3_s2"])[-2:]
    out["meta"] = np.asarray(json.dumps(meta))
    return out, meta


if __name__ == "__main__":
    out, meta = build()
    path = os.path.join(HERE, "gpf.npz")
    np.savez_compressed(path, **out)
    print({k: v for k, v in meta.items() if k != "cases"})
    print("%s: %d bytes" % (path, os.path.getsize(path)))

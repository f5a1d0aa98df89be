"""Helpers of the OGC-DR preparation tests (no tests here): numpy mirrors of the three operators of DESIGN §4m and of the reference's
crop expression, and the inputs the CPU and the GPU files share."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xffffffff)


def philox4x32_10(counter, key):
    """counter: four uint64 arrays holding 32-bit words, key: two Python ints (32 bits each) -> four uint64 arrays of 32-bit words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK32 for c in counter)
    k0, k1 = int(key[0]) & 0xffffffff, int(key[1]) & 0xffffffff
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                      # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & MASK32, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & MASK32
        k0, k1 = (k0 + W0) & 0xffffffff, (k1 + W1) & 0xffffffff
    return c0, c1, c2, c3


def uniform53(hi, lo):
    return (((hi >> np.uint64(5)) << np.uint64(26)) | (lo >> np.uint64(6))).astype(np.float64) * 2.0 ** -53


def candidate_uniforms(seed, mesh, count):
    """The three uniforms of candidates 0 .. count - 1 of mesh `mesh`: (count, 3) float64."""
    seed = int(seed) & 0xffffffffffffffff
    key = (seed & 0xffffffff, seed >> 32)
    j = np.arange(count, dtype=np.uint64)
    m = np.full(count, mesh, dtype=np.uint64)
    zero = np.zeros(count, dtype=np.uint64)
    a = philox4x32_10((j, m, zero, zero), key)
    b = philox4x32_10((j, m, zero + np.uint64(1), zero), key)
    return np.stack([uniform53(a[0], a[1]), uniform53(a[2], a[3]), uniform53(b[0], b[1])], 1)


def face_areas(vertices, faces):
    v = np.asarray(vertices, dtype=np.float64)
    return 0.5 * np.linalg.norm(np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]]), axis=1)


def cumulative_areas(vertices, faces, face_offsets):
    areas = face_areas(vertices, faces)
    cum = np.zeros(len(faces), dtype=np.float64)
    for m in range(len(face_offsets) - 1):
        lo, hi = face_offsets[m], face_offsets[m + 1]
        cum[lo:hi] = np.cumsum(areas[lo:hi])
    return cum


def candidates_mirror(vertices, faces, cum_area, face_offsets, cand_offsets, seed):
    """The mirror of ogc_surface_candidates -> (points (C, 3) float64, face_idx (C,) int32, barycentric (C, 2) float64)."""
    points, face_idx, bary = [], [], []
    for m in range(len(face_offsets) - 1):
        count = int(cand_offsets[m + 1] - cand_offsets[m])
        if count == 0:
            continue
        f0, f1 = int(face_offsets[m]), int(face_offsets[m + 1])
        cum = cum_area[f0:f1]
        u = candidate_uniforms(seed, m, count)
        pick = u[:, 0] * cum[-1]
        f = np.minimum(np.searchsorted(cum, pick, side="right"), np.searchsorted(cum, cum[-1], side="left")) + f0
        u1, u2 = u[:, 1].copy(), u[:, 2].copy()
        flip = u1 + u2 > 1.0
        u1[flip], u2[flip] = 1.0 - u1[flip], 1.0 - u2[flip]
        o = vertices[faces[f, 0]]
        e1, e2 = vertices[faces[f, 1]] - o, vertices[faces[f, 2]] - o
        points.append((o + u1[:, None] * e1) + u2[:, None] * e2)
        face_idx.append(f.astype(np.int32))
        bary.append(np.stack([u1, u2], 1))
    if not points:
        return np.zeros((0, 3)), np.zeros(0, dtype=np.int32), np.zeros((0, 2))
    return np.concatenate(points), np.concatenate(face_idx), np.concatenate(bary)


def within(p, q, r):
    """The pair test of the thinning, exactly: ((dx*dx) + (dy*dy)) + (dz*dz) <= r * r in float64; p, q (..., 3)."""
    d = np.asarray(p, dtype=np.float64) - np.asarray(q, dtype=np.float64)
    return ((d[..., 0] * d[..., 0]) + (d[..., 1] * d[..., 1])) + (d[..., 2] * d[..., 2]) <= np.float64(r) * np.float64(r)


def _thin_loop(points, r):
    n = len(points)
    keep = np.zeros(n, dtype=np.int32)
    kept = []
    for i in range(n):
        if not kept or not within(points[kept], points[i], r).any():
            keep[i] = 1
            kept.append(i)
    return keep


def _thin_tree(points, r):
    from scipy.spatial import cKDTree
    n = len(points)
    pairs = cKDTree(points).query_pairs(float(r) * (1.0 + 1e-9) + 1e-300, output_type="ndarray")    # a superset; the exact test decides
    pairs = pairs[within(points[pairs[:, 0]], points[pairs[:, 1]], r)]
    lo, hi = pairs.min(1), pairs.max(1)
    order = np.argsort(hi, kind="stable")
    lo, hi = lo[order], hi[order]
    first = np.searchsorted(hi, np.arange(n + 1))
    keep = np.ones(n, dtype=np.int32)
    for i in range(n):
        if keep[lo[first[i]:first[i + 1]]].any():
            keep[i] = 0
    return keep


def greedy_thin_reference(points, cand_offsets, radius, method=None):
    """The sequential definition of ogc_surface_thin -> keep (C,) int32.  A plain loop for meshes of up to 4096 candidates,
    cKDTree.query_pairs and one ordered pass beyond (method "loop" / "tree" forces one)."""
    points = np.asarray(points, dtype=np.float64)
    keep = np.zeros(len(points), dtype=np.int32)
    for m in range(len(cand_offsets) - 1):
        lo, hi = int(cand_offsets[m]), int(cand_offsets[m + 1])
        if hi == lo:
            continue
        use = method or ("loop" if hi - lo <= 4096 else "tree")
        keep[lo:hi] = (_thin_loop if use == "loop" else _thin_tree)(points[lo:hi], radius[m])
    return keep


def thin_rounds_simulation(points, r, rs=None, stale=0.0):
    """The round form on one mesh, simulated: -> (keep, rounds).  Without `rs` a round sees the states as its launch found them.
    With a RandomState the undecided act in random order and see what the running round has written so far, and each state a
    candidate reads appears as still undecided with probability `stale` — the freedoms the device has.  (The lowest undecided
    index reads the truth: its neighbours were decided by earlier launches.)"""
    points = np.asarray(points, dtype=np.float64)
    n = len(points)
    nb = [np.nonzero(within(points[:i], points[i], r))[0] for i in range(n)]
    state = np.full(n, -1, dtype=np.int32)
    rounds = 0
    while (state == -1).any():
        rounds += 1
        assert rounds <= n + 1
        undecided = np.nonzero(state == -1)[0]
        source = state.copy() if rs is None else state
        for i in (undecided if rs is None else rs.permutation(undecided)):
            seen = source[nb[i]].copy()
            if rs is not None and i != undecided[0]:
                seen[rs.rand(len(seen)) < stale] = -1
            if (seen == 1).any():
                state[i] = 0
            elif not (seen == -1).any():
                state[i] = 1
    return state, rounds


def nearest_label_reference(query, source, labels):
    """scipy cdist, then argmin: query (B, Nq, 3), source (B, Ns, 3) float32, labels (B, Ns) -> (label (B, Nq), idx (B, Nq)) int32."""
    from scipy.spatial.distance import cdist
    idx = np.stack([cdist(q, s).argmin(1) for q, s in zip(query, source)]).astype(np.int32)
    return np.take_along_axis(np.asarray(labels), idx.astype(np.int64), 1).astype(np.int32), idx


GROUND_THICKNESS, GROUND_HEIGHT, WALL_THICKNESS = 0.01, -0.5, 0.01
GROUND_LEVEL = GROUND_HEIGHT + GROUND_THICKNESS


def crop_mask_reference(points, xz_range):
    """The five thickness tests of data_prepare/ogcdr/sample_pointcloud.py:69-73 with numpy's own typing, which is what decides the
    points on the bounds: `points` is a float32 array and the y bound a Python float, so numpy compares in float32 against the
    bound rounded to float32; `xz_range` is a float64 array, so the x and z bounds are float64 scalars and those four tests
    compare in float64.  Each bound is built in the reference's order of operations: half the range, the wall, then the 1e-4."""
    assert points.dtype == np.float32 and np.asarray(xz_range).dtype == np.float64
    mask = points[:, 1] > (GROUND_LEVEL - 1e-4)
    for column, extent in ((2, xz_range[1]), (0, xz_range[0])):
        half = extent / 2.                                      # np.float64
        mask &= points[:, column] > (-half + WALL_THICKNESS - 1e-4)
        mask &= points[:, column] < (half - WALL_THICKNESS + 1e-4)
    return mask


def cube_mesh(size=1.0, centre=(0.0, 0.0, 0.0)):
    """A closed box of 12 triangles: (vertices (8, 3) float64, faces (12, 3) int32)."""
    size = np.broadcast_to(np.asarray(size, dtype=np.float64), (3,))
    v = np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)], dtype=np.float64) * size + np.asarray(centre)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                  [1, 5, 7], [1, 7, 3]], dtype=np.int32)
    return v, f


def cube_surface_points(n, seed, size=1.0):
    """n candidates on a cube by the candidate mirror -> (n, 3) float64."""
    v, f = cube_mesh(size)
    cum = cumulative_areas(v, f, [0, 12])
    return candidates_mirror(v, f, cum, [0, 12], [0, n], seed)[0]

"""ogc_rigid_icp / ogc_amd.utils.icp_util on the MI355X against tests/golden/icp.npz — what the reference's `icp`
(utils/icp_util.py:73-124) returns in float64 on the same float32 clouds (tests/golden/make_icp_golden.py).

Discrete results must be equal: `iters`, and the correspondences of the last search.  The kernel returns distances, not
indices; the fixture's smallest gap between nearest and second-nearest distance is 5.8e-5, so a distance that agrees with the
distance to the fixture's index to DIST_TOL = 1e-8 cannot belong to any other index.

Tolerances:
  T           the reference centres the float32 source of its LAST fit in float32 (numpy keeps the dtype of `A`), the kernel in
              float64 like everything else; the fixture records how far an all-float64 numpy evaluation lies from the stored T
              (`f32_centring_effect`: 4.0e-9 on rotation entries, 5.6e-8 x largest |coordinate| on the translation), which is
              the floor of any comparison.  The kernel's own deviation over all cases: 4.0e-9 on rotation entries (case a8),
              6.9e-8 x cloud extent on the translation (case a5) — figures of the kernel source run thread for thread on the
              host, the same IEEE double operations in the same order; NOT yet measured on an MI355X, each test
              prints its figures.  The bound is 100x that deviation, capped at 1e-6 on rotation entries and 1e-6 x cloud
              extent on the translation — the resolution at which the fp32 flow made from T changes: 4.0e-7 and the cap.
  distances   float64 round-off through at most 8 fits of sums of <= 1500 terms over coordinates <= 30 m, conditioned by the
              smallest singular-value ratio 5e-4 of the fixture: 1500 * 1.1e-16 * 30 / 5e-4 = 1e-8.
  flow        atol 1e-5, about one fp32 ulp at the 40-60 m the coordinates reach."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ("a5", "a8", "a16", "b", "c", "d", "e", "f")
MEASURED_ROT, MEASURED_TRANS_REL = 4.0e-9, 6.9e-8       # largest deviations of the kernel over all cases (see above)
ROT_TOL = min(100 * MEASURED_ROT, 1e-6)
TRANS_TOL_REL = min(100 * MEASURED_TRANS_REL, 1e-6)     # x cloud extent
DIST_TOL = 1e-8


@pytest.fixture(scope="module")
def golden():
    data = np.load(os.path.join(HERE, "golden", "icp.npz"))
    return data, json.loads(str(data["meta"]))


def _inputs(golden, name):
    data, meta = golden
    case = meta["cases"][name]
    key = case["inputs"]
    src, dst = torch.from_numpy(data[key + "_src"]).cuda(), torch.from_numpy(data[key + "_dst"]).cuda()
    init = torch.from_numpy(data[key + "_init"]).cuda() if case["has_init"] else None
    return src, dst, init, {"max_iterations": case["max_iterations"], "tolerance": case["tolerance"]}


@pytest.fixture(scope="module")
def results(golden):
    """One launch per case (case e: its three pairs in one), shared by the parity tests and left unchanged."""
    from ogc_amd.utils.icp_util import icp_batch
    out = {}
    for name in CASES:
        src, dst, init, kw = _inputs(golden, name)
        T, dist, iters = icp_batch(src, dst, init, **kw)
        out[name] = (T.cpu().numpy(), dist.cpu().numpy(), iters.cpu().numpy())
    return out


@pytest.mark.parametrize("name", CASES)
def test_fixture_parity(golden, results, name):
    data, meta = golden
    T, dist, iters = results[name]
    key = meta["cases"][name]["inputs"]
    both = np.concatenate([data[key + "_src"], data[key + "_dst"]], 1)
    extent = float((both.max(1) - both.min(1)).max())
    rot = float(np.abs(T[:, :3, :3] - data[name + "_T"][:, :3, :3]).max())
    trans = float(np.abs(T[:, :3, 3] - data[name + "_T"][:, :3, 3]).max())
    ddev = float(np.abs(dist - data[name + "_distances"]).max())
    print("ICP_PARITY %s iters %s want %s rot_dev %.3e trans_dev %.3e trans_dev/extent %.3e dist_dev %.3e"
          % (name, iters.tolist(), data[name + "_iters"].tolist(), rot, trans, trans / extent, ddev))
    assert np.array_equal(iters, data[name + "_iters"])
    assert dist.shape == data[name + "_distances"].shape
    assert ddev < DIST_TOL, "a last-search correspondence differs from the fixture's, or the distances do"
    assert np.array_equal(T[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (T.shape[0], 1)))
    assert rot <= ROT_TOL
    assert trans <= TRANS_TOL_REL * extent


@pytest.mark.parametrize("name", CASES)
def test_flow_from_the_fitted_transform(golden, results, name):
    from ogc_amd.utils.icp_util import rigid_flow
    data, meta = golden
    pc = data[meta["cases"][name]["inputs"] + "_src"]
    got = rigid_flow(torch.from_numpy(pc).cuda(), torch.from_numpy(results[name][0]).cuda()).cpu().numpy()
    T = data[name + "_T"]
    p = pc.astype(np.float64)
    want = (np.einsum("bij,bnj->bni", T[:, :3, :3], p) + T[:, None, :3, 3] - p).astype(np.float32)
    assert got.dtype == np.float32 and got.shape == pc.shape
    print("ICP_FLOW %s dev %.3e" % (name, float(np.abs(got - want).max())))
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-5)


@pytest.mark.parametrize("name", ("a5", "d", "e"))
def test_two_calls_give_identical_bits(golden, results, name):
    from ogc_amd.utils.icp_util import icp_batch
    src, dst, init, kw = _inputs(golden, name)
    T, dist, iters = icp_batch(src, dst, init, **kw)
    first = results[name]
    assert np.array_equal(T.cpu().numpy().view(np.uint64), first[0].view(np.uint64))
    assert np.array_equal(dist.cpu().numpy().view(np.uint64), first[1].view(np.uint64))
    assert np.array_equal(iters.cpu().numpy(), first[2])


def test_graph_capture_replays_the_eager_call(golden):
    from ogc_amd.utils.icp_util import icp_batch
    src, dst, init, kw = _inputs(golden, "e")
    eager = icp_batch(src, dst, init, **kw)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = icp_batch(src, dst, init, **kw)      # a synchronisation inside would end the capture with an error
    for t in captured:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(captured, eager):
        assert torch.equal(got.view(torch.int32 if got.dtype == torch.int32 else torch.int64),
                           want.view(torch.int32 if want.dtype == torch.int32 else torch.int64))


def test_largest_cloud_recovers_a_known_motion():
    """n = OGC_ICP_MAX_POINTS: four source points per thread and the whole LDS budget, a size no fixture case reaches.  The second
    cloud is the first one moved by 1 cm / 1 mrad — far below the point spacing, so every correspondence is the point itself —
    in float64, rounded to fp32 and shuffled.  The only error in the data is that rounding, at most half an ulp of 20 m =
    9.5e-7 per coordinate: a least-squares fit cannot miss the translation by more than a few of those (bound 5e-6) nor the
    rotation entries by more than that over the 10 m lever of the cloud (bound 1e-6)."""
    from ogc_amd.utils.icp_util import icp_batch
    header = open(os.path.join(os.path.dirname(HERE), "include", "ogc_ops.h")).read()
    n = int(header.split("#define OGC_ICP_MAX_POINTS")[1].split()[0])
    rs = np.random.RandomState(7)
    src = ((rs.rand(n, 3) - 0.5) * np.array([40.0, 4.0, 40.0])).astype(np.float32)
    c, s = np.cos(1e-3), np.sin(1e-3)
    R, t = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]), np.array([0.01, 0.0, -0.01])
    dst = (src.astype(np.float64) @ R.T + t).astype(np.float32)[rs.permutation(n)]
    T, dist, iters = icp_batch(torch.from_numpy(src).cuda()[None], torch.from_numpy(dst).cuda()[None])
    T, dist = T[0].cpu().numpy(), dist[0].cpu().numpy()
    print("ICP_MAXN iters %d rot_dev %.3e trans_dev %.3e max_dist %.3e"
          % (int(iters[0]), np.abs(T[:3, :3] - R).max(), np.abs(T[:3, 3] - t).max(), dist.max()))
    assert int(iters[0]) <= 2
    assert np.abs(T[:3, :3] - R).max() < 1e-6 and np.abs(T[:3, 3] - t).max() < 5e-6
    assert dist.shape == (n,) and dist.max() < 1e-5


def test_numpy_form_returns_the_reference_types(golden):
    from ogc_amd.utils.icp_util import icp
    data, _ = golden
    A, B = data["b_src"][0], data["b_dst"][0]
    T, dist, i = icp(A, B)
    assert isinstance(T, np.ndarray) and T.shape == (4, 4) and T.dtype == np.float64
    assert isinstance(dist, np.ndarray) and dist.shape == (200,) and dist.dtype == np.float64
    assert isinstance(i, int) and i == int(data["b_iters"][0])
    T2, dist2, i2 = icp(torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda(), init_pose=np.eye(4))
    assert np.array_equal(T2, T) and np.array_equal(dist2, dist) and i2 == i    # the identity pose changes nothing


def test_bad_arguments_are_refused_with_a_message():
    from ogc_amd import _lib
    from ogc_amd.utils.icp_util import icp_batch
    header = open(os.path.join(os.path.dirname(HERE), "include", "ogc_ops.h")).read()
    limit = int(header.split("#define OGC_ICP_MAX_POINTS")[1].split()[0])
    assert limit >= 2048
    ok = torch.zeros(1, 8, 3, device="cuda")
    for src, kw, word in ((torch.zeros(1, limit + 1, 3, device="cuda"), {}, "OGC_ICP_MAX_POINTS"),
                          (torch.zeros(1, 2, 3, device="cuda"), {}, "at least 3 points"),
                          (ok, {"max_iterations": 0}, "max_iterations")):
        with pytest.raises(_lib.OgcOpsError) as err:
            icp_batch(src, src.clone(), **kw)
        assert word in str(err.value)
    torch.cuda.synchronize()        # nothing was launched: nothing can have faulted
    T, dist, iters = icp_batch(torch.zeros(0, 8, 3, device="cuda"), torch.zeros(0, 8, 3, device="cuda"))
    assert T.shape == (0, 4, 4) and dist.shape == (0, 8) and iters.shape == (0,)

"""ogc_flow_eval (ogc_amd/csrc/flow_eval.hip) and ogc_amd.metrics.flow_eval on the device, against float64 numpy on the same fp32
inputs and against the reference's own eval_flow (tests/golden/flow_eval.npz, written by tests/golden/make_flow_eval_golden.py).

Cases: the fixture's — (B, N) = (3, 1) one point, (2, 63) below a wavefront, (2, 64) exactly one, (5, 65) one past it and, N
being odd, sample bases that are not 16-byte aligned, (1, 257), (6, 2048) two workgroups per sample — and three drawn here by
the fixture's recipe: (2, 1023) a tail workgroup, (3, 4099) tail and misaligned bases, (1, 100003) ninety-eight workgroups for
one sample.  Every case keeps every point's error and ratio at least 1e-5 (relative, float64) away from the five thresholds
(asserted here too); four fp32 roundings move a norm or a ratio by at most 4 * 2**-24 = 2.4e-7, forty times less.

Bounds:
  counts    exactly the float64 counts, per sample (a condition, not a tolerance: see the margin).
  epe_sum   within 4 * 2**-24 relative of the float64 sum of the norms, per sample: one rounding in the subtraction and at most
            three in the norm (the squares' sum twice, the root), each 2**-24 relative; the fp64 accumulation of at most 1e5
            terms adds about 1e-11.
  fixture   rates within 2**-23 relative of the reference's (it rounds an exact count once when it divides in fp32; its
            float -> double conversion is exact, and 2**-24 would do: the bound leaves a factor of two); EPE within
            |ref - truth64| + 4 * 2**-24 * truth64, the first term being the reference's own fp32 error, computed here.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EPE_RTOL = 4 * 2.0 ** -24
RATE_RTOL = 2.0 ** -23
FIXTURE_CASES = ("n1", "n63", "n64", "n65", "n257", "n2048")
DRAWN_CASES = {"n1023": (2, 1023, 0.05, 10), "n4099": (3, 4099, 0.01, 1011), "n100003": (1, 100003, 0.05, 3012)}
ALL_CASES = FIXTURE_CASES + tuple(DRAWN_CASES)


def _recipe():
    spec = importlib.util.spec_from_file_location("make_flow_eval_golden", os.path.join(HERE, "golden", "make_flow_eval_golden.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


@pytest.fixture(scope="module")
def cases():
    """name -> dict(gt, pred, thresh, epe64 (B, N), counts64 (B, 3), ref / ref_per_sample or None, epe_sum, counts, device
    tensors): inputs, float64 truth and ONE evaluation on the device per case, shared by the tests and left unchanged."""
    from ogc_amd.metrics.flow_eval import flow_eval_batch
    recipe = _recipe()
    golden = np.load(os.path.join(HERE, "golden", "flow_eval.npz"))
    out = {}
    for name in ALL_CASES:
        if name in DRAWN_CASES:
            B, N, thresh, seed = DRAWN_CASES[name]
            gt, pred = recipe.draw(B, N, thresh, seed)
            ref = per = None
        else:
            gt, pred, thresh = golden[name + "_gt"], golden[name + "_pred"], float(golden[name + "_thresh"])
            ref, per = golden[name + "_ref"], golden[name + "_ref_per_sample"]
        epe64, counts64, margin = recipe.truth64(gt, pred, thresh)
        assert margin > recipe.MARGIN, (name, margin)
        d_gt, d_pred = torch.from_numpy(gt).cuda(), torch.from_numpy(pred).cuda()
        res = flow_eval_batch(d_gt, d_pred, epe_norm_thresh=thresh)
        out[name] = dict(gt=gt, pred=pred, thresh=thresh, epe64=epe64, counts64=counts64, ref=ref, per=per, d_gt=d_gt,
                         d_pred=d_pred, epe_sum=res.epe_sum.cpu().numpy(), counts=res.counts.cpu().numpy(), n_point=res.n_point)
    return out


@pytest.mark.parametrize("name", ALL_CASES)
def test_counts_are_exact_and_the_error_sum_is_within_four_roundings(cases, name):
    c = cases[name]
    B, N = c["gt"].shape[:2]
    assert c["counts"].shape == (B, 3) and c["counts"].dtype == np.int32 and c["epe_sum"].shape == (B,)
    assert c["epe_sum"].dtype == np.float64 and c["n_point"] == N
    truth = c["epe64"].sum(axis=1)
    rel = np.abs(c["epe_sum"] - truth) / truth
    print(name, "counts", c["counts"].tolist(), "epe_sum rel err", rel.max(), "bound", EPE_RTOL)
    assert np.array_equal(c["counts"].astype(np.int64), c["counts64"])
    assert (rel <= EPE_RTOL).all()


@pytest.mark.parametrize("name", FIXTURE_CASES)
def test_eval_flow_device_against_the_reference(cases, name):
    from ogc_amd.metrics.flow_eval import eval_flow_device
    c = cases[name]
    B, N = c["gt"].shape[:2]
    total, per_sample = eval_flow_device(c["d_gt"], c["d_pred"], epe_norm_thresh=c["thresh"])
    assert isinstance(total, tuple) and len(total) == 4 and all(isinstance(v, float) for v in total)
    assert per_sample.shape == (B, 4) and per_sample.dtype == np.float64
    # the batch values are totals over all samples divided by B * N in float64; the table is per sample
    assert np.array_equal(per_sample[:, 0], c["epe_sum"] / N) and np.array_equal(per_sample[:, 1:], c["counts"] / float(N))
    assert total[0] == c["epe_sum"].sum() / (B * N) and list(total[1:]) == list(c["counts"].sum(axis=0) / float(B * N))
    for got, ref, truth_epe in ((np.array(total)[None], c["ref"][None], c["epe64"].mean()[None]),
                                (per_sample, c["per"], c["epe64"].mean(axis=1))):
        rate_err = np.abs(got[:, 1:] - ref[:, 1:])
        epe_bound = np.abs(ref[:, 0] - truth_epe) + EPE_RTOL * truth_epe
        print(name, "rates rel err", (rate_err / np.maximum(ref[:, 1:], 1e-300)).max(), "EPE err", np.abs(got[:, 0] - ref[:, 0]).max(),
              "bound", epe_bound.min(), "reference's own rel err", (np.abs(ref[:, 0] - truth_epe) / truth_epe).max())
        assert (rate_err <= RATE_RTOL * ref[:, 1:]).all()
        assert (np.abs(got[:, 0] - ref[:, 0]) <= epe_bound).all()


def test_a_perfect_prediction(cases):
    from ogc_amd.metrics.flow_eval import flow_eval_batch
    c = cases["n65"]
    res = flow_eval_batch(c["d_gt"], c["d_gt"].clone(), epe_norm_thresh=c["thresh"])
    B, N = c["gt"].shape[:2]
    assert res.epe_sum.cpu().tolist() == [0.0] * B
    assert res.counts.cpu().tolist() == [[N, N, 0]] * B


def test_a_nan_stays_in_its_own_sample(cases):
    from ogc_amd.metrics.flow_eval import flow_eval_batch
    c = cases["n4099"]          # three samples, several workgroups each
    pred = c["d_pred"].clone()
    pred[1, 2500, 1] = float("nan")
    res = flow_eval_batch(c["d_gt"], pred, epe_norm_thresh=c["thresh"])
    epe_sum, counts = res.epe_sum.cpu().numpy(), res.counts.cpu().numpy()
    assert np.isnan(epe_sum[1]) and epe_sum[[0, 2]].tobytes() == c["epe_sum"][[0, 2]].tobytes()
    assert np.array_equal(counts[[0, 2]], c["counts"][[0, 2]])
    # the NaN point satisfies no comparison: it leaves every count it was in
    e, r = c["epe64"][1, 2500], c["epe64"][1, 2500] / (np.linalg.norm(c["gt"][1, 2500].astype(np.float64)) + 1e-10)
    t = c["thresh"]
    was = np.array([e < t or r < 0.05, e < 2 * t or r < 0.1, e > 6 * t or r > 0.1], np.int64)
    assert np.array_equal(counts[1], c["counts"][1] - was)


@pytest.mark.parametrize("name", ("n65", "n2048", "n100003"))
def test_outputs_do_not_depend_on_their_previous_contents_and_calls_repeat_to_the_bit(cases, name):
    from ogc_amd import pointnet2_cuda
    c = cases[name]
    B, N = c["gt"].shape[:2]
    for fill in (float("nan"), 1e300):
        epe_sum = torch.full((B,), fill, dtype=torch.float64, device="cuda")
        counts = torch.full((B, 3), -123456789, dtype=torch.int32, device="cuda")
        pointnet2_cuda.flow_eval_wrapper(B, N, c["d_gt"], c["d_pred"], c["thresh"], 1e-10, epe_sum, counts)
        assert epe_sum.cpu().numpy().tobytes() == c["epe_sum"].tobytes()
        assert counts.cpu().numpy().tobytes() == c["counts"].tobytes()


def test_graph_capture_replays_the_eager_call(cases):
    from ogc_amd.metrics.flow_eval import flow_eval_batch
    c = cases["n4099"]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = flow_eval_batch(c["d_gt"], c["d_pred"], epe_norm_thresh=c["thresh"])   # a synchronisation inside would end the capture
    for _ in range(2):
        captured.epe_sum.fill_(-1.0)
        captured.counts.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert captured.epe_sum.cpu().numpy().tobytes() == c["epe_sum"].tobytes()
        assert captured.counts.cpu().numpy().tobytes() == c["counts"].tobytes()


def test_the_python_layer_refuses_what_the_kernel_cannot_take(cases):
    from ogc_amd.metrics.flow_eval import flow_eval_batch
    c = cases["n64"]
    gt, pred = c["d_gt"], c["d_pred"]
    with pytest.raises(TypeError):
        flow_eval_batch(gt.double(), pred)
    with pytest.raises(TypeError):
        flow_eval_batch(gt, pred.double())
    with pytest.raises(TypeError):
        flow_eval_batch(c["gt"], pred)
    with pytest.raises(ValueError):
        flow_eval_batch(gt, pred[:, :63])
    with pytest.raises(ValueError):
        flow_eval_batch(gt[0], pred[0])
    with pytest.raises(ValueError):
        flow_eval_batch(gt[:, :, :2], pred[:, :, :2])
    with pytest.raises(RuntimeError) as err:
        flow_eval_batch(gt.cpu(), pred)
    assert "no CPU path" in str(err.value)
    with pytest.raises(RuntimeError):
        flow_eval_batch(gt, pred, epe_norm_thresh=0.0)
    with pytest.raises(RuntimeError):
        flow_eval_batch(gt, pred, eps=-1.0)


def test_non_contiguous_and_misaligned_inputs_give_the_same_bits(cases):
    from ogc_amd.metrics.flow_eval import flow_eval_batch
    c = cases["n2048"]
    B, N = c["gt"].shape[:2]
    # a transposed view: made contiguous by the Python layer
    gt_t = c["d_gt"].transpose(1, 2).contiguous().transpose(1, 2)
    assert not gt_t.is_contiguous()
    res = flow_eval_batch(gt_t, c["d_pred"], epe_norm_thresh=c["thresh"])
    assert res.epe_sum.cpu().numpy().tobytes() == c["epe_sum"].tobytes() and np.array_equal(res.counts.cpu().numpy(), c["counts"])
    # a contiguous view that starts 4 bytes into its storage: the scalar path of every group, the same order of the sum
    flat = torch.empty(B * N * 3 + 1, dtype=torch.float32, device="cuda")
    flat[1:] = c["d_pred"].reshape(-1)
    shifted = flat[1:].view(B, N, 3)
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 4
    res = flow_eval_batch(c["d_gt"], shifted, epe_norm_thresh=c["thresh"])
    assert res.epe_sum.cpu().numpy().tobytes() == c["epe_sum"].tobytes() and np.array_equal(res.counts.cpu().numpy(), c["counts"])

"""ogc_seg_eval / ogc_amd.metrics.seg_eval on the MI355X against two oracles: tests/golden/seg_eval.npz (the reference's
metrics/seg_metric.py on the same inputs, tests/golden/make_seg_eval_golden.py) and the existing functions of
ogc_amd/metrics/seg_metric.py evaluated on CPU tensors here.

Integers (`hard`, `counts`, `valid`, `n_gt`, `rows`, `status`, Pred_Matched) must be EQUAL, with no exclusions; the fixture's
generator asserts what makes that fair (its margins are in the fixture's metadata).  Bounds of the rest:
  pred_iou    1 ulp (2^-52 relative) of the CPU fp64 `_prediction_table` — one correctly rounded division of exact integers on
              both sides; rtol 1e-12 against the fixture.
  confidence  (2n + 2) * 2^-53 relative of the CPU fp64 path — both sides sum at most n non-negative terms in fp64 and divide
              once; rtol 1e-6 against the fixture (the reference's float32 mean).
  miou        64 * 2^-24 = 3.9e-6 absolute of `ClusteringMetrics` and of the fixture — at most 64 float32 terms of at most 1 each,
              whichever optimal assignment a tie picks.
  ri          bit-equal to the integer formula divided in Python; within 2^-22 of the fixture's float32 value.
Each test prints its deviations as SEG_EVAL_PARITY; the largest measured are in DESIGN.md 4e."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ("n1", "n63", "batch5", "n65", "n1023", "special", "n2048")
TAGS = ("t0", "tp")
FIELDS = ("hard", "counts", "pred_iou", "confidence", "valid", "n_gt", "score", "rows", "ri", "status", "col", "miou")
MIOU_TOL = 64 * 2.0 ** -24


@pytest.fixture(scope="module")
def golden():
    data = np.load(os.path.join(HERE, "golden", "seg_eval.npz"))
    return data, json.loads(str(data["meta"]))


def _as_numpy(res):
    return {f: getattr(res, f).cpu().numpy() for f in FIELDS}


@pytest.fixture(scope="module")
def results(golden):
    """One call of seg_eval_batch per case and threshold, shared by the tests below and left unchanged."""
    from ogc_amd.metrics.seg_eval import seg_eval_batch
    data, meta = golden
    out = {}
    for name in CASES:
        segm, mask = torch.from_numpy(data[name + "_segm"]).cuda(), torch.from_numpy(data[name + "_mask"]).cuda()
        for tag in TAGS:
            res = seg_eval_batch(segm, mask, meta["cases"][name]["thresh"][tag])
            assert all(getattr(res, f).is_cuda for f in FIELDS)
            assert res.pred_iou.dtype == res.confidence.dtype == res.ri.dtype == res.miou.dtype == torch.float64
            assert res.hard.dtype == res.counts.dtype == res.rows.dtype == res.status.dtype == torch.int32
            assert res.valid.dtype == torch.bool and res.score.dtype == torch.float32
            out[name, tag] = _as_numpy(res)
    return out


@pytest.fixture(scope="module")
def cpu_oracle(golden):
    """The existing torch path on CPU tensors, once per case and threshold."""
    from ogc_amd.metrics.seg_metric import ClusteringMetrics, _prediction_table
    data, meta = golden
    out = {}
    for name in CASES:
        segm, mask = torch.from_numpy(data[name + "_segm"]).long(), torch.from_numpy(data[name + "_mask"])
        for tag in TAGS:
            thresh = meta["cases"][name]["thresh"][tag]
            pred_iou, confidence, valid, n_gt = _prediction_table(segm, mask, thresh)
            clu = ClusteringMetrics()(mask, segm, thresh)
            out[name, tag] = dict(pred_iou=pred_iou.numpy(), confidence=confidence.numpy(), valid=valid.numpy(),
                                  n_gt=n_gt.numpy(), miou=np.asarray(clu["iou"], np.float64), ri=clu["ri"])
    return out


def _integer_oracle(segm, hard, k, thresh):
    """counts, rows and the Rand index from their definitions, in Python integers."""
    B = segm.shape[0]
    counts = np.zeros((B, 64, k), np.int64)
    rows, ri = [], []
    for b in range(B):
        np.add.at(counts[b], (segm[b], hard[b]), 1)
        sizes = counts[b].sum(1)
        top = int(segm[b].max()) + 1
        kept_rows = (sizes >= thresh) if thresh > 0 else np.ones(64, bool)
        rows.append(int(kept_rows[:top].sum()))
        tab = counts[b] * kept_rows[:, None]
        n_v = int(tab.sum())
        agree = n_v * n_v - sum(int(a) ** 2 for a in tab.sum(1)) - sum(int(c) ** 2 for c in tab.sum(0)) \
            + 2 * sum(int(m) ** 2 for m in tab.reshape(-1))
        ri.append(agree / (n_v * n_v) if n_v else float("nan"))
    return counts, np.asarray(rows), np.asarray(ri, np.float64)


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("name", CASES)
def test_parity(golden, results, cpu_oracle, name, tag):
    data, meta = golden
    got, cpu = results[name, tag], cpu_oracle[name, tag]
    segm, mask = data[name + "_segm"], data[name + "_mask"]
    B, n, k = mask.shape
    thresh = meta["cases"][name]["thresh"][tag]
    pre = "%s_%s_" % (name, tag)

    want_hard = torch.from_numpy(mask).argmax(dim=2).numpy()
    counts, rows, ri = _integer_oracle(segm, want_hard, k, thresh)
    assert np.array_equal(got["status"], np.zeros(B, np.int32))
    assert np.array_equal(got["hard"], want_hard)
    assert np.array_equal(got["counts"], counts)
    assert np.array_equal(got["valid"], cpu["valid"])
    assert np.array_equal(got["valid"].sum(1), data[pre + "n_valid"])
    assert np.array_equal(got["n_gt"], cpu["n_gt"]) and np.array_equal(got["n_gt"], data[pre + "n_gt"])
    assert np.array_equal(got["rows"], rows)

    v = got["valid"]
    iou, iou_cpu, iou_ref = got["pred_iou"][v], cpu["pred_iou"][v], data[pre + "pred_iou"]
    conf, conf_cpu, conf_ref = got["confidence"][v], cpu["confidence"][v], data[pre + "confidence"]
    assert np.array_equal((iou >= 0.5).astype(float), data[pre + "pred_matched"])
    assert np.array_equal(iou >= 0.5, iou_cpu >= 0.5)
    iou_dev_cpu = float(np.max(np.abs(iou - iou_cpu) / iou_cpu.clip(1e-300), initial=0.0))
    iou_dev_ref = float(np.max(np.abs(iou - iou_ref) / np.abs(iou_ref).clip(1e-300), initial=0.0))
    conf_dev_cpu = float(np.max(np.abs(conf - conf_cpu) / conf_cpu.clip(1e-300), initial=0.0))
    conf_dev_ref = float(np.max(np.abs(conf - conf_ref) / np.abs(conf_ref).clip(1e-300), initial=0.0))
    miou_dev_cpu = float(np.abs(got["miou"] - cpu["miou"]).max())
    miou_dev_ref = float(np.abs(got["miou"] - data[pre + "miou"]).max())
    ri_dev_ref = float(np.abs(got["ri"] - data[pre + "ri"]).max())
    print("SEG_EVAL_PARITY %s %s B %d n %d k %d thresh %d valid %d pred_iou rel vs cpu %.3e vs fixture %.3e confidence rel vs cpu "
          "%.3e (bound %.3e) vs fixture %.3e miou abs vs cpu %.3e vs fixture %.3e ri abs vs fixture %.3e"
          % (name, tag, B, n, k, thresh, int(v.sum()), iou_dev_cpu, iou_dev_ref, conf_dev_cpu, (2 * n + 2) * 2.0 ** -53,
             conf_dev_ref, miou_dev_cpu, miou_dev_ref, ri_dev_ref))
    assert iou_dev_cpu <= 2.0 ** -52
    assert iou_dev_ref <= 1e-12
    assert conf_dev_cpu <= (2 * n + 2) * 2.0 ** -53
    assert conf_dev_ref <= 1e-6
    assert miou_dev_cpu <= MIOU_TOL and miou_dev_ref <= MIOU_TOL
    assert np.array_equal(got["ri"].view(np.uint64), ri.view(np.uint64))
    assert np.allclose(got["ri"], np.asarray(cpu["ri"], np.float64), rtol=0, atol=1e-15)
    assert ri_dev_ref <= 2.0 ** -22


@pytest.mark.parametrize("name", ("batch5", "special"))
def test_accumulate_returns_the_reference_tuple(golden, name):
    from ogc_amd.metrics.seg_eval import accumulate_seg_eval
    data, meta = golden
    segm, mask = torch.from_numpy(data[name + "_segm"]).cuda(), torch.from_numpy(data[name + "_mask"]).cuda()
    for tag in TAGS:
        pre = "%s_%s_" % (name, tag)
        iou, matched, conf, n_gt, miou, ri = accumulate_seg_eval(segm.long(), mask, meta["cases"][name]["thresh"][tag])
        assert isinstance(n_gt, int) and n_gt == int(data[pre + "n_gt"].sum())
        assert np.array_equal(matched, data[pre + "pred_matched"])
        np.testing.assert_allclose(iou, data[pre + "pred_iou"], rtol=1e-12, atol=0)
        np.testing.assert_allclose(conf, data[pre + "confidence"], rtol=1e-6, atol=0)
        assert np.abs(miou - data[pre + "miou"]).max() <= MIOU_TOL
        assert np.abs(ri - data[pre + "ri"]).max() <= 2.0 ** -22


def test_no_kept_object_and_nan_rows():
    """What the reference cannot run, against the existing torch path on the CPU: every GT object ignored (pred_iou 0, rows 0,
    miou NaN), and NaNs in mask rows (the first NaN is the arg-max)."""
    from ogc_amd.metrics.seg_eval import seg_eval_batch
    from ogc_amd.metrics.seg_metric import _prediction_table
    g = torch.Generator().manual_seed(5)
    segm = torch.zeros(2, 100, dtype=torch.int32)
    segm[0, 60:] = 3
    segm[1, 50:] = 9
    mask = torch.softmax(4 * torch.rand(2, 100, 5, generator=g), dim=2)
    res = seg_eval_batch(segm.cuda(), mask.cuda(), 70)
    pred_iou, _, valid, n_gt = _prediction_table(segm.long(), mask, 70)
    assert torch.equal(res.pred_iou.cpu(), torch.zeros(2, 5, dtype=torch.float64)) and not pred_iou.any()
    assert torch.equal(res.valid.cpu(), valid) and not valid.any()
    assert torch.equal(res.n_gt.cpu().long(), n_gt) and not n_gt.any()
    assert res.rows.tolist() == [0, 0] and res.status.tolist() == [0, 0]
    assert torch.isnan(res.miou).all() and torch.isnan(res.ri).all()

    nan = float("nan")
    rows = torch.tensor([[[.1, nan, .5, nan], [.3, .3, .1, .3], [nan, .9, .1, .2], [.1, .2, .2, nan]]])
    assert torch.argmax(rows, dim=2).tolist() == [[1, 0, 0, 3]]
    mask = torch.softmax(4 * torch.rand(3, 130, 4, generator=g), dim=2)
    mask[0, :4] = rows[0]
    mask[1, 64:68] = rows[0]
    mask[2, ::3, 2] = nan
    wide = torch.softmax(torch.rand(1, 70, 7, generator=g), dim=2)          # the scalar row loop
    wide[0, ::2, 5] = nan
    wide[0, 1::4, 1] = nan
    for m in (mask, wide):
        segm = torch.randint(0, 6, m.shape[:2], generator=g, dtype=torch.int32)
        res = seg_eval_batch(segm.cuda(), m.cuda())
        assert torch.equal(res.hard.cpu().long(), torch.argmax(m, dim=2))
        assert res.status.tolist() == [0] * m.shape[0]
    print("SEG_EVAL_PARITY nan rows: hard equals torch.argmax on %d + %d points" % (mask[..., 0].numel(), wide[..., 0].numel()))


@pytest.mark.parametrize("name,tag", (("n1", "t0"), ("special", "tp"), ("n2048", "tp"), ("batch5", "t0")))
def test_two_calls_give_identical_bits(golden, results, name, tag):
    from ogc_amd.metrics.seg_eval import seg_eval_batch
    data, meta = golden
    segm, mask = torch.from_numpy(data[name + "_segm"]).cuda(), torch.from_numpy(data[name + "_mask"]).cuda()
    again = _as_numpy(seg_eval_batch(segm, mask, meta["cases"][name]["thresh"][tag]))
    for f in FIELDS:
        first, second = results[name, tag][f], again[f]
        assert first.tobytes() == second.tobytes(), f


def test_graph_capture_replays_the_eager_call(golden):
    from ogc_amd.metrics.seg_eval import seg_eval_batch
    data, meta = golden
    segm, mask = torch.from_numpy(data["special_segm"]).cuda(), torch.from_numpy(data["special_mask"]).cuda()
    eager = seg_eval_batch(segm, mask, 50)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = seg_eval_batch(segm, mask, 50)       # a synchronisation inside would end the capture with an error
    for f in FIELDS:
        getattr(captured, f).zero_()
    graph.replay()
    torch.cuda.synchronize()
    for f in FIELDS:
        assert _as_numpy(captured)[f].tobytes() == _as_numpy(eager)[f].tobytes(), f


def test_labels_out_of_range_are_flagged_and_stay_apart(golden):
    """[ok, a label 64, a negative label, ok] in one batch: statuses 0, 1, 2, 0; the flagged samples are zero everywhere else; the
    neighbours equal their stand-alone results; accumulate_seg_eval falls back for the first and raises for the second."""
    from ogc_amd.metrics.seg_eval import accumulate_seg_eval, seg_eval_batch
    from ogc_amd.metrics.seg_metric import ClusteringMetrics, accumulate_eval_results
    data, _ = golden
    segm = torch.from_numpy(np.repeat(data["n65_segm"], 2, 0)).long()      # (4, 65), int64 on purpose
    mask = torch.from_numpy(np.repeat(data["n65_mask"], 2, 0)).clone()
    mask[3] = mask[3].roll(7, dims=0)
    segm[1, 11] = 64
    segm[2, 64] = -3
    segm[2, 3] = 2 ** 40                                                   # both bits may be set: the negative one decides
    res = seg_eval_batch(segm.cuda(), mask.cuda(), 8)
    status = res.status.tolist()
    assert status[0] == 0 and status[1] == 1 and status[2] & 2 and status[3] == 0
    segm[2, 3] = 0
    res = seg_eval_batch(segm.cuda(), mask.cuda(), 8)
    assert res.status.tolist() == [0, 1, 2, 0]
    got = _as_numpy(res)
    for b in (1, 2):
        for f in FIELDS:
            if f not in ("status", "col", "miou"):
                assert not got[f][b].any(), (f, b)
    for b in (0, 3):
        alone = _as_numpy(seg_eval_batch(segm[b:b + 1].cuda(), mask[b:b + 1].cuda(), 8))
        for f in FIELDS:
            assert got[f][b].tobytes() == alone[f][0].tobytes(), (f, b)

    with pytest.raises(ValueError) as err:
        accumulate_seg_eval(segm.cuda(), mask.cuda(), 8)
    assert "sample 2" in str(err.value)
    keep = [0, 1, 3]
    iou, matched, conf, n_gt, miou, ri = accumulate_seg_eval(segm[keep].cuda(), mask[keep].cuda(), 8)
    w_iou, w_matched, w_conf, w_n_gt = accumulate_eval_results(segm[keep], mask[keep], 8)
    clu = ClusteringMetrics()(mask[keep], segm[keep], 8)
    assert n_gt == w_n_gt and np.array_equal(matched, w_matched)
    np.testing.assert_allclose(iou, w_iou, rtol=2.0 ** -52, atol=0)
    np.testing.assert_allclose(conf, w_conf, rtol=132 * 2.0 ** -53, atol=0)
    assert np.abs(miou - np.asarray(clu["iou"])).max() <= MIOU_TOL
    np.testing.assert_allclose(ri, np.asarray(clu["ri"]), rtol=0, atol=1e-15)


def test_bad_arguments_are_refused_with_a_message():
    from ogc_amd import _lib
    from ogc_amd.metrics.seg_eval import seg_eval_batch
    header = open(os.path.join(os.path.dirname(HERE), "include", "ogc_ops.h")).read()
    assert int(header.split("#define OGC_SEG_EVAL_MAX_LABELS")[1].split()[0]) == 64
    segm = torch.zeros(2, 16, dtype=torch.int32, device="cuda")
    for k, word in ((0, "slots"), (65, "slots")):
        with pytest.raises(_lib.OgcOpsError) as err:
            seg_eval_batch(segm, torch.zeros(2, 16, k, device="cuda"))
        assert word in str(err.value)
    with pytest.raises(_lib.OgcOpsError) as err:
        seg_eval_batch(segm[:, :0], torch.zeros(2, 0, 4, device="cuda"))
    assert "at least one point" in str(err.value)
    ok = torch.zeros(2, 16, 4, device="cuda")
    with pytest.raises(RuntimeError) as err:
        seg_eval_batch(segm.cpu(), ok.cpu())
    assert "CUDA tensor" in str(err.value)
    with pytest.raises(RuntimeError):
        seg_eval_batch(segm.cpu(), ok)
    with pytest.raises(TypeError) as err:
        seg_eval_batch(segm, ok.double())
    assert "float32" in str(err.value)
    with pytest.raises(TypeError):
        seg_eval_batch(segm.float(), ok)
    with pytest.raises(TypeError):
        seg_eval_batch(segm.cpu().numpy(), ok)
    with pytest.raises(ValueError):
        seg_eval_batch(segm[:, :8], ok)
    with pytest.raises(ValueError):
        seg_eval_batch(segm, ok, -1)
    torch.cuda.synchronize()        # nothing was launched: nothing can have faulted
    res = seg_eval_batch(segm[:0], ok[:0])
    assert res.hard.shape == (0, 16) and res.counts.shape == (0, 64, 4) and res.pred_iou.shape == (0, 4)
    assert res.score.shape == (0, 64, 64) and res.miou.shape == (0,) and res.status.shape == (0,)

"""ogc_seg_eval_ignore / ogc_amd.metrics.seg_eval (ignore=) on the MI355X against tests/golden/seg_eval_ignore.npz (the
reference's metrics/seg_metric.py on the relabelled samples: DESIGN.md 4h, tests/golden/make_seg_eval_ignore_golden.py), against
the numpy path ogc_amd/metrics/seg_metric_ignmask.py, and against ogc_seg_eval itself where the two must coincide.

Integers (`hard`, `counts`, `ignored`, `valid`, `n_gt`, `rows`, `status`, Pred_Matched) must be EQUAL.  Bounds of the rest, those
of tests/test_seg_eval_gpu.py for the same quantities, unchanged:
  pred_iou    1 ulp (2^-52 relative) of the fp64 numpy path; rtol 1e-12 against the fixture.
  confidence  (2n + 2) * 2^-53 relative of the fp64 numpy path; rtol 1e-6 against the fixture (the reference's float32 mean).
  miou        64 * 2^-24 absolute of the numpy path and of the fixture.
  ri          bit-equal to the integer formula divided in Python; within 2^-22 of the fixture's float32 value.
Each parity test prints its deviations as SEG_EVAL_IGNORE_PARITY."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ("n1", "n63", "n65", "n1025", "n2048")
TAGS = ("t0", "tp")
FIELDS = ("hard", "counts", "pred_iou", "confidence", "valid", "n_gt", "score", "rows", "ri", "status", "col", "miou", "ignored")
MIOU_TOL = 64 * 2.0 ** -24


@pytest.fixture(scope="module")
def golden():
    data = np.load(os.path.join(HERE, "golden", "seg_eval_ignore.npz"))
    return data, json.loads(str(data["meta"]))


def _as_numpy(res):
    return {f: getattr(res, f).cpu().numpy() for f in FIELDS}


def _cuda(data, name):
    return tuple(torch.from_numpy(data[name + s]).cuda() for s in ("_segm", "_mask", "_ignore"))


@pytest.fixture(scope="module")
def results(golden):
    """One call of seg_eval_batch(ignore=) per case and threshold, shared by the tests below and left unchanged."""
    from ogc_amd.metrics.seg_eval import seg_eval_batch
    data, meta = golden
    out = {}
    for name in CASES:
        segm, mask, ignore = _cuda(data, name)
        for tag in TAGS:
            res = seg_eval_batch(segm, mask, meta["cases"][name]["thresh"][tag], ignore=ignore)
            assert all(getattr(res, f).is_cuda for f in FIELDS)
            assert res.ignored.dtype == res.hard.dtype == res.counts.dtype == torch.int32 and res.valid.dtype == torch.bool
            out[name, tag] = _as_numpy(res)
    return out


def _integer_oracle(segm, hard, ignore, k, thresh):
    """counts, ignored, rows and the Rand index from their definitions, in Python integers."""
    B = segm.shape[0]
    counts, ignored = np.zeros((B, 64, k), np.int64), np.zeros((B, k), np.int64)
    rows, ri = [], []
    for b in range(B):
        seen = ignore[b] == 0
        np.add.at(counts[b], (segm[b][seen], hard[b][seen]), 1)
        np.add.at(ignored[b], hard[b][~seen], 1)
        sizes = counts[b].sum(1)
        top = int(np.nonzero(sizes)[0].max()) + 1 if sizes.any() else 0
        kept_rows = (sizes >= thresh) if thresh > 0 else np.ones(64, bool)
        rows.append(int(kept_rows[:top].sum()))
        tab = counts[b] * kept_rows[:, None]
        n_v = int(tab.sum())
        agree = n_v * n_v - sum(int(a) ** 2 for a in tab.sum(1)) - sum(int(c) ** 2 for c in tab.sum(0)) \
            + 2 * sum(int(m) ** 2 for m in tab.reshape(-1))
        ri.append(agree / (n_v * n_v) if n_v else float("nan"))
    return counts, ignored, np.asarray(rows), np.asarray(ri, np.float64)


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("name", CASES)
def test_parity(golden, results, name, tag):
    from ogc_amd.metrics import seg_metric_ignmask as cpu
    data, meta = golden
    got = results[name, tag]
    segm, mask, ignore = data[name + "_segm"], data[name + "_mask"], data[name + "_ignore"]
    B, n, k = mask.shape
    thresh = meta["cases"][name]["thresh"][tag]
    pre = "%s_%s_" % (name, tag)

    want_hard = torch.from_numpy(mask).argmax(dim=2).numpy()
    counts, ignored, rows, ri = _integer_oracle(segm, want_hard, ignore, k, thresh)
    assert np.array_equal(got["status"], np.zeros(B, np.int32))
    assert np.array_equal(got["hard"], want_hard)
    assert np.array_equal(got["counts"], counts)
    assert np.array_equal(got["ignored"], ignored)
    assert np.array_equal(got["valid"].sum(1), data[pre + "n_valid"])
    assert np.array_equal(got["n_gt"], data[pre + "n_gt"])
    assert np.array_equal(got["rows"], rows)
    assert np.array_equal(got["ri"].view(np.uint64), ri.view(np.uint64))

    v = got["valid"]
    per_sample = [cpu.eval_segm(segm[b], mask[b], ignore[b], thresh) for b in range(B)]
    iou_cpu, conf_cpu = np.concatenate([p[0] for p in per_sample]), np.concatenate([p[2] for p in per_sample])
    assert [len(p[0]) for p in per_sample] == v.sum(1).tolist()
    clu = cpu.ClusteringMetrics()(mask, segm, ignore, thresh)
    iou, iou_ref = got["pred_iou"][v], data[pre + "pred_iou"]
    conf, conf_ref = got["confidence"][v], data[pre + "confidence"]
    assert np.array_equal((iou >= 0.5).astype(float), data[pre + "pred_matched"])
    iou_dev_cpu = float(np.max(np.abs(iou - iou_cpu) / iou_cpu.clip(1e-300), initial=0.0))
    iou_dev_ref = float(np.max(np.abs(iou - iou_ref) / np.abs(iou_ref).clip(1e-300), initial=0.0))
    conf_dev_cpu = float(np.max(np.abs(conf - conf_cpu) / conf_cpu.clip(1e-300), initial=0.0))
    conf_dev_ref = float(np.max(np.abs(conf - conf_ref) / np.abs(conf_ref).clip(1e-300), initial=0.0))
    miou_dev_cpu = float(np.abs(got["miou"] - np.asarray(clu["iou"])).max())
    miou_dev_ref = float(np.abs(got["miou"] - data[pre + "miou"]).max())
    ri_dev_ref = float(np.abs(got["ri"] - data[pre + "ri"]).max())
    print("SEG_EVAL_IGNORE_PARITY %s %s B %d n %d k %d thresh %d ignored %d valid %d pred_iou rel vs cpu %.3e vs fixture %.3e "
          "confidence rel vs cpu %.3e (bound %.3e) vs fixture %.3e miou abs vs cpu %.3e vs fixture %.3e ri abs vs fixture %.3e"
          % (name, tag, B, n, k, thresh, int(ignored.sum()), int(v.sum()), iou_dev_cpu, iou_dev_ref, conf_dev_cpu,
             (2 * n + 2) * 2.0 ** -53, conf_dev_ref, miou_dev_cpu, miou_dev_ref, ri_dev_ref))
    assert iou_dev_cpu <= 2.0 ** -52
    assert iou_dev_ref <= 1e-12
    assert conf_dev_cpu <= (2 * n + 2) * 2.0 ** -53
    assert conf_dev_ref <= 1e-6
    assert miou_dev_cpu <= MIOU_TOL and miou_dev_ref <= MIOU_TOL
    assert np.allclose(got["ri"], np.asarray(clu["ri"], np.float64), rtol=0, atol=1e-15)
    assert ri_dev_ref <= 2.0 ** -22


@pytest.mark.parametrize("name", CASES)
def test_accumulate_returns_the_reference_tuple(golden, name):
    """accumulate_seg_eval(ignore=) with int64 labels and a bool mask against the fixture."""
    from ogc_amd.metrics.seg_eval import accumulate_seg_eval
    data, meta = golden
    segm, mask, ignore = _cuda(data, name)
    for tag in TAGS:
        pre = "%s_%s_" % (name, tag)
        iou, matched, conf, n_gt, miou, ri = accumulate_seg_eval(segm.long(), mask, meta["cases"][name]["thresh"][tag],
                                                                 ignore=ignore.bool())
        assert isinstance(n_gt, int) and n_gt == int(data[pre + "n_gt"].sum())
        assert np.array_equal(matched, data[pre + "pred_matched"])
        np.testing.assert_allclose(iou, data[pre + "pred_iou"], rtol=1e-12, atol=0)
        np.testing.assert_allclose(conf, data[pre + "confidence"], rtol=1e-6, atol=0)
        assert np.abs(miou - data[pre + "miou"]).max() <= MIOU_TOL
        assert np.abs(ri - data[pre + "ri"]).max() <= 2.0 ** -22


def _raw(segm, mask, ignore, thresh):
    """The entry point itself through its wrapper: every output buffer pre-filled with a pattern it must overwrite."""
    from ogc_amd import pointnet2_cuda as nat
    B, n, k = mask.shape
    dev = mask.device
    i32 = lambda *s: torch.full(s, -7, dtype=torch.int32, device=dev)  # noqa: E731
    f64 = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device=dev)  # noqa: E731
    out = dict(hard=i32(B, n), counts=i32(B, 64, k), ignored=i32(B, k), pred_iou=f64(B, k), confidence=f64(B, k), valid=i32(B, k),
               n_gt=i32(B), score=torch.full((B, 64, 64), -7.0, device=dev), rows=i32(B), ri=f64(B), status=i32(B))
    nat.seg_eval_ignore_wrapper(B, n, k, segm, mask, ignore, thresh, out["hard"], out["counts"], out["ignored"], out["pred_iou"],
                                out["confidence"], out["valid"], out["n_gt"], out["score"], out["rows"], out["ri"], out["status"])
    return {f: t.cpu().numpy() for f, t in out.items()}


@pytest.mark.parametrize("name,tag", (("n65", "t0"), ("n1025", "tp"), ("n2048", "tp")))
def test_raw_entry_point(golden, results, name, tag):
    """Any non-zero word ignores a point; the raw outputs are those seg_eval_batch returned."""
    data, meta = golden
    segm, mask, ignore = _cuda(data, name)
    ignore = ignore * torch.where(torch.arange(ignore.shape[1], device="cuda") % 2 == 0, -1, 1 << 20).to(torch.int32)
    got = _raw(segm, mask, ignore, meta["cases"][name]["thresh"][tag])
    for f, value in got.items():
        want = results[name, tag][f]
        assert value.tobytes() == (want.astype(np.int32) if f == "valid" else want).tobytes(), f


@pytest.mark.parametrize("name", ("n63", "n65", "n1025", "n2048"))
def test_all_zero_mask_has_the_bits_of_seg_eval(golden, name):
    """(a) nothing ignored: every output is bit-identical to ogc_seg_eval's, and `ignored` is zero."""
    from ogc_amd.metrics.seg_eval import seg_eval_batch
    data, meta = golden
    segm, mask, ignore = _cuda(data, name)
    segm = torch.from_numpy(_real_labels(data, name)).cuda()
    for tag in TAGS:
        thresh = meta["cases"][name]["thresh"][tag]
        plain = _as_numpy(seg_eval_batch(segm, mask, thresh))
        zero = _as_numpy(seg_eval_batch(segm, mask, thresh, ignore=torch.zeros_like(ignore)))
        for f in FIELDS:
            assert plain[f].tobytes() == zero[f].tobytes(), (f, tag)
        assert not zero["ignored"].any()


def _real_labels(data, name):
    """The fixture stores 0 under ignored points; for the identities every point needs a label of its own choosing."""
    segm, ignore = data[name + "_segm"].copy(), data[name + "_ignore"]
    rng = np.random.default_rng(11)
    labels = np.unique(segm)
    fill = labels[rng.integers(0, len(labels), segm.shape)]
    return np.where(ignore != 0, fill, segm).astype(np.int32)


@pytest.mark.parametrize("name,thresh", (("n63", 12), ("n65", 8), ("n1025", 50), ("n2048", 120), ("n2048", 1)))
def test_mask_of_the_small_objects_is_the_threshold(name, thresh):
    """(b) ignore = the points of objects smaller than T, thresh = T: every output has the bits of ogc_seg_eval(thresh = T) except
    `counts`, whose dropped rows are now empty, and `ignored`, which holds what left them.  The inputs are those of the
    unmasked fixture, whose objects straddle its thresholds."""
    from ogc_amd.metrics.seg_eval import seg_eval_batch
    data = np.load(os.path.join(HERE, "golden", "seg_eval.npz"))
    name = {"n1025": "special"}.get(name, name)
    segm_np, mask = data[name + "_segm"], torch.from_numpy(data[name + "_mask"]).cuda()
    B, n, k = mask.shape
    sizes = np.stack([np.bincount(segm_np[b], minlength=64) for b in range(B)])
    small = sizes < thresh
    ignore_np = np.take_along_axis(small, segm_np.astype(np.int64), 1)
    assert thresh == 1 or ignore_np.any()
    segm, ignore = torch.from_numpy(segm_np).cuda(), torch.from_numpy(ignore_np).cuda()
    plain = _as_numpy(seg_eval_batch(segm, mask, thresh))
    masked = _as_numpy(seg_eval_batch(segm, mask, thresh, ignore=ignore))
    for f in FIELDS:
        if f not in ("counts", "ignored"):
            assert plain[f].tobytes() == masked[f].tobytes(), f
    assert np.array_equal(masked["counts"], plain["counts"] * ~small[:, :, None])
    assert np.array_equal(masked["ignored"], (plain["counts"] * small[:, :, None]).sum(1))


@pytest.mark.parametrize("name,tag", (("n65", "t0"), ("n1025", "tp"), ("n2048", "t0")))
def test_two_calls_give_identical_bits(golden, results, name, tag):
    """(c)"""
    from ogc_amd.metrics.seg_eval import seg_eval_batch
    data, meta = golden
    segm, mask, ignore = _cuda(data, name)
    again = _as_numpy(seg_eval_batch(segm, mask, meta["cases"][name]["thresh"][tag], ignore=ignore))
    for f in FIELDS:
        assert results[name, tag][f].tobytes() == again[f].tobytes(), f


def test_all_points_ignored():
    """n_gt = rows = 0, no valid prediction, ri and miou NaN, `ignored` the slot sizes; the neighbour in the batch is untouched."""
    from ogc_amd.metrics.seg_eval import accumulate_seg_eval, seg_eval_batch
    g = torch.Generator().manual_seed(7)
    mask = torch.softmax(4 * torch.rand(2, 1100, 6, generator=g), dim=2).cuda()
    segm = torch.randint(0, 5, (2, 1100), generator=g, dtype=torch.int32).cuda()
    ignore = torch.zeros(2, 1100, dtype=torch.int32, device="cuda")
    ignore[0] = 1
    res = seg_eval_batch(segm, mask, 0, ignore=ignore)
    hard = mask.argmax(dim=2)
    assert torch.equal(res.hard.long(), hard)
    assert res.n_gt.tolist()[0] == 0 and res.rows.tolist()[0] == 0 and res.status.tolist() == [0, 0]
    assert not res.valid[0].any() and not res.counts[0].any() and not res.pred_iou[0].any() and not res.score[0].any()
    assert torch.equal(res.ignored[0].long(), torch.bincount(hard[0], minlength=6))
    assert torch.isnan(res.ri[0]) and torch.isnan(res.miou[0])
    alone = seg_eval_batch(segm[1:], mask[1:], 0)
    for f in FIELDS:
        assert getattr(res, f)[1].cpu().numpy().tobytes() == getattr(alone, f)[0].cpu().numpy().tobytes(), f
    iou, matched, conf, n_gt, miou, ri = accumulate_seg_eval(segm[:1], mask[:1], ignore=ignore[:1])
    assert len(iou) == len(matched) == len(conf) == 0 and n_gt == 0 and np.isnan(miou[0]) and np.isnan(ri[0])


def test_labels_out_of_range(golden):
    """-5 and 99 under ignored points only: status 0 and the results of the clean labels.  The same labels on a point that
    counts: the status bit, every other output zero; accumulate_seg_eval falls back to the numpy path for the label that is too
    large and raises for the negative one."""
    from ogc_amd.metrics import seg_metric_ignmask as cpu
    from ogc_amd.metrics.seg_eval import accumulate_seg_eval, seg_eval_batch
    data, _ = golden
    segm, mask, ignore = _cuda(data, "n1025")
    clean = _as_numpy(seg_eval_batch(segm, mask, 50, ignore=ignore))
    dirty_segm = segm.clone()
    at = ignore != 0
    dirty_segm[at] = torch.where(torch.arange(int(at.sum()), device="cuda") % 2 == 0, -5, 99).to(torch.int32)
    dirty = _as_numpy(seg_eval_batch(dirty_segm, mask, 50, ignore=ignore))
    assert dirty["status"].tolist() == [0, 0]
    for f in FIELDS:
        assert clean[f].tobytes() == dirty[f].tobytes(), f

    counted = [int(i) for i in torch.nonzero(ignore[0] == 0)[:2, 0]]
    for label, bit in ((99, 1), (-5, 2)):
        bad = dirty_segm.clone()
        bad[0, counted[0]] = label
        res = seg_eval_batch(bad, mask, 50, ignore=ignore)
        got = _as_numpy(res)
        assert got["status"].tolist() == [bit, 0]
        for f in FIELDS:
            if f not in ("status", "col", "miou"):
                assert not got[f][0].any(), (f, label)
                assert got[f][1].tobytes() == clean[f][1].tobytes(), (f, label)
        if bit == 2:
            with pytest.raises(ValueError) as err:
                accumulate_seg_eval(bad, mask, 50, ignore=ignore)
            assert "sample 0" in str(err.value)
        else:
            iou, matched, conf, n_gt, miou, ri = accumulate_seg_eval(bad, mask, 50, ignore=ignore)
            w_iou, w_matched, w_conf, w_n_gt = cpu.accumulate_eval_results(bad, mask, ignore, 50)
            clu = cpu.ClusteringMetrics()(mask, bad, ignore, 50)
            assert n_gt == w_n_gt and np.array_equal(matched, w_matched)
            np.testing.assert_allclose(iou, w_iou, rtol=2.0 ** -52, atol=0)
            np.testing.assert_allclose(conf, w_conf, rtol=(2 * 1025 + 2) * 2.0 ** -53, atol=0)
            assert np.abs(miou - np.asarray(clu["iou"])).max() <= MIOU_TOL
            np.testing.assert_allclose(ri, np.asarray(clu["ri"]), rtol=0, atol=1e-15)


def test_bad_arguments_are_refused_with_a_message():
    from ogc_amd import _lib
    from ogc_amd.metrics.seg_eval import seg_eval_batch
    segm = torch.zeros(2, 16, dtype=torch.int32, device="cuda")
    ignore = torch.zeros(2, 16, dtype=torch.int32, device="cuda")
    for k in (0, 65):
        with pytest.raises(_lib.OgcOpsError) as err:
            seg_eval_batch(segm, torch.zeros(2, 16, k, device="cuda"), ignore=ignore)
        assert "ogc_seg_eval_ignore" in str(err.value) and "slots" in str(err.value)
    ok = torch.zeros(2, 16, 4, device="cuda")
    good = seg_eval_batch(segm, ok, ignore=ignore)
    ptr = lambda t: t.data_ptr()  # noqa: E731
    valid = torch.zeros(2, 4, dtype=torch.int32, device="cuda")
    args = [2, 16, 4, ptr(segm), ptr(ok), None, 0, ptr(good.hard), ptr(good.counts), ptr(good.ignored), ptr(good.pred_iou),
            ptr(good.confidence), ptr(valid), ptr(good.n_gt), ptr(good.score),
            ptr(good.rows), ptr(good.ri), ptr(good.status), None]
    with pytest.raises(_lib.OgcOpsError) as err:
        _lib.call("ogc_seg_eval_ignore", *args)                    # a null `ignore`
    assert "null pointer" in str(err.value)
    with pytest.raises(ValueError):
        seg_eval_batch(segm, ok, ignore=ignore[:, :8])
    with pytest.raises(ValueError):
        seg_eval_batch(segm, ok, ignore=ignore.reshape(-1))
    with pytest.raises(RuntimeError):
        seg_eval_batch(segm, ok, ignore=ignore.cpu())
    with pytest.raises(TypeError):
        seg_eval_batch(segm, ok, ignore=ignore.float())
    with pytest.raises(TypeError):
        seg_eval_batch(segm, ok, ignore=ignore.cpu().numpy())
    torch.cuda.synchronize()        # nothing was launched by the refused calls: nothing can have faulted
    res = seg_eval_batch(segm[:0], ok[:0], ignore=ignore[:0])
    assert res.hard.shape == (0, 16) and res.ignored.shape == (0, 4) and res.miou.shape == (0,)

"""ogc_amd/metrics/seg_metric_ignmask.py (the numpy path of the ignore-mask metric) against
tests/golden/seg_eval_ignore.npz: the reference's metrics/seg_metric.py on the relabelled samples (every ignored point an object
of one point, threshold max(thresh, 2); tests/golden/make_seg_eval_ignore_golden.py).  CPU only.

Bounds, those tests/test_seg_eval_gpu.py uses for the same quantities against its fixture: counts and Pred_Matched equal,
pred_iou rtol 1e-12, confidence rtol 1e-6 (the reference's float32 mean), miou 64 * 2^-24 absolute, ri 2^-22 absolute."""
import json
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ("n1", "n63", "n65", "n1025", "n2048")
TAGS = ("t0", "tp")
MIOU_TOL = 64 * 2.0 ** -24


@pytest.fixture(scope="module")
def golden():
    data = np.load(os.path.join(HERE, "golden", "seg_eval_ignore.npz"))
    return data, json.loads(str(data["meta"]))


def test_fixture_holds_the_cases_of_the_definition(golden):
    data, meta = golden
    assert tuple(meta["cases"]) == CASES
    shapes = {name: (c["B"], c["n"], c["k"]) for name, c in meta["cases"].items()}
    assert shapes["n1"] == (1, 1, 1) and shapes["n63"][1:] == (63, 2) and shapes["n65"][1:] == (65, 64)
    assert shapes["n1025"][1:] == (1025, 15) and shapes["n2048"] == (3, 2048, 22)
    assert not data["n1_ignore"].any() and (data["n65_segm"] == 63).any()
    ign = data["n2048_ignore"]
    assert ign[0].any() and not ign[1].any() and ign[2].any()
    m = meta["smallest_margins"]
    assert m["pred_iou_from_half"] >= 1e-9 and m["confidence_gap"] >= 1e-5 and m["ignore_ratio_from_half"] >= 1e-9
    assert m["exact_half_ratios"] >= 1


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("name", CASES)
def test_numpy_path_against_the_relabelled_reference(golden, name, tag):
    from ogc_amd.metrics.seg_metric_ignmask import ClusteringMetrics, accumulate_eval_results, eval_segm
    data, meta = golden
    segm, mask, ignore = data[name + "_segm"], data[name + "_mask"], data[name + "_ignore"]
    thresh = meta["cases"][name]["thresh"][tag]
    pre = "%s_%s_" % (name, tag)
    iou, matched, conf, n_gt = accumulate_eval_results(torch.from_numpy(segm), torch.from_numpy(mask), torch.from_numpy(ignore),
                                                       ignore_npoint_thresh=thresh)
    per_sample = [eval_segm(segm[b], mask[b], ignore[b], thresh) for b in range(segm.shape[0])]
    assert [len(p[0]) for p in per_sample] == data[pre + "n_valid"].tolist()
    assert [p[3] for p in per_sample] == data[pre + "n_gt"].tolist()
    assert isinstance(n_gt, int) and n_gt == int(data[pre + "n_gt"].sum())
    assert np.array_equal(matched, data[pre + "pred_matched"])
    np.testing.assert_allclose(iou, data[pre + "pred_iou"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(conf, data[pre + "confidence"], rtol=1e-6, atol=0)
    clu = ClusteringMetrics()(torch.from_numpy(mask), torch.from_numpy(segm), torch.from_numpy(ignore), ignore_npoint_thresh=thresh)
    assert np.abs(np.asarray(clu["iou"]) - data[pre + "miou"]).max() <= MIOU_TOL
    assert np.abs(np.asarray(clu["ri"]) - data[pre + "ri"]).max() <= 2.0 ** -22


def test_labels_of_ignored_points_are_not_read(golden):
    """Anything under an ignored point, out-of-range values included, changes nothing; a negative label on a point that counts
    is refused."""
    from ogc_amd.metrics.seg_metric_ignmask import ClusteringMetrics, accumulate_eval_results
    data, _ = golden
    segm, mask, ignore = data["n1025_segm"].copy(), data["n1025_mask"], data["n1025_ignore"]
    want = accumulate_eval_results(segm, mask, ignore)
    want_clu = ClusteringMetrics()(mask, segm, ignore)
    idx = np.nonzero(ignore)
    segm[idx] = np.resize(np.array([-5, 99, 3, 2 ** 30], np.int32), len(idx[0]))
    got = accumulate_eval_results(segm, mask, ignore)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    assert ClusteringMetrics()(mask, segm, ignore) == want_clu
    segm[0, np.nonzero(ignore[0] == 0)[0][0]] = -1
    with pytest.raises(ValueError):
        accumulate_eval_results(segm, mask, ignore)


def test_all_points_ignored():
    from ogc_amd.metrics.seg_metric_ignmask import ClusteringMetrics, accumulate_eval_results
    g = torch.Generator().manual_seed(3)
    mask = torch.softmax(4 * torch.rand(1, 50, 4, generator=g), dim=2)
    segm, ignore = torch.zeros(1, 50, dtype=torch.int64), torch.ones(1, 50, dtype=torch.bool)
    iou, matched, conf, n_gt = accumulate_eval_results(segm, mask, ignore)
    assert len(iou) == len(matched) == len(conf) == 0 and n_gt == 0
    clu = ClusteringMetrics()(mask, segm, ignore)
    assert np.isnan(clu["iou"][0]) and np.isnan(clu["ri"][0])


def test_ap_pq_f1_on_the_concatenated_results(golden):
    """calculate_AP / calculate_PQ_F1 of the module on all cases together, from the module's results and from the fixture's."""
    from ogc_amd.metrics import seg_metric, seg_metric_ignmask as m
    assert m.calculate_AP is seg_metric.calculate_AP and m.calculate_PQ_F1 is seg_metric.calculate_PQ_F1
    data, meta = golden
    for tag in TAGS:
        got, ref, n_gt, n_gt_ref = [[], [], []], [[], [], []], 0, 0
        for name in CASES:
            pre = "%s_%s_" % (name, tag)
            out = m.accumulate_eval_results(data[name + "_segm"], data[name + "_mask"], data[name + "_ignore"],
                                            ignore_npoint_thresh=meta["cases"][name]["thresh"][tag])
            for i in range(3):
                got[i].append(out[i])
                ref[i].append(data[pre + ("pred_iou", "pred_matched", "confidence")[i]])
            n_gt += out[3]
            n_gt_ref += int(data[pre + "n_gt"].sum())
        got, ref = [np.concatenate(x) for x in got], [np.concatenate(x) for x in ref]
        assert n_gt == n_gt_ref
        # the fixture's confidences are 1e-5 apart over all cases together as well, ten times the bound on a confidence: the
        # order AP sorts by cannot differ
        assert np.diff(np.sort(ref[2])).min() >= 1e-5
        ap = m.calculate_AP(got[1], got[2], n_gt)
        assert ap == m.calculate_AP(ref[1], ref[2], n_gt_ref)
        assert 0.0 < ap <= 1.0
        pq, f1, pre_, rec = m.calculate_PQ_F1(got[0], got[1], n_gt)
        pq_r, f1_r, pre_r, rec_r = m.calculate_PQ_F1(ref[0], ref[1], n_gt_ref)
        assert (f1, pre_, rec) == (f1_r, pre_r, rec_r) and abs(pq - pq_r) <= 1e-12
        tp = got[1].sum()
        assert pre_ == tp / len(got[1]) and rec == tp / n_gt

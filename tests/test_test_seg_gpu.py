"""ogc_amd.test_seg on the MI355X: `evaluate` against the existing metric functions of ogc_amd/metrics/seg_metric.py on the same
masks, and `main` end to end on synthetic roots (utils/synthetic.py::write_labelled_root, N = 1024, 4 scenes).

Bounds: AP / PQ / F1 / Pre / Rec rtol 1e-12 (functions of pred_iou, 1 ulp from the tensor path, of Pred_Matched and of the order
of the confidences); the per-scan mIoU means and standard deviations 64 * 2^-24 absolute (the per-sample bound of
tests/test_seg_eval_gpu.py; mean and standard deviation over a scan move by at most the largest per-sample deviation); the
per-scan RI ones 1e-15 (per sample the same integers divided once)."""
import os
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_POINTS, N_OBJECTS, N_SCENES, N_SLOT = 1024, 6, 4, 10
MIOU_TOL = 64 * 2.0 ** -24


def _loader(tmp_path, layout, batch_size):
    from ogc_amd import datasets
    from ogc_amd.utils.synthetic import write_labelled_root
    mapping, _ = write_labelled_root(str(tmp_path), layout, N_SCENES, N_POINTS, N_OBJECTS, seed=40)
    if layout == "kittisf":
        ds = datasets.KITTISceneFlowDataset(str(tmp_path), mapping, downsampled=True, view_sels=[[0, 1], [1, 0]], decentralize=True)
    else:
        ds = datasets.KITTIDetectionDataset(str(tmp_path), mapping, decentralize=True)
    return ds, torch.utils.data.DataLoader(ds, batch_size=batch_size, shuffle=False, num_workers=0)


def _fixed_masks(loader):
    """One (B, N, K) soft-max mask per batch: random logits with a bonus at slot (label mod K), so that some predictions match."""
    g = torch.Generator().manual_seed(8)
    masks = []
    for _, segms, _, _ in loader:
        segm = segms[:, 0].long()
        logits = 3 * torch.rand(segm.shape[0], segm.shape[1], N_SLOT, generator=g)
        logits.scatter_add_(2, (segm % N_SLOT).unsqueeze(2), torch.full(segm.shape + (1,), 2.0))
        masks.append(torch.softmax(logits, dim=2))
    return masks


def _existing_path(loader, masks, n_frame, thresh):
    """test_seg.py's loop on the existing functions, on CPU tensors."""
    from ogc_amd.metrics.seg_metric import ClusteringMetrics, accumulate_eval_results, calculate_AP, calculate_PQ_F1
    from ogc_amd.utils.pytorch_util import AverageMeter
    meter, ious, matched, confs, n_gt = AverageMeter(), [], [], [], 0
    for (_, segms, _, _), mask in zip(loader, masks):
        segm = segms[:, 0].long()
        a, b, c, d = accumulate_eval_results(segm, mask, thresh)
        ious.append(a), matched.append(b), confs.append(c)
        n_gt += d
        for sid in range(segm.shape[0] // n_frame):
            scan = slice(n_frame * sid, n_frame * (sid + 1))
            per = ClusteringMetrics()(mask[scan], segm[scan], thresh)
            meter.append_loss({"per_scan_iou_avg": np.mean(per["iou"]), "per_scan_iou_std": np.std(per["iou"]),
                               "per_scan_ri_avg": np.mean(per["ri"]), "per_scan_ri_std": np.std(per["ri"])})
    ious, matched, confs = np.concatenate(ious), np.concatenate(matched), np.concatenate(confs)
    pq, f1, pre, rec = calculate_PQ_F1(ious, matched, n_gt)
    out = {"AP": calculate_AP(matched, confs, n_gt), "PQ": pq, "F1": f1, "Pre": pre, "Rec": rec}
    out.update(meter.get_mean_loss_dict())
    return out


@pytest.mark.parametrize("layout,n_frame,batch_size", (("kittisf", 2, 4), ("kittidet", 1, 2)))
def test_evaluate_equals_the_existing_functions(tmp_path, layout, n_frame, batch_size):
    from ogc_amd.test_seg import OUTDOOR_IGNORE_NPOINT_THRESH, evaluate
    _, loader = _loader(tmp_path, layout, batch_size)
    masks = _fixed_masks(loader)
    served = iter(masks)
    got = evaluate(lambda pc, feats: next(served).cuda(), loader, n_frame, OUTDOOR_IGNORE_NPOINT_THRESH)
    want = _existing_path(loader, masks, n_frame, OUTDOOR_IGNORE_NPOINT_THRESH)
    assert got["n_batches"] == len(masks) == N_SCENES * n_frame // batch_size and got["n_skipped"] == 0
    print("TEST_SEG_PARITY %s " % layout + " ".join("%s %.6f (%.2e)" % (k, got[k], abs(got[k] - want[k])) for k in want))
    for key in ("AP", "PQ", "F1", "Pre", "Rec"):
        assert 0 < want[key] <= 1
        np.testing.assert_allclose(got[key], want[key], rtol=1e-12, atol=0)
    for key in ("per_scan_iou_avg", "per_scan_iou_std"):
        assert abs(got[key] - want[key]) <= MIOU_TOL
    for key in ("per_scan_ri_avg", "per_scan_ri_std"):
        assert abs(got[key] - want[key]) <= 1e-15


def test_one_hot_ground_truth_scores_one(tmp_path):
    from ogc_amd.test_seg import OUTDOOR_IGNORE_NPOINT_THRESH, evaluate
    _, loader = _loader(tmp_path, "kittisf", 4)
    labels = iter([segms[:, 0].long() for _, segms, _, _ in loader])
    got = evaluate(lambda pc, feats: torch.nn.functional.one_hot(next(labels), N_SLOT).float().cuda(), loader, 2,
                   OUTDOOR_IGNORE_NPOINT_THRESH)
    for key in ("AP", "PQ", "F1", "Pre", "Rec", "per_scan_iou_avg", "per_scan_ri_avg"):
        assert got[key] == pytest.approx(1.0, abs=1e-12), key
    assert got["per_scan_iou_std"] == 0.0 and got["per_scan_ri_std"] == 0.0


def test_curate_by_object_passes_over_small_scenes():
    """Batches of one scene (two frames): the scenes whose first sample has at most T objects are passed over, as
    test_seg.py:189-191 does; what is left gives the metrics of those scenes alone."""
    from ogc_amd.test_seg import evaluate
    from ogc_amd.utils.synthetic import make_scene_batch
    batches = []
    for seed, objects in ((1, 3), (2, 6), (3, 2), (4, 5)):
        pcs, segms, flows, valids = make_scene_batch(1, 512, objects, seed=seed, outdoor=False)
        assert torch.unique(segms[0, 0]).shape[0] == objects
        # the two samples of a scene: the frame pair in both orders, as view_sels [[0, 1], [1, 0]] gives them
        batches.append(tuple(torch.stack([t[0], t[0].flip(0)]) for t in (pcs, segms.int(), flows, valids.float())))
    g = torch.Generator().manual_seed(2)
    masks = [torch.softmax(4 * torch.rand(2, 512, 8, generator=g), dim=2) for _ in batches]

    def run(selected, curate):
        served = iter([masks[i] for i in selected])
        saved = []
        out = evaluate(lambda pc, feats: next(served).cuda(), [batches[i] for i in selected], 2, 0, curate_by_object=curate,
                       saver=lambda hard, i: saved.append((i, hard.cpu())))
        return out, saved
    everything, saved_all = run([0, 1, 2, 3], 0)
    assert everything["n_batches"] == 4 and everything["n_skipped"] == 0 and [i for i, _ in saved_all] == [0, 1, 2, 3]
    served = iter([masks[1], masks[3]])
    saved = []
    curated = evaluate(lambda pc, feats: next(served).cuda(), batches, 2, 0, curate_by_object=3,
                       saver=lambda hard, i: saved.append((i, hard.cpu())))
    alone, _ = run([1, 3], 0)
    assert curated["n_batches"] == 2 and curated["n_skipped"] == 2
    assert [i for i, _ in saved] == [1, 3]          # the loader's batch index, as the reference passes `offset=i`
    assert torch.equal(saved[0][1].long(), masks[1].argmax(2)) and torch.equal(saved[1][1].long(), masks[3].argmax(2))
    for key in alone:
        if key not in ("n_batches", "n_skipped"):
            assert curated[key] == alone[key], key
    with pytest.raises(ValueError):
        evaluate(lambda pc, feats: None, batches, 2, 0, curate_by_object=6)


def test_main_saves_the_arg_max_of_the_network():
    """`main` on 4 synthetic KITTI-Det scenes with the real network at random weights: the saved segm.npy equal the arg-max of a
    second forward wherever the two largest mask values differ by more than 1e-4 (at most 5 % of the points may be left out)."""
    import yaml
    from ogc_amd import datasets
    from ogc_amd.test_seg import build_segnet, main
    config = os.path.join(ROOT, "config", "kittidet_unsup_synthetic.yaml")
    metrics = main([config, "--split", "val", "--synthetic", "4", "--save", "--test_batch_size", "4", "--num_workers", "0"])
    save_dir = metrics["save_dir"]
    data_root = os.path.dirname(os.path.dirname(save_dir))
    try:
        assert os.path.basename(save_dir) == "OGC_R0" and os.path.basename(os.path.dirname(save_dir)) == "segm_preds"
        for key in ("AP", "PQ", "F1", "Pre", "Rec", "per_scan_iou_avg", "per_scan_ri_avg"):
            assert 0 <= metrics[key] <= 1, key
        with open(config) as f:
            cfg = yaml.safe_load(f)
        torch.manual_seed(cfg["random_seed"])
        segnet = build_segnet(cfg).cuda().eval()
        ds = datasets.KITTIDetectionDataset(data_root, os.path.join(data_root, "val.txt"), decentralize=True)
        assert len(ds) == 4
        pc = torch.from_numpy(np.stack([ds[i][0][0] for i in range(4)])).cuda()
        with torch.no_grad():
            mask = segnet(pc, pc).float().cpu()
        top = mask.topk(2, dim=2).values
        clear = (top[..., 0] - top[..., 1] > 1e-4).numpy()
        want = mask.argmax(2).numpy()
        differ = 0
        for i in range(4):
            stored = np.load(os.path.join(save_dir, ds.data_ids[i], "segm.npy"))
            assert stored.dtype == np.int64 and stored.shape == (N_POINTS,)
            differ += int((stored != want[i])[clear[i]].sum())
        left_out = int((~clear).sum())
        print("TEST_SEG_SAVE points %d left out %d differing among the rest %d" % (clear.size, left_out, differ))
        assert left_out <= 0.05 * clear.size
        assert differ == 0
    finally:
        shutil.rmtree(data_root, ignore_errors=True)

"""ogc_amd.test_flow on the MI355X: `evaluate` against the same loop built from the existing tensor path
(ogc_amd/metrics/flow_metric.py::flow_metrics), and `main --save` end to end on synthetic SAPIEN (N = 512) and OGC-DR (N = 1024)
roots of 3 scenes x 4 frames: 18 ordered pairs, batches of 12 and 6, so the partial last batch is covered.

Bounds: the three rates within 2**-23 relative (both paths divide an exact count once; the stand-in predictions keep every point
at least 1e-5, relative, from the five thresholds — asserted — so the counts agree); EPE within 1e-6 relative (flow_metrics sums
up to 12 * 1024 fp32 norms in fp32; the kernel's own error is 4 * 2**-24 = 2.4e-7)."""
import importlib.util
import json
import os
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
N_SCENES, BATCH = 3, 12
N_POINTS = {"ogcdr": 1024, "sapien": 512}
RATE_RTOL, EPE_RTOL = 2.0 ** -23, 1e-6


def _recipe():
    spec = importlib.util.spec_from_file_location("make_flow_eval_golden", os.path.join(HERE, "golden", "make_flow_eval_golden.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def _test_set(tmp_path, dataset, predflow_path=None):
    from ogc_amd.test_flow import build_test_set
    from ogc_amd.utils.synthetic import write_ogcdr_root, write_sapien_root
    if dataset == "sapien":
        write_sapien_root(str(tmp_path / "mbs-shapepart"), N_SCENES, N_POINTS[dataset], split="val")
    else:
        write_ogcdr_root(str(tmp_path), N_SCENES, N_POINTS[dataset], split="val")
    return build_test_set(dataset, "val", str(tmp_path), predflow_path)[0]


def _stand_in_predictions(loader, thresh):
    """Per batch gt + a unit direction times thresh * 10**U(-1.5, 1.5), seeded, re-drawn until every point keeps the fixture's margin."""
    recipe = _recipe()
    g = torch.Generator().manual_seed(77)
    preds = []
    for _, _, flows, _ in loader:
        gt = flows[:, 0]
        for _ in range(16):     # the generator goes on: the first draw that keeps the margin
            direction = torch.randn(gt.shape, generator=g, dtype=torch.float64)
            direction /= direction.norm(dim=2, keepdim=True)
            magnitude = thresh * 10.0 ** (3.0 * torch.rand(gt.shape[0], gt.shape[1], 1, generator=g, dtype=torch.float64) - 1.5)
            pred = (gt.double() + direction * magnitude).float()
            if recipe.truth64(gt.numpy(), pred.numpy(), thresh)[2] > recipe.MARGIN:
                break
        assert recipe.truth64(gt.numpy(), pred.numpy(), thresh)[2] > recipe.MARGIN
        preds.append(pred)
    return preds


@pytest.mark.parametrize("dataset", ("ogcdr", "sapien"))
def test_evaluate_equals_the_existing_tensor_path(tmp_path, dataset):
    from ogc_amd.metrics.flow_metric import flow_metrics
    from ogc_amd.test_flow import EPE_NORM_THRESH, evaluate
    from ogc_amd.utils.pytorch_util import AverageMeter
    loader = torch.utils.data.DataLoader(_test_set(tmp_path, dataset), batch_size=BATCH, shuffle=False, num_workers=0)
    preds = _stand_in_predictions(loader, EPE_NORM_THRESH)
    assert [p.shape[0] for p in preds] == [12, 6]
    served, seen = iter(preds), []
    got = evaluate(lambda pc1, pc2, f1, f2, iters: [None, next(served).cuda()], loader, torch.device("cuda"), EPE_NORM_THRESH, 4,
                   on_batch=lambda i, flow_pred: seen.append((i, tuple(flow_pred.shape), flow_pred.is_cuda)))
    assert seen == [(0, (12, N_POINTS[dataset], 3), True), (1, (6, N_POINTS[dataset], 3), True)]
    meter = AverageMeter()
    for (_, _, flows, _), pred in zip(loader, preds):
        epe, acc_s, acc_r, outlier = flow_metrics(flows[:, 0].cuda(), pred.cuda(), EPE_NORM_THRESH).tolist()
        meter.append_loss({"EPE": epe, "AccS": acc_s, "AccR": acc_r, "Outlier": outlier})
    want = meter.get_mean_loss_dict()
    print("TEST_FLOW_PARITY %s " % dataset + " ".join("%s %.8f (rel %.2e)" % (k, got[k], abs(got[k] - want[k]) / want[k]) for k in want))
    assert set(got) == {"EPE", "AccS", "AccR", "Outlier"}
    for key in ("AccS", "AccR", "Outlier"):
        assert 0.05 < want[key] < 0.95                     # the stand-in straddles the thresholds
        assert abs(got[key] - want[key]) <= RATE_RTOL * want[key]
    assert abs(got["EPE"] - want["EPE"]) <= EPE_RTOL * want["EPE"]


@pytest.mark.parametrize("dataset", ("ogcdr", "sapien"))
def test_main_saves_what_the_network_predicted(dataset):
    from ogc_amd import datasets
    from ogc_amd.test_flow import VIEW_SELS, main
    config = os.path.join(ROOT, "config", "%s_flow_test_synthetic.yaml" % dataset)
    recorded = []
    metrics = main([config, "--split", "val", "--synthetic", str(N_SCENES), "--test_batch_size", str(BATCH), "--save",
                    "--num_workers", "0"], on_batch=lambda i, flow_pred: recorded.append(flow_pred.cpu().numpy()))
    save_dir = metrics["save_dir"]
    data_root = os.path.dirname(os.path.dirname(save_dir))
    tmp = os.path.dirname(data_root) if dataset == "sapien" else data_root
    try:
        n = N_POINTS[dataset]
        assert [r.shape for r in recorded] == [(12, n, 3), (6, n, 3)]
        assert all(np.isfinite(metrics[k]) for k in ("EPE", "AccS", "AccR", "Outlier")) and metrics["EPE"] > 0
        assert json.load(open(save_dir + ".json")) == {"view_sel": VIEW_SELS}
        files = sorted(os.listdir(save_dir))
        assert len(files) == N_SCENES and all(np.load(os.path.join(save_dir, f)).shape == (6, n, 3) for f in files)
        cls = datasets.SapienDataset if dataset == "sapien" else datasets.OGCDynamicRoomDataset
        ds = cls(data_root=data_root, split="val", view_sels=VIEW_SELS, predflow_path="flowstep3d")
        predicted = np.concatenate(recorded)
        assert len(ds) == predicted.shape[0] == 6 * N_SCENES
        for sid in range(len(ds)):
            flows = ds[sid][2]
            assert flows[0].tobytes() == predicted[sid].tobytes(), sid
            assert flows[1].tobytes() == predicted[sid ^ 1].tobytes(), sid   # the pair's other direction is its neighbour
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def test_save_needs_whole_scenes_in_a_batch():
    from ogc_amd.test_flow import main
    config = os.path.join(ROOT, "config", "ogcdr_flow_test_synthetic.yaml")
    with pytest.raises(ValueError) as err:
        main([config, "--split", "val", "--synthetic", "1", "--test_batch_size", "8", "--save", "--num_workers", "0"])
    assert "multiple of 6" in str(err.value)

"""The supervised Waymo trainer against THE REFERENCE'S OWN train_seg_waymo_sup.Trainer.train, and the two Waymo drivers end to
end.

tests/golden/train_seg_waymo_sup_trace.npz holds what the reference's trainer did over 2 epochs of the six-scene, 512-point set of
tests/waymo_sup_cases.py (batches (pcs, segms, valids)) with segnet_kitti (tests/golden/make_waymo_sup_golden.py ran it),
train_seg_waymo_sup_trace_f64.npz the same run in float64.  ogc_amd.train_seg_waymo_sup.Trainer replays it and must reproduce,
iteration by iteration, the loss_dict, the learning rate, the norm momentum and the weights after the step, including the
NaN-gradient step that must change nothing; epoch by epoch the validation loss and loss_dict, PQ / F1 / Pre / Rec AT THRESHOLD 0
and the best-checkpoint decision.  The comparison rule and the tolerances are those of tests/test_train_sup_driver.py (which
takes them from tests/test_driver_golden.py).  CPU test on the oracle's operators.

The GPU test runs `train_seg_waymo_sup --synthetic` for a few steps, then `test_seg_waymo --save` on the checkpoint it left, and
compares the printed metrics with the numpy path (metrics/seg_metric_ignmask.py) on the very masks the evaluation saw."""
import json
import os

import numpy as np
import pytest
import torch

import sup_cases as sc
import waymo_sup_cases as wc
from test_driver_golden import BUDGET, WEIGHT_REL, Budget, load, rel_l2, weight_summary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIOU_TOL = 64 * 2.0 ** -24


def run_waymo_sup(dev, tmp_path):
    from ogc_amd.models.segnet_kitti import MaskFormer3D
    from ogc_amd.train_seg import norm_momentum, schedule_factor
    from ogc_amd.train_seg_sup import build_sup_criterion
    from ogc_amd.train_seg_waymo_sup import Trainer
    from ogc_amd.train_step import make_optimizer
    from ogc_amd.utils.pytorch_util import BNMomentumScheduler, LambdaLR
    gold, truth, cfg = load("train_seg_waymo_sup_trace"), load("train_seg_waymo_sup_trace_f64"), wc.CFG
    net = sc.detgen.fill_module(MaskFormer3D(**cfg["segnet"]), 35).to(dev)
    optimizer = make_optimizer(net.parameters(), lr=cfg["lr"], weight_decay=cfg["weight_decay"])
    lr_scheduler = LambdaLR(optimizer, lr_lambda=lambda it: schedule_factor(cfg, it * cfg["batch_size"]))
    bnm_scheduler = BNMomentumScheduler(net, bn_lambda=lambda it: norm_momentum(cfg, it * cfg["batch_size"]))
    names = list(gold["loss_names"])
    seen, after, lines = [], [], []
    trainer = Trainer(net, build_sup_criterion(cfg["loss"]), optimizer, str(tmp_path / "sup"), lr_scheduler=lr_scheduler,
                      bnm_scheduler=bnm_scheduler, device=torch.device(dev), log=lines.append,
                      on_iteration=lambda it, ld, stepped: seen.append((it, [ld[k] for k in names], stepped)))
    assert trainer.ignore_npoint_thresh == 0
    inner = trainer._train_it

    def recording(it, batch, aug_transform=False, **kw):
        out = inner(it, batch, aug_transform, **kw)
        mom = next(m.momentum for m in net.modules() if isinstance(m, torch.nn.GroupNorm))
        after.append((optimizer.param_groups[0]["lr"], mom) + weight_summary(net))
        return out

    trainer._train_it = recording
    seed = int(gold["data_seed"][0])
    train_set, val_set = wc.WaymoSupScenes(True, seed), wc.WaymoSupScenes(False, seed)
    sc.nan_gradient_hook(net, train_set)
    train_loader = torch.utils.data.DataLoader(train_set, batch_size=cfg["batch_size"], shuffle=False)
    val_loader = torch.utils.data.DataLoader(val_set, batch_size=cfg["batch_size"], shuffle=False)
    best = trainer.train(cfg["epochs"], train_loader, val_loader)

    assert len(seen) == len(after) == len(gold["lr"]) == 6
    nan_it = 5   # the second time scene 5 is drawn (the last iteration of epoch 2): its gradients are NaN
    budget, ref_w, worst_w = Budget(names), 0.0, 0.0
    for i, ((it, losses, stepped), (lr, mom, norms, heads)) in enumerate(zip(seen, after)):
        assert it == i
        budget.close(losses, gold["loss"][i], truth["loss"][i], names, "iteration %d" % i)
        assert abs(lr - gold["lr"][i]) <= 1e-12 and abs(mom - gold["momentum"][i]) <= 1e-12, (i, lr, mom)
        assert stepped == (i != nan_it), "iteration %d: NaN rule" % i
        ref_w = max(ref_w, rel_l2(gold["heads"][i], truth["heads"][i]))
        w32, w64 = rel_l2(heads, gold["heads"][i]), rel_l2(heads, truth["heads"][i])
        assert w32 <= WEIGHT_REL or w64 <= WEIGHT_REL + BUDGET * ref_w, \
            "iteration %d: weights %.2e from the reference's fp32 run, %.2e from the float64 truth (reference itself: %.2e)" % (i, w32, w64, ref_w)
        worst_w = max(worst_w, w32)
    assert np.array_equal(after[nan_it][3], after[nan_it - 1][3]) and not np.array_equal(after[nan_it - 1][3], after[nan_it - 2][3])
    assert np.array_equal(gold["heads"][nan_it], gold["heads"][nan_it - 1])
    recs = [json.loads(line) for line in lines]
    assert [r["skipped_steps"] for r in recs] == [0, 1]
    vnames = list(gold["val_names"])
    vbudget = Budget(vnames)
    vbudget.worst = dict(budget.worst)
    for e, r in enumerate(recs):
        vbudget.close([r["val_loss"]], [gold["val_loss"][e]], [truth["val_loss"][e]], ["sum"], "epoch %d validation loss" % (e + 1), atol=1e-5)
        vbudget.close([r["val_terms"][k] for k in vnames], gold["val_avg"][e], truth["val_avg"][e], vnames,
                      "epoch %d validation" % (e + 1), atol=2e-5)
        got_pq = [r["val"][k] for k in ("PQ", "F1", "Pre", "Rec")]
        assert np.allclose(got_pq, gold["val_pq"][e], atol=1e-4), (got_pq, gold["val_pq"][e])
        assert r["is_best"] == bool(gold["is_best"][e])
    vbudget.close([best], [float(gold["best"][0])], [float(truth["best"][0])], ["sum"], "best validation loss", atol=1e-6)
    assert sorted(os.listdir(str(tmp_path / "sup"))) == ["best.pth.tar", "current.pth.tar"]
    ck = torch.load(str(tmp_path / "sup" / "best.pth.tar"))
    assert sorted(ck.keys()) == list(gold["ckpt_top"]) and sorted(ck["model_state"].keys()) == list(gold["ckpt_keys"])
    return worst_w


def test_waymo_sup_trainer_replays_the_reference_trainer_cpu(tmp_path, monkeypatch, oracle):
    import ogc_amd.pointnet2.pointnet2 as api
    monkeypatch.setattr(api, "_native", oracle.Pointnet2CudaCPU())
    run_waymo_sup("cpu", tmp_path)


def test_trace_shares_the_stable_seed_of_the_sup_trace():
    """The two reference trainers differ in the monitored metrics only: the losses of this trace equal train_seg_sup's, whose data
    seed was chosen for a run that does not move under one-ulp changes of the inputs (make_waymo_sup_golden.py asserts it too)."""
    gold, sup = load("train_seg_waymo_sup_trace"), load("train_seg_sup_trace")
    assert int(gold["data_seed"][0]) == int(sup["data_seed"][0])
    assert np.array_equal(gold["loss"], sup["loss"]) and np.array_equal(gold["val_loss"], sup["val_loss"])


def test_constructor_and_batches_are_the_reference_s(tmp_path, monkeypatch, oracle):
    """No `ignore_npoint_thresh` argument; `_train_it` takes (pcs, segms, valids) and returns what the reference returns."""
    import inspect
    import ogc_amd.pointnet2.pointnet2 as api
    from ogc_amd.models.segnet_kitti import MaskFormer3D
    from ogc_amd.train_seg_sup import build_sup_criterion
    from ogc_amd.train_seg_waymo_sup import IGNORE_CLASS_IDS, Trainer
    from ogc_amd.train_step import make_optimizer
    monkeypatch.setattr(api, "_native", oracle.Pointnet2CudaCPU())
    params = list(inspect.signature(Trainer.__init__).parameters)
    assert params[:7] == ["self", "segnet", "criterion", "optimizer", "exp_base", "lr_scheduler", "bnm_scheduler"]
    assert IGNORE_CLASS_IDS == [2, 3]
    cfg = wc.CFG
    net = sc.detgen.fill_module(MaskFormer3D(**cfg["segnet"]), 35)
    trainer = Trainer(net, build_sup_criterion(cfg["loss"]), make_optimizer(net.parameters(), lr=cfg["lr"]), str(tmp_path / "x"))
    loader = torch.utils.data.DataLoader(wc.WaymoSupScenes(False), batch_size=2, shuffle=False)
    batch = next(iter(loader))
    assert len(batch) == 3
    loss_dict, segm, mask = trainer._train_it(0, batch)
    assert sorted(loss_dict) == ["cross_entropy", "dice", "sum"] and all(isinstance(v, float) for v in loss_dict.values())
    assert segm.shape == (2, sc.N_SUP) and mask.shape == (2, sc.N_SUP, sc.K_SUP) and not mask.requires_grad


def test_config_is_the_reference_schema():
    import yaml
    with open(os.path.join(ROOT, "config", "waymo_sup_synthetic.yaml")) as f:
        cfg = yaml.safe_load(f)
    assert cfg["dataset"] == "waymo" and cfg["segnet"]["n_slot"] == 22 and cfg["ignore_npoint_thresh"] == 50
    for key in ("save_path", "random_seed", "epochs", "batch_size", "lr", "lr_decay", "lr_clip", "bn_momentum", "bn_decay",
                "weight_decay", "decay_step", "loss", "data"):
        assert key in cfg, key
    assert cfg["loss"]["weights"] == [2.0, 0] and cfg["loss"]["use_focal"] is False


@pytest.mark.gpu
def test_command_line_driver_then_test_seg_waymo_on_its_checkpoint(tmp_path, capsys, monkeypatch):
    import yaml
    from ogc_amd import test_seg_waymo, train_seg_waymo_sup
    from ogc_amd.metrics import seg_metric_ignmask as cpu
    with open(os.path.join(ROOT, "config", "waymo_sup_synthetic.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg["save_path"] = str(tmp_path / "ckpt" / "waymo_sup")
    cfg["segnet"]["n_point"] = 2048
    cfg["batch_size"] = 2
    cfg["data"]["root"] = str(tmp_path / "root")       # where test_seg_waymo --synthetic writes, and saves
    path = str(tmp_path / "waymo_sup.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    best = train_seg_waymo_sup.main([path, "--synthetic", "2", "--max-iters", "6", "--num_workers", "0"])
    lines = [json.loads(line) for line in capsys.readouterr().out.splitlines() if line.startswith("{")]
    assert len(lines) == 2 and lines[-1]["it"] == 6 and all(r["skipped_steps"] == 0 for r in lines)
    assert np.isfinite(best) and all(np.isfinite(r["train"]["sum"]) and np.isfinite(r["val_loss"]) for r in lines)
    assert all(np.isfinite(list(r["val"].values())).all() and np.isfinite(list(r["train_pq"].values())).all() for r in lines)
    assert sorted(os.listdir(cfg["save_path"])) == ["best.pth.tar", "current.pth.tar"]

    seen = {"masks": []}
    real_evaluate = test_seg_waymo.evaluate

    def recording_evaluate(segnet, loader, *args, **kwargs):
        def recorder(pc1, pc2):
            mask = segnet(pc1, pc2)
            seen["masks"].append(mask.detach().float().cpu())
            return mask
        seen["set"] = loader.dataset
        return real_evaluate(recorder, loader, *args, **kwargs)

    monkeypatch.setattr(test_seg_waymo, "evaluate", recording_evaluate)
    metrics = test_seg_waymo.main([path, "--split", "val", "--synthetic", "2", "--save", "--num_workers", "0",
                                   "--test_batch_size", "4"])
    out = capsys.readouterr().out
    assert "Loaded weights from %s" % os.path.join(cfg["save_path"], "best.pth.tar") in out
    assert "AveragePrecision@50:" in out and "PanopticQuality@50:" in out and "per_scan_iou_avg" in out
    keys = ("AP", "PQ", "F1", "Pre", "Rec", "per_scan_iou_avg", "per_scan_iou_std", "per_scan_ri_avg", "per_scan_ri_std")
    assert all(np.isfinite(metrics[k]) for k in keys)

    test_set, masks = seen["set"], torch.cat(seen["masks"]).numpy()
    assert test_set.ignore_class_ids == [2, 3] and test_set.ignore_npoint_thresh == 50 and test_set.downsampled
    assert len(test_set) == masks.shape[0] == 2 * train_seg_waymo_sup.SYNTHETIC_FRAMES and masks.shape[2] == 22
    # the files: <root>/segm_preds/OGC_R0/<sequence>/segm_%04d.npy, the arg-max of the masks
    save_dir = os.path.join(cfg["data"]["root"], "segm_preds", "OGC_R0")
    assert metrics["save_dir"] == save_dir
    for sid, (name, view) in enumerate(test_set.data_ids):
        saved = np.load(os.path.join(save_dir, name, "segm_%04d.npy" % view))
        assert saved.dtype == np.int64 and np.array_equal(saved, masks[sid].argmax(1))
    assert sum(len(files) for _, _, files in os.walk(save_dir)) == len(test_set)

    # the numpy path on the same masks
    samples = [test_set[sid] for sid in range(len(test_set))]
    segm = np.stack([s[1][0] for s in samples])
    ignore = 1 - np.stack([s[2][0] for s in samples])
    assert 0 < ignore.sum() < ignore.size
    iou, matched, conf, n_gt = cpu.accumulate_eval_results(segm, masks, ignore)
    clu = cpu.ClusteringMetrics()(masks, segm, ignore)
    pq, f1, pre, rec = cpu.calculate_PQ_F1(iou, matched, n_gt)
    assert (metrics["F1"], metrics["Pre"], metrics["Rec"]) == (float(f1), float(pre), float(rec))
    assert abs(metrics["PQ"] - pq) <= 1e-12 and abs(metrics["AP"] - cpu.calculate_AP(matched, conf, n_gt)) <= 1e-9
    assert abs(metrics["per_scan_iou_avg"] - np.mean(clu["iou"])) <= MIOU_TOL
    # eight bit-equal numbers of at most 1 averaged in two orders: seven additions of at most 2^-53 relative each, per side
    assert abs(metrics["per_scan_ri_avg"] - np.mean(clu["ri"])) <= 16 * 2.0 ** -53
    assert metrics["per_scan_iou_std"] == 0.0 and metrics["per_scan_ri_std"] == 0.0    # one frame per scan

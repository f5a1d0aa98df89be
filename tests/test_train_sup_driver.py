"""The supervised trainer against the REFERENCE'S OWN train_seg_sup.Trainer.train: tests/golden/train_seg_sup_trace.npz holds
what it did over 2 epochs of the six-scene, 512-point set of tests/sup_cases.py (SupScenes) with segnet_kitti
(tests/golden/make_sup_golden.py ran it), train_seg_sup_trace_f64.npz the same run in float64.  ogc_amd.train_seg_sup.Trainer
replays it — same configuration, data and initial weights — and must reproduce, iteration by iteration, the loss_dict, the
learning rate, the norm momentum and the weights after the step, including the NaN-gradient step that must change nothing;
epoch by epoch the validation loss and loss_dict, PQ / F1 / Pre / Rec and the best-checkpoint decision.  The comparison rule and
the tolerances are those tests/test_driver_golden.py applies to train_seg_trace (imported from there).  CPU test on the
oracle's operators (the loss's tensor path), GPU test on the HIP operators (the loss's kernel path).

One end-to-end GPU test runs the command-line driver on a --synthetic root for a few iterations and then test_seg on the
checkpoint it left."""
import json
import os

import numpy as np
import pytest
import torch

import sup_cases as sc
from test_driver_golden import BUDGET, WEIGHT_REL, Budget, load, rel_l2, weight_summary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_sup(dev, tmp_path):
    from ogc_amd.models.segnet_kitti import MaskFormer3D
    from ogc_amd.train_seg import norm_momentum, schedule_factor
    from ogc_amd.train_seg_sup import Trainer, build_sup_criterion
    from ogc_amd.train_step import make_optimizer
    from ogc_amd.utils.pytorch_util import BNMomentumScheduler, LambdaLR
    gold, truth, cfg = load("train_seg_sup_trace"), load("train_seg_sup_trace_f64"), sc.SUP_CFG
    net = sc.detgen.fill_module(MaskFormer3D(**cfg["segnet"]), 35).to(dev)
    optimizer = make_optimizer(net.parameters(), lr=cfg["lr"], weight_decay=cfg["weight_decay"])
    lr_scheduler = LambdaLR(optimizer, lr_lambda=lambda it: schedule_factor(cfg, it * cfg["batch_size"]))
    bnm_scheduler = BNMomentumScheduler(net, bn_lambda=lambda it: norm_momentum(cfg, it * cfg["batch_size"]))
    names = list(gold["loss_names"])
    seen, after, lines = [], [], []
    trainer = Trainer(net, build_sup_criterion(cfg["loss"]), optimizer, cfg["ignore_npoint_thresh"], str(tmp_path / "sup"),
                      lr_scheduler=lr_scheduler, bnm_scheduler=bnm_scheduler, device=torch.device(dev), log=lines.append,
                      on_iteration=lambda it, ld, stepped: seen.append((it, [ld[k] for k in names], stepped)))
    inner = trainer._train_it

    def recording(it, batch, aug_transform=False, **kw):
        out = inner(it, batch, aug_transform, **kw)
        mom = next(m.momentum for m in net.modules() if isinstance(m, torch.nn.GroupNorm))
        after.append((optimizer.param_groups[0]["lr"], mom) + weight_summary(net))
        return out

    trainer._train_it = recording
    seed = int(gold["data_seed"][0])   # the seed whose run is stable under one-ulp changes of the inputs (make_sup_golden.py)
    train_set, val_set = sc.SupScenes(True, seed), sc.SupScenes(False, seed)
    sc.nan_gradient_hook(net, train_set)
    train_loader = torch.utils.data.DataLoader(train_set, batch_size=cfg["batch_size"], shuffle=False)
    val_loader = torch.utils.data.DataLoader(val_set, batch_size=cfg["batch_size"], shuffle=False)
    import collections
    from ogc_amd import _lib
    _lib.CALL_COUNTS = collections.Counter()
    try:
        best = trainer.train(cfg["epochs"], train_loader, val_loader)
    finally:
        calls, _lib.CALL_COUNTS = _lib.CALL_COUNTS, None
    # the loss took the kernel path on the GPU (6 training steps, 2 validation batches), the tensor path on the CPU
    assert calls["ogc_sup_match_cost"] == calls["ogc_sup_mask_loss_fwd"] == (8 if dev == "cuda" else 0)
    assert calls["ogc_sup_mask_loss_bwd"] == (6 if dev == "cuda" else 0)

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
    # the NaN-gradient step changed nothing, the one before it did (as in the reference's own trace)
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


def test_train_seg_sup_trainer_replays_the_reference_trainer_cpu(tmp_path, monkeypatch, oracle):
    import ogc_amd.pointnet2.pointnet2 as api
    monkeypatch.setattr(api, "_native", oracle.Pointnet2CudaCPU())
    run_sup("cpu", tmp_path)


@pytest.mark.gpu
def test_train_seg_sup_trainer_replays_the_reference_trainer_gpu(tmp_path):
    print("weights rel L2 vs the reference's supervised trainer: %.2e" % run_sup("cuda", tmp_path))


def test_train_it_returns_what_the_reference_returns(tmp_path, monkeypatch, oracle):
    """(loss_dict of floats, GT labels (B, N), detached masks (B, N, K)); eval_epoch -> (loss, mean loss_dict, the AP meter)."""
    import ogc_amd.pointnet2.pointnet2 as api
    from ogc_amd.models.segnet_kitti import MaskFormer3D
    from ogc_amd.train_seg_sup import Trainer, build_sup_criterion
    from ogc_amd.train_step import make_optimizer
    monkeypatch.setattr(api, "_native", oracle.Pointnet2CudaCPU())
    cfg = sc.SUP_CFG
    net = sc.detgen.fill_module(MaskFormer3D(**cfg["segnet"]), 35)
    trainer = Trainer(net, build_sup_criterion(cfg["loss"]), make_optimizer(net.parameters(), lr=cfg["lr"]), 60, str(tmp_path / "x"))
    loader = torch.utils.data.DataLoader(sc.SupScenes(False), batch_size=2, shuffle=False)
    loss_dict, segm, mask = trainer._train_it(0, next(iter(loader)))
    assert sorted(loss_dict) == ["cross_entropy", "dice", "sum"] and all(isinstance(v, float) for v in loss_dict.values())
    assert segm.shape == (2, sc.N_SUP) and mask.shape == (2, sc.N_SUP, sc.K_SUP) and not mask.requires_grad
    val_loss, val_avg, ap = trainer.eval_epoch(loader)
    assert isinstance(val_loss, float) and sorted(val_avg) == ["cross_entropy", "dice", "sum"]
    assert sorted(ap) == ["Confidence", "N_GT_Inst", "Pred_IoU", "Pred_Matched"] and len(ap["Pred_IoU"]) == 1
    assert abs(val_loss - val_avg["sum"] / 2.0) <= 1e-6   # one batch: the sum divided by n + 1


@pytest.mark.gpu
def test_command_line_driver_then_test_seg_on_its_checkpoint(tmp_path, capsys):
    import yaml
    from ogc_amd import test_seg, train_seg_sup
    with open(os.path.join(ROOT, "config", "kittisf_sup_synthetic.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg["save_path"] = str(tmp_path / "ckpt" / "kittisf_sup")
    cfg["segnet"]["n_point"] = 1024
    cfg["batch_size"] = 4
    path = str(tmp_path / "sup.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    best = train_seg_sup.main([path, "--synthetic", "8", "--max-iters", "6", "--num_workers", "0"])
    lines = [json.loads(line) for line in capsys.readouterr().out.splitlines() if line.startswith("{")]
    assert len(lines) == 2 and lines[-1]["it"] == 6 and all(r["skipped_steps"] == 0 for r in lines)
    assert np.isfinite(best) and all(np.isfinite(r["train"]["sum"]) and np.isfinite(r["val_loss"]) for r in lines)
    assert sorted(os.listdir(cfg["save_path"])) == ["best.pth.tar", "current.pth.tar"]
    metrics = test_seg.main([path, "--split", "val", "--synthetic", "4", "--num_workers", "0", "--test_batch_size", "4"])
    assert "Loaded weights from" in capsys.readouterr().out
    assert all(np.isfinite(metrics[k]) for k in ("AP", "PQ", "F1", "Pre", "Rec", "per_scan_iou_avg", "per_scan_ri_avg"))

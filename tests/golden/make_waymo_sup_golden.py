"""Writes tests/golden/train_seg_waymo_sup_trace.npz (and, with the argument `trace64`, its float64 twin
train_seg_waymo_sup_trace_f64.npz, in a process of its own) by running THE REFERENCE'S OWN train_seg_waymo_sup.Trainer.train
(train_seg_waymo_sup.py:19-198, imported from /root/reference at generation time only) on the CPU, as make_sup_golden.py's
`trace` does for train_seg_sup: 2 epochs of the six-scene, 512-point set of tests/waymo_sup_cases.py (WaymoSupScenes: batches
(pcs, segms, valids)) with segnet_kitti, detgen weights, LambdaLR(lr_curve), BNMomentumScheduler(bn_curve) and a stubbed
tensorboardX.  Per iteration the loss_dict, the learning rate, the norm momentum and a summary of the weights after the step (one
NaN-gradient step included); per epoch the validation loss, its loss_dict, PQ / F1 / Pre / Rec (threshold 0: :107) and the
best-checkpoint decision.  Only data is written.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_waymo_sup_golden.py [trace64]

The data seed is the one stored in train_seg_sup_trace.npz, which make_sup_golden.py chose because its run does not move under
one-ulp changes of the coordinates.  The two trainers differ in the monitored metrics only, and this script asserts that the
float32 losses, learning rates, momenta and weights of this run EQUAL that trace's, so the choice carries over."""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import detgen  # noqa: E402
import sup_cases as sc  # noqa: E402
import waymo_sup_cases as wc  # noqa: E402
from make_golden import install_shims, save  # noqa: E402


def trace(f64, seed):
    import shutil
    import tempfile
    import types

    import train_seg_waymo_sup as ref
    from losses import seg_loss_sup as ref_loss
    from metrics.seg_metric import calculate_PQ_F1
    from models.segnet_kitti import MaskFormer3D
    from utils.pytorch_util import BNMomentumScheduler
    from make_driver_golden import weight_summary
    cfg = wc.CFG
    ref.args = types.SimpleNamespace(**cfg)
    if f64:     # the reference's einsum raises on its float32 permutation matrix times double labels
        inner_match = ref_loss.match_mask_by_cost
        ref_loss.match_mask_by_cost = lambda cost: inner_match(cost).to(cost.dtype)
    net = detgen.fill_module(MaskFormer3D(**cfg["segnet"]), 35)
    if f64:
        net = net.double()
    optimizer = torch.optim.Adam(net.parameters(), lr=cfg["lr"], weight_decay=cfg["weight_decay"])
    lr_scheduler = torch.optim.lr_scheduler.LambdaLR(optimizer, lr_lambda=ref.lr_curve)
    bnm_scheduler = BNMomentumScheduler(net, bn_lambda=ref.bn_curve)
    L = cfg["loss"]
    ce_loss = ref_loss.FocalLoss(**L["focal_loss_params"]) if L["use_focal"] else ref_loss.CrossEntropyLoss()
    criterion = ref_loss.SupervisedMaskLoss(ce_loss, ref_loss.DiceLoss(), weights=L["weights"])
    tmp = tempfile.mkdtemp()
    trainer = ref.Trainer(segnet=net, criterion=criterion, optimizer=optimizer, exp_base=os.path.join(tmp, "sup"),
                          lr_scheduler=lr_scheduler, bnm_scheduler=bnm_scheduler)
    dtype = np.float64 if f64 else np.float32
    train_set, val_set = wc.WaymoSupScenes(True, seed, 0, dtype), wc.WaymoSupScenes(False, seed, 0, dtype)
    sc.nan_gradient_hook(net, train_set)
    train_loader = torch.utils.data.DataLoader(train_set, batch_size=cfg["batch_size"], shuffle=False)
    val_loader = torch.utils.data.DataLoader(val_set, batch_size=cfg["batch_size"], shuffle=False)
    its, epochs = [], []
    inner, inner_eval = trainer._train_it, trainer.eval_epoch

    def recording_train_it(it, batch, aug_transform=False):
        out = inner(it, batch, aug_transform=aug_transform)
        norms, heads = weight_summary(net)
        mom = next(m.momentum for m in net.modules() if isinstance(m, torch.nn.GroupNorm))
        its.append(dict(loss=dict(out[0]), lr=optimizer.param_groups[0]["lr"], momentum=mom, norms=norms, heads=heads))
        return out

    def recording_eval(loader):
        val_loss, val_avg, ap = inner_eval(loader)
        pq = calculate_PQ_F1(np.concatenate(ap["Pred_IoU"]), np.concatenate(ap["Pred_Matched"]), np.sum(ap["N_GT_Inst"]))
        epochs.append(dict(val_loss=val_loss, val_avg=dict(val_avg), pq=pq))
        return val_loss, val_avg, ap

    trainer._train_it, trainer.eval_epoch = recording_train_it, recording_eval
    best = trainer.train(cfg["epochs"], train_loader, val_loader)
    names = sorted(its[0]["loss"])
    val_loss = np.array([e["val_loss"] for e in epochs])
    out = dict(loss_names=np.array(names), loss=np.array([[r["loss"][k] for k in names] for r in its], np.float64),
               lr=np.array([r["lr"] for r in its]), momentum=np.array([r["momentum"] for r in its]),
               norms=np.stack([r["norms"] for r in its]), heads=np.stack([r["heads"] for r in its]), val_loss=val_loss,
               val_names=np.array(sorted(epochs[0]["val_avg"])),
               val_avg=np.array([[e["val_avg"][k] for k in sorted(e["val_avg"])] for e in epochs]),
               val_pq=np.array([e["pq"] for e in epochs], np.float64), best=np.array([best]),
               is_best=np.array([v < np.min(np.append(val_loss[:i], 1e10)) for i, v in enumerate(val_loss)]),
               data_seed=np.array([seed]))
    ck = torch.load(os.path.join(tmp, "sup", "best.pth.tar"))
    out["ckpt_keys"], out["ckpt_top"] = np.array(sorted(ck["model_state"].keys())), np.array(sorted(ck.keys()))
    assert sorted(os.listdir(os.path.join(tmp, "sup"))) == ["best.pth.tar", "current.pth.tar"]    # the stub writes no log
    shutil.rmtree(tmp)
    assert np.isfinite(out["loss"]).all() and len(out["lr"]) == 6
    return out


if __name__ == "__main__":
    f64 = "trace64" in sys.argv[1:]
    writer = type("_Writer", (), {"__init__": lambda self, *a, **k: None, "add_scalar": lambda self, *a, **k: None,
                                  "flush": lambda self: None})
    if f64:
        from make_truth_f64 import install_shims_f64
        install_shims_f64()
        torch.set_default_dtype(torch.float64)
    else:
        install_shims()
    sys.modules["tensorboardX"].SummaryWriter = writer
    sup = np.load(os.path.join(HERE, "train_seg_sup_trace" + ("_f64" if f64 else "") + ".npz"))
    out = trace(f64, int(sup["data_seed"][0]))
    for key in ("loss", "lr", "momentum", "norms", "heads", "val_loss", "val_avg"):
        assert np.array_equal(out[key], sup[key]), "%s differs from the train_seg_sup trace" % key
    print("val PQ / F1 / Pre / Rec at threshold 0:", out["val_pq"].tolist(), "(train_seg_sup's at 60:", sup["val_pq"].tolist(), ")")
    save("train_seg_waymo_sup_trace" + ("_f64" if f64 else ""), **out)

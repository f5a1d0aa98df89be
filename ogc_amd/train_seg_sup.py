"""Supervised segmentation training driver: the `OGC_sup` baseline an unsupervised result is compared with (counterpart of the
reference's train_seg_sup.py:19-347 with losses/seg_loss_sup.py, on this package's layers).

    python -m ogc_amd.train_seg_sup config.yaml [--round R] [--synthetic N_SCENES] [--max-iters K] [--data-root DIR]

One frame per sample: the network sees frame 0 of the pair, the loss (ogc_amd/losses/seg_loss_sup.py: Hungarian matching by a
cross-entropy or focal + Dice cost, then the same terms on the matched pairs) compares its soft masks with the one-hot labels
the readers deliver under `onehot_label=True` (ogc_amd/datasets.py).  Kept from the reference so that its configs and
checkpoints carry over: the YAML schema (config/seg/*/*_sup.yaml: loss{use_focal, focal_loss_params, weights},
ignore_npoint_thresh, data{...}), Adam + LambdaLR(lr_curve) + the norm-momentum schedule driven by `it * batch_size`, the
NaN-gradient rule, `current` / `best` checkpoints chosen by the validation loss (its sum over n batches divided by n + 1, the
reference's counter), the initial weights saved as both.  The checkpoint directory is `<save_path>` for round 0 and
`<save_path>_R<round>` otherwise, which is where `test_seg --round R` looks.

What differs from the reference is invisible in the numbers: the optimiser step is train_step's (the NaN rule and Adam on the
device, no host round trip), the loss does not synchronise (sync=False), and the monitored PQ / F1 / Pre / Rec of every
iteration and epoch come from metrics.seg_eval — one ogc_seg_eval launch and one small copy — where the reference copies the
full soft masks to the host every iteration.  `_train_it` therefore returns device tensors.  No tensorboard: one JSON line per
epoch.  The Waymo baseline (train_seg_waymo_sup.py) is ogc_amd/train_seg_waymo_sup.py, a subclass of this Trainer on batches
without flows.  Out of scope: data-parallel training, HIP-graph replay.

Self-training (kittidet): `data.load_prediction: NAME` makes the TRAIN set read its labels from <root>/segm_preds/NAME, where
`export_pseudo_labels --split train` (or `test_seg --split train --save`) left them, and `data.load_confidence: true` scales
every object's target column by the confidence `export_pseudo_labels` wrote beside them (datasets.py, the reference's reader
arguments).  The validation set keeps its ground truth.  The reference's trainer never passes these two arguments to its reader:
the config keys are this package's own.
"""
import argparse
import json
import os
import shutil
import tempfile
import time

import numpy as np
import torch
import yaml

from .losses.seg_loss_sup import CrossEntropyLoss, DiceLoss, FocalLoss, SupervisedMaskLoss
from .train_seg import MAX_CONSECUTIVE_SKIPS, norm_momentum, schedule_factor
from .train_step import PendingStep, _must_surface, _nan_safe_step, make_optimizer
from .utils.pytorch_util import AverageMeter, BNMomentumScheduler, LambdaLR, checkpoint_state, save_checkpoint

DATASETS = ("sapien", "ogcdr", "kittisf", "kittidet")
INDOOR_VIEW_SELS = [[0, 1], [1, 2], [2, 3], [3, 2]]      # train_seg_sup.py:267
KITTISF_VIEW_SELS = [[0, 1], [1, 0]]                      # train_seg_sup.py:286


def build_sup_criterion(cfg):
    """The `loss` block of a *_sup.yaml -> SupervisedMaskLoss (train_seg_sup.py:329-335)."""
    ce_loss = FocalLoss(**cfg["focal_loss_params"]) if cfg["use_focal"] else CrossEntropyLoss()
    return SupervisedMaskLoss(ce_loss, DiceLoss(), weights=cfg["weights"])


def _eval_results(segm, mask, ignore_npoint_thresh):
    """(Pred_IoU, Pred_Matched, Confidence, N_GT_Inst) of a batch: the evaluation kernel on the GPU, the tensor path elsewhere."""
    if mask.is_cuda:
        from .metrics.seg_eval import accumulate_seg_eval
        return accumulate_seg_eval(segm, mask.float(), ignore_npoint_thresh)[:4]
    from .metrics.seg_metric import accumulate_eval_results
    return accumulate_eval_results(segm, mask, ignore_npoint_thresh)


def _pq(meter):
    from .metrics.seg_metric import calculate_PQ_F1
    pq, f1, pre, rec = calculate_PQ_F1(np.concatenate(meter["Pred_IoU"]), np.concatenate(meter["Pred_Matched"]),
                                       int(np.sum(meter["N_GT_Inst"])))
    return {"PQ": round(float(pq), 4), "F1": round(float(f1), 4), "Pre": round(float(pre), 4), "Rec": round(float(rec), 4)}


def _new_meter():
    return {"Pred_IoU": [], "Pred_Matched": [], "Confidence": [], "N_GT_Inst": []}


def _append(meter, results):
    for key, value in zip(("Pred_IoU", "Pred_Matched", "Confidence", "N_GT_Inst"), results):
        meter[key].append(value)


class Trainer(object):
    """The reference's Trainer (train_seg_sup.py:19-202): same constructor arguments, `_train_it(it, batch)`,
    `eval_epoch(loader)` and `train(n_epochs, train_loader, test_loader)`, same schedule calls, NaN rule, best-checkpoint rule
    and checkpoint files.  Keyword-only extras: the device the batches go to, a cap on the number of iterations, a log sink
    and a per-iteration callback for tests."""

    def __init__(self, segnet, criterion, optimizer, ignore_npoint_thresh, exp_base, lr_scheduler=None, bnm_scheduler=None, *,
                 device=None, max_iters=0, log=print, on_iteration=None):
        self.segnet = segnet
        self.criterion = criterion
        self.optimizer = optimizer
        self.ignore_npoint_thresh = ignore_npoint_thresh
        self.lr_scheduler = lr_scheduler
        self.bnm_scheduler = bnm_scheduler
        self.exp_base = exp_base
        self.device = device if device is not None else next(segnet.parameters()).device
        self.max_iters, self.log, self.on_iteration = max_iters, log, on_iteration
        os.makedirs(exp_base, exist_ok=True)
        self.checkpoint_name, self.best_name = "current", "best"
        self.cur_epoch = 0
        self._skipped_in_a_row = 0

    def _frame0(self, batch):
        pcs, segms, _, valids = batch
        return tuple(x[:, 0].contiguous().to(self.device, non_blocking=True) for x in (pcs, segms, valids))

    # ---- one optimisation step (train_seg_sup.py:45-79)
    def _train_it(self, it, batch, aug_transform=False, sync=True):
        """-> (loss_dict, segm (B, N) GT labels, mask (B, N, K) detached), the tensors on the trainer's device.  With sync=False
        the first item is a PendingStep whose result() gives (loss_dict, stepped) without having stopped the launch thread."""
        from .utils.streams import HostScalars
        self.segnet.train()
        if self.lr_scheduler is not None:
            self.lr_scheduler.step(it)
        if self.bnm_scheduler is not None:
            self.bnm_scheduler.step(it)
        self.optimizer.zero_grad(set_to_none=True)
        pc, gt_mask, valid = self._frame0(batch)
        mask = self.segnet(pc, pc)
        loss, losses = self.criterion(mask, gt_mask, valid, sync=False)
        segm = gt_mask.argmax(2)
        try:
            loss.backward()
            flag = _nan_safe_step(list(self.segnet.parameters()), self.optimizer)
        except RuntimeError as err:     # the reference returns without stepping (:69-72)
            if _must_surface(err):
                raise
            flag = HostScalars(torch.tensor([True]))
        pending = PendingStep(losses, flag)
        return (pending.result()[0] if sync else pending), segm, mask.detach()

    # ---- validation (train_seg_sup.py:82-116)
    def eval_epoch(self, d_loader):
        """(validation loss, mean loss_dict, {'Pred_IoU', 'Pred_Matched', 'Confidence', 'N_GT_Inst'} lists).  The loss is the
        reference's number: the sum over the n batches divided by n + 1 (its counter starts at 1.0, :88, :116)."""
        self.segnet.eval()
        eval_meter = AverageMeter()
        total_loss, count = 0.0, 1.0
        ap_eval_meter = _new_meter()
        with torch.no_grad():
            for batch in d_loader:
                pc, gt_mask, valid = self._frame0(batch)
                mask = self.segnet(pc, pc)
                loss, loss_dict = self.criterion(mask, gt_mask, valid)
                total_loss += float(loss)
                count += 1
                eval_meter.append_loss(loss_dict)
                _append(ap_eval_meter, _eval_results(gt_mask.argmax(2), mask, self.ignore_npoint_thresh))
        return total_loss / count, eval_meter.get_mean_loss_dict(), ap_eval_meter

    def _save(self, is_best):
        save_checkpoint(checkpoint_state(self.segnet), is_best, filename=os.path.join(self.exp_base, self.checkpoint_name),
                        bestname=os.path.join(self.exp_base, self.best_name))

    # ---- the epoch loop (train_seg_sup.py:119-202)
    def train(self, n_epochs, train_loader, test_loader=None):
        it, best_loss = 0, 1e10
        self._save(True)    # the initial weights as current and best (:125-128)
        for epoch in range(1, n_epochs + 1):
            self.cur_epoch = epoch
            train_meter, ap_meter, t0, skipped = AverageMeter(), _new_meter(), time.time(), 0
            for batch in train_loader:
                pending, segm, mask = self._train_it(it, batch, sync=False)
                # the step is queued; this copy (the iteration's only one besides the three scalars) waits for the forward pass
                _append(ap_meter, _eval_results(segm, mask, self.ignore_npoint_thresh))
                loss_dict, stepped = pending.result()
                skipped += 0 if stepped else 1
                self._skipped_in_a_row = 0 if stepped else self._skipped_in_a_row + 1
                if self._skipped_in_a_row >= MAX_CONSECUTIVE_SKIPS:
                    raise RuntimeError("%d optimisation steps in a row were skipped (NaN gradients or a failing backward pass): "
                                       "the weights are not being updated" % self._skipped_in_a_row)
                train_meter.append_loss(loss_dict)
                if self.on_iteration is not None:
                    self.on_iteration(it, loss_dict, stepped)
                it += 1
                if self.max_iters and it >= self.max_iters:
                    break
            record = {"epoch": epoch, "it": it, "lr": self.optimizer.param_groups[0]["lr"],
                      "train": {k: round(v, 5) for k, v in train_meter.get_mean_loss_dict().items()}, "train_pq": _pq(ap_meter),
                      "skipped_steps": skipped}
            if test_loader is not None:
                val_loss, val_avg, ap = self.eval_epoch(test_loader)
                is_best = val_loss < best_loss
                best_loss = min(best_loss, val_loss)
                self._save(is_best)
                record.update(val_loss=round(val_loss, 5), val_terms={k: round(v, 5) for k, v in val_avg.items()}, is_best=is_best,
                              val=_pq(ap))
            record["sec"] = round(time.time() - t0, 2)
            self.log(json.dumps(record))
            if self.max_iters and it >= self.max_iters:
                break
        return best_loss


def checkpoint_dir(cfg, round_):
    """<save_path> for round 0, <save_path>_R<round> otherwise: where test_seg.weight_path looks."""
    return cfg["save_path"] + ("_R%d" % round_ if round_ > 0 else "")


def build_sets(cfg, roots):
    """(train set, validation set) of the config's dataset with one-hot labels (train_seg_sup.py:265-319).  roots: {split:
    (data root, split file or None)}."""
    from . import datasets
    name, data, n_slot = cfg["dataset"], cfg.get("data") or {}, cfg["segnet"]["n_slot"]
    decentralize = bool(data.get("decentralize", False))
    aug = dict(aug_transform=bool(data.get("aug_transform", False)), aug_transform_args=data.get("aug_transform_args"))
    if aug["aug_transform_args"] in (None, "None"):   # the reference's ogcdr_sup.yaml spells it as the string
        aug = dict(aug_transform=False, aug_transform_args=None)
    thresh = cfg.get("ignore_npoint_thresh", 0)
    out = []
    for split, extra in (("train", aug), ("val", {})):
        root, mapping = roots[split]
        if name in ("sapien", "ogcdr"):
            cls = datasets.SapienDataset if name == "sapien" else datasets.OGCDynamicRoomDataset
            sub = os.path.join(root, "mbs-shapepart")                                    # train_seg_sup.py:268-269
            out.append(cls(data_root=sub if name == "sapien" and os.path.isdir(sub) else root, split=split,
                           view_sels=INDOOR_VIEW_SELS, decentralize=decentralize, onehot_label=True, max_n_object=n_slot, **extra))
        elif name == "kittisf":
            out.append(datasets.KITTISceneFlowDataset(data_root=root, mapping_path=mapping, downsampled=True,
                                                      view_sels=KITTISF_VIEW_SELS, decentralize=decentralize, onehot_label=True,
                                                      max_n_object=n_slot, ignore_npoint_thresh=thresh, **extra))
        elif name == "kittidet":
            if split == "train":   # the predictions of another model as labels; validation stays on the ground truth
                extra = dict(extra, load_prediction=data.get("load_prediction"),
                             load_confidence=bool(data.get("load_confidence", False)))
            out.append(datasets.KITTIDetectionDataset(data_root=root, mapping_path=mapping, decentralize=decentralize,
                                                      onehot_label=True, max_n_object=n_slot, ignore_npoint_thresh=thresh, **extra))
        else:
            raise KeyError("Unrecognized dataset %r (the supervised trainer covers %s)" % (name, ", ".join(DATASETS)))
    return tuple(out)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("config")
    ap.add_argument("--round", type=int, default=0)
    ap.add_argument("--synthetic", type=int, default=0,
                    help="train on this many labelled synthetic scenes written to a temporary root (utils/synthetic.py)")
    ap.add_argument("--max-iters", type=int, default=0, help="stop after this many optimisation steps (0 = all epochs)")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--data-root", default=None, help="the data set's root (default: data.root of the config)")
    ap.add_argument("--num_workers", type=int, default=4)
    args = ap.parse_args(argv)
    with open(args.config) as f:
        cfg = yaml.safe_load(f)
    if cfg["dataset"] not in DATASETS:
        raise KeyError("Unrecognized dataset %r (the supervised trainer covers %s)" % (cfg["dataset"], ", ".join(DATASETS)))
    device = torch.device(args.device)
    np.random.seed(cfg["random_seed"])
    torch.manual_seed(cfg["random_seed"])
    if device.type == "cuda" and cfg.get("matmul_precision", "fp32") != "fp32":
        from .pointnet2 import pointnet2 as _api
        _api._native.set_matmul_precision(cfg["matmul_precision"])
    from .test_seg import build_segnet
    net = build_segnet(cfg).to(device)

    data, tmp = cfg.get("data") or {}, None
    if args.synthetic:
        from .utils.synthetic import write_supervised_roots
        tmp = tempfile.mkdtemp(prefix="ogc_train_seg_sup_")
        roots = write_supervised_roots(tmp, cfg["dataset"], args.synthetic, max(args.synthetic // 4, cfg["batch_size"]),
                                       data.get("n_points", cfg["segnet"]["n_point"]), data.get("n_objects", 4))
    else:
        root = args.data_root or data["root"]
        roots = {"train": (root, data.get("train_mapping")), "val": (root, data.get("val_mapping"))}
    try:
        train_set, val_set = build_sets(cfg, roots)
        train_loader = torch.utils.data.DataLoader(train_set, batch_size=cfg["batch_size"], shuffle=True, pin_memory=True,
                                                   num_workers=args.num_workers)
        val_loader = torch.utils.data.DataLoader(val_set, batch_size=cfg["batch_size"], shuffle=False, pin_memory=True,
                                                 num_workers=args.num_workers)
        optimizer = make_optimizer(net.parameters(), lr=cfg["lr"], weight_decay=cfg["weight_decay"])
        lr_scheduler = LambdaLR(optimizer, lr_lambda=lambda it: schedule_factor(cfg, it * cfg["batch_size"]))
        bnm_scheduler = BNMomentumScheduler(net, bn_lambda=lambda it: norm_momentum(cfg, it * cfg["batch_size"]))
        trainer = Trainer(net, build_sup_criterion(cfg["loss"]), optimizer, cfg.get("ignore_npoint_thresh", 0),
                          checkpoint_dir(cfg, args.round), lr_scheduler=lr_scheduler, bnm_scheduler=bnm_scheduler, device=device,
                          max_iters=args.max_iters, log=lambda line: print(line, flush=True))
        return trainer.train(cfg["epochs"], train_loader, val_loader)
    finally:
        if tmp is not None:
            shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()

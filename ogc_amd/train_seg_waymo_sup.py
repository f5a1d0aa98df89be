"""Supervised segmentation training on single Waymo frames: the `OGC_sup` row of the Waymo table (counterpart of the
reference's train_seg_waymo_sup.py:19-297, a thin layer over ogc_amd/train_seg_sup.py).

    python -m ogc_amd.train_seg_waymo_sup config.yaml [--round R] [--synthetic N_SEQUENCES] [--max-iters K] [--data-root DIR]

What differs from train_seg_sup, as in the reference: the reader is WaymoSingleFrameDataset (ogc_amd/datasets.py) with
`ignore_class_ids = [2, 3]` (pedestrians, cyclists) and the config's `ignore_npoint_thresh` — the filtering happens THERE, so the
one-hot labels arrive with the ignored points zeroed and `valid` marks them for the loss; a batch is (pcs, segms, valids) with no
flows; the trainer's constructor has no threshold and the PQ / F1 / Pre / Rec it monitors are `accumulate_eval_results(segm,
mask)` at threshold 0 on `gt_mask.argmax(2)` (:107, :149) — through metrics.seg_eval on the GPU, as in train_seg_sup.  The
config is the reference's config/seg/waymo/waymo_sup.yaml (data.train_select_frame / val_select_frame name the json files of
sample ids).  Schedules, the NaN rule and the `current` / `best` checkpoints are train_seg_sup's.  `--synthetic N` writes N
training and max(N // 4, 1) validation sequences of synthetic single-frame Waymo data (utils/synthetic.py:
write_waymo_singleframe_roots) into a temporary root.  ogc_amd.test_seg_waymo evaluates the checkpoint.  Out of scope:
data-parallel training, HIP-graph replay.
"""
import argparse
import shutil
import tempfile

import numpy as np
import torch
import yaml

from . import train_seg_sup as _sup
from .train_seg import norm_momentum, schedule_factor
from .train_seg_sup import build_sup_criterion, checkpoint_dir
from .train_step import make_optimizer
from .utils.pytorch_util import BNMomentumScheduler, LambdaLR

IGNORE_CLASS_IDS = [2, 3]        # train_seg_waymo_sup.py:250
SYNTHETIC_FRAMES = 4             # frames per synthetic sequence


class Trainer(_sup.Trainer):
    """The reference's Trainer (train_seg_waymo_sup.py:19-198): train_seg_sup's without `ignore_npoint_thresh` (the monitored
    metrics use threshold 0) and on batches (pcs, segms, valids)."""

    def __init__(self, segnet, criterion, optimizer, exp_base, lr_scheduler=None, bnm_scheduler=None, **extras):
        super().__init__(segnet, criterion, optimizer, 0, exp_base, lr_scheduler=lr_scheduler, bnm_scheduler=bnm_scheduler, **extras)

    def _frame0(self, batch):
        pcs, segms, valids = batch
        return tuple(x[:, 0].contiguous().to(self.device, non_blocking=True) for x in (pcs, segms, valids))


def build_segnet(cfg):
    """models/segnet_kitti.py, whatever `dataset` says (train_seg_waymo_sup.py:238-247)."""
    from .models.segnet_kitti import MaskFormer3D
    seg = cfg["segnet"]
    return MaskFormer3D(n_slot=seg["n_slot"], n_point=seg["n_point"], use_xyz=seg["use_xyz"],
                        n_transformer_layer=seg["n_transformer_layer"], transformer_embed_dim=seg["transformer_embed_dim"],
                        transformer_input_pos_enc=seg["transformer_input_pos_enc"])


def build_sets(cfg, roots):
    """(train set, validation set) (train_seg_waymo_sup.py:249-270).  roots: {split: (data root, split file, select_frame json
    or None)}."""
    from .datasets import WaymoSingleFrameDataset
    data = cfg.get("data") or {}
    common = dict(downsampled=True, decentralize=bool(data.get("decentralize", False)), onehot_label=True,
                  max_n_object=cfg["segnet"]["n_slot"], ignore_class_ids=IGNORE_CLASS_IDS,
                  ignore_npoint_thresh=cfg.get("ignore_npoint_thresh", 0))
    (root, mapping, select), (vroot, vmapping, vselect) = roots["train"], roots["val"]
    train_set = WaymoSingleFrameDataset(data_root=root, mapping_path=mapping, select_frame=select,
                                        aug_transform=bool(data.get("aug_transform", False)),
                                        aug_transform_args=data.get("aug_transform_args"), **common)
    return train_set, WaymoSingleFrameDataset(data_root=vroot, mapping_path=vmapping, select_frame=vselect, **common)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("config")
    ap.add_argument("--round", type=int, default=0)
    ap.add_argument("--synthetic", type=int, default=0,
                    help="train on this many synthetic sequences written to a temporary root (utils/synthetic.py)")
    ap.add_argument("--max-iters", type=int, default=0, help="stop after this many optimisation steps (0 = all epochs)")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--data-root", default=None, help="the data set's root (default: data.root of the config)")
    ap.add_argument("--num_workers", type=int, default=4)
    args = ap.parse_args(argv)
    with open(args.config) as f:
        cfg = yaml.safe_load(f)
    if cfg["dataset"] != "waymo":
        raise KeyError("Unrecognized dataset %r (this is the Waymo trainer; see train_seg_sup for the others)" % (cfg["dataset"],))
    device = torch.device(args.device)
    np.random.seed(cfg["random_seed"])
    torch.manual_seed(cfg["random_seed"])
    if device.type == "cuda" and cfg.get("matmul_precision", "fp32") != "fp32":
        from .pointnet2 import pointnet2 as _api
        _api._native.set_matmul_precision(cfg["matmul_precision"])
    net = build_segnet(cfg).to(device)

    data, tmp = cfg.get("data") or {}, None
    if args.synthetic:
        from .utils.synthetic import write_waymo_singleframe_roots
        tmp = tempfile.mkdtemp(prefix="ogc_train_seg_waymo_sup_")
        made = write_waymo_singleframe_roots(tmp, args.synthetic, max(args.synthetic // 4, 1), SYNTHETIC_FRAMES,
                                             data.get("n_points", cfg["segnet"]["n_point"]))
        roots = {split: (tmp, made[split]["mapping"], None) for split in ("train", "val")}
    else:
        root = args.data_root or data["root"]
        roots = {split: (root, data[split + "_mapping"], data.get(split + "_select_frame")) for split in ("train", "val")}
    try:
        train_set, val_set = build_sets(cfg, roots)
        train_loader = torch.utils.data.DataLoader(train_set, batch_size=cfg["batch_size"], shuffle=True, pin_memory=True,
                                                   num_workers=args.num_workers)
        val_loader = torch.utils.data.DataLoader(val_set, batch_size=cfg["batch_size"], shuffle=False, pin_memory=True,
                                                 num_workers=args.num_workers)
        optimizer = make_optimizer(net.parameters(), lr=cfg["lr"], weight_decay=cfg["weight_decay"])
        lr_scheduler = LambdaLR(optimizer, lr_lambda=lambda it: schedule_factor(cfg, it * cfg["batch_size"]))
        bnm_scheduler = BNMomentumScheduler(net, bn_lambda=lambda it: norm_momentum(cfg, it * cfg["batch_size"]))
        trainer = Trainer(net, build_sup_criterion(cfg["loss"]), optimizer, checkpoint_dir(cfg, args.round),
                          lr_scheduler=lr_scheduler, bnm_scheduler=bnm_scheduler, device=device, max_iters=args.max_iters,
                          log=lambda line: print(line, flush=True))
        return trainer.train(cfg["epochs"], train_loader, val_loader)
    finally:
        if tmp is not None:
            shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()

"""Evaluation of a trained MaskFormer3D on a data set: the stage that produces the numbers people quote (counterpart of the
reference's test_seg.py:15-228 on this package's operators).

    python -m ogc_amd.test_seg CONFIG --split S [--round R] [--test_batch_size 64] [--curate_by_object T] [--save]
                               [--mapping FILE] [--synthetic N] [--num_workers 4]

`dataset` of the config is one of sapien, ogcdr, kittisf, kittidet, semantickitti — the last two are the single-frame sets a
KITTI-SF model is tested on for generalisation.  View selections, frames per scene, the ignore threshold (0 indoors, 50 points
outdoors), the checkpoint (`<save_path>[_R<round>]/best.pth.tar`) and the output directory (`<root>/segm_preds/OGC_R<round>`)
are the reference's (:32-122, :166-228).

`evaluate` is the loop body.  Per batch: the network, then `accumulate_seg_eval` (metrics/seg_eval.py) — one launch of
ogc_seg_eval, one of ogc_lsap_maximize and ONE small device->host copy, where the reference copies labels and soft masks to the
host and loops over (object, prediction) pairs in numpy and scipy — and, with `--save`, the kernel's hard labels go to
`_save_predsegm`: soft masks are never copied to the host.  It returns and prints AP / PQ / F1 / Pre / Rec @50 over all valid
predictions, and the mean over scenes of the per-scene mean and standard deviation of mIoU and RI over a scene's `n_frame`
samples, exactly as the reference averages them.

`--synthetic N` writes N labelled scenes into a temporary root (utils/synthetic.py::write_labelled_root: kittisf, kittidet,
semantickitti) and runs on those; the checkpoint is optional there (random weights when there is none).  Left out: `--visualize`
(needs open3d) and the Waymo script (test_seg_waymo.py calls `accumulate_eval_results` with a per-point tensor where its metrics
module takes an integer threshold: there is no reference behaviour to match).
"""
import argparse
import importlib
import json
import os
import shutil
import tempfile

import numpy as np
import torch
import yaml

from .metrics.seg_eval import accumulate_seg_eval, seg_eval_batch
from .metrics.seg_metric import calculate_AP, calculate_PQ_F1
from .utils.pytorch_util import AverageMeter

SEGNETS = {"sapien": "segnet_sapien", "ogcdr": "segnet_ogcdr", "kittisf": "segnet_kitti", "kittidet": "segnet_kitti",
           "semantickitti": "segnet_kitti"}
INDOOR_VIEW_SELS = [[0, 1], [1, 2], [2, 3], [3, 2]]
KITTISF_VIEW_SELS = [[0, 1], [1, 0]]
OUTDOOR_IGNORE_NPOINT_THRESH = 50
SEMANTICKITTI_SEQUENCES = list(range(11))


def evaluate(segnet, loader, n_frame, ignore_npoint_thresh, curate_by_object=0, saver=None, device="cuda"):
    """The reference's loop (test_seg.py:176-228).  segnet: any callable pc, pc -> (B, N, K) soft masks on the device; loader
    yields (pcs, segms, flows, valids) with the n_frame samples of a scene adjacent in one batch; a batch whose FIRST sample
    has at most `curate_by_object` objects is passed over; saver(hard (B, N) i32 device tensor, batch index) stores the
    predictions.  -> {'AP', 'PQ', 'F1', 'Pre', 'Rec', 'per_scan_iou_avg', 'per_scan_iou_std', 'per_scan_ri_avg',
    'per_scan_ri_std', 'n_batches', 'n_skipped'}."""
    meter = AverageMeter()
    pred_iou, pred_matched, confidence, n_gt_inst = [], [], [], 0
    n_batches = n_skipped = 0
    for i, batch in enumerate(loader):
        pcs, segms = batch[0], batch[1]
        segm = segms[:, 0].contiguous()
        if torch.unique(segm[0]).shape[0] <= curate_by_object:
            n_skipped += 1
            continue
        pc = pcs[:, 0].contiguous().to(device)
        segm = segm.to(device)
        if segm.shape[0] % n_frame != 0:
            raise ValueError("a batch of %d samples does not hold whole scenes of %d frames" % (segm.shape[0], n_frame))
        with torch.no_grad():
            mask = segnet(pc, pc)
        mask = mask.detach().float()
        result = seg_eval_batch(segm, mask, ignore_npoint_thresh)
        iou, matched, conf, n_gt, miou, ri = accumulate_seg_eval(segm, mask, ignore_npoint_thresh, result=result)
        pred_iou.append(iou)
        pred_matched.append(matched)
        confidence.append(conf)
        n_gt_inst += n_gt
        for sid in range(segm.shape[0] // n_frame):
            scan = slice(n_frame * sid, n_frame * (sid + 1))
            meter.append_loss({"per_scan_iou_avg": np.mean(miou[scan]), "per_scan_iou_std": np.std(miou[scan]),
                               "per_scan_ri_avg": np.mean(ri[scan]), "per_scan_ri_std": np.std(ri[scan])})
        if saver is not None:
            hard = result.hard
            if bool((result.status != 0).any()):    # labels beyond the kernel's table: its arg-max of that sample is zeroed
                hard = torch.where(result.status[:, None] != 0, mask.argmax(dim=2).to(torch.int32), hard)
            saver(hard, i)
        n_batches += 1
    if n_batches == 0:
        raise ValueError("no batch was evaluated (%d passed over by curate_by_object = %d)" % (n_skipped, curate_by_object))
    pred_iou, pred_matched, confidence = np.concatenate(pred_iou), np.concatenate(pred_matched), np.concatenate(confidence)
    pq, f1, pre, rec = calculate_PQ_F1(pred_iou, pred_matched, n_gt_inst)
    out = {"AP": float(calculate_AP(pred_matched, confidence, n_gt_inst)), "PQ": float(pq), "F1": float(f1), "Pre": float(pre),
           "Rec": float(rec)}
    out.update(meter.get_mean_loss_dict())
    out.update(n_batches=n_batches, n_skipped=n_skipped)
    return out


def build_segnet(cfg):
    seg = cfg["segnet"]
    MaskFormer3D = importlib.import_module("ogc_amd.models." + SEGNETS[cfg["dataset"]]).MaskFormer3D
    return MaskFormer3D(n_slot=seg["n_slot"], n_point=seg["n_point"], use_xyz=seg["use_xyz"],
                        n_transformer_layer=seg["n_transformer_layer"], transformer_embed_dim=seg["transformer_embed_dim"],
                        transformer_input_pos_enc=seg["transformer_input_pos_enc"])


def weight_path(cfg, round_):
    """<save_path>_R<round>/best.pth.tar, <save_path>/best.pth.tar for round 0 (test_seg.py:80-83)."""
    return os.path.join(cfg["save_path"] + ("_R%d" % round_ if round_ > 0 else ""), "best.pth.tar")


def build_test_set(cfg, split, data_root, mapping=None):
    """-> (data set, n_frame, ignore_npoint_thresh, data root as the data set sees it) (test_seg.py:32-65, :88-116)."""
    from . import datasets
    name = cfg["dataset"]
    data = cfg.get("data") or {}
    decentralize = bool(data.get("decentralize", False))
    if name in ("sapien", "ogcdr"):
        if name == "sapien":
            data_root = os.path.join(data_root, "mbs-sapien" if split == "test" else "mbs-shapepart")
        cls = datasets.SapienDataset if name == "sapien" else datasets.OGCDynamicRoomDataset
        return (cls(data_root=data_root, split=split, view_sels=INDOOR_VIEW_SELS, decentralize=decentralize),
                len(INDOOR_VIEW_SELS), 0, data_root)
    if name == "semantickitti":
        return (datasets.SemanticKITTIDataset(data_root=data_root, sequence_list=SEMANTICKITTI_SEQUENCES,
                                              decentralize=decentralize), 1, OUTDOOR_IGNORE_NPOINT_THRESH, data_root)
    if name not in ("kittisf", "kittidet"):
        raise KeyError("Unrecognized dataset %r" % name)
    if mapping is None:
        mapping = data.get("val_mapping" if split == "val" else "train_mapping") or os.path.join(data_root, split + ".txt")
    if name == "kittisf":
        return (datasets.KITTISceneFlowDataset(data_root=data_root, mapping_path=mapping, downsampled=True,
                                               view_sels=KITTISF_VIEW_SELS, decentralize=decentralize),
                len(KITTISF_VIEW_SELS), OUTDOOR_IGNORE_NPOINT_THRESH, data_root)
    return (datasets.KITTIDetectionDataset(data_root=data_root, mapping_path=mapping, decentralize=decentralize), 1,
            OUTDOOR_IGNORE_NPOINT_THRESH, data_root)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("config")
    ap.add_argument("--split", default="val", help="data set split")
    ap.add_argument("--round", type=int, default=0, help="trained segmentation model of which round")
    ap.add_argument("--test_batch_size", type=int, default=64)
    ap.add_argument("--curate_by_object", type=int, default=0,
                    help="test on the scenes with more objects than this (one scene per batch)")
    ap.add_argument("--save", action="store_true", help="write the predictions under <root>/segm_preds/OGC_R<round>")
    ap.add_argument("--mapping", default=None, help="kittisf, kittidet: the split file (default data.<split>_mapping, then "
                                                    "<data.root>/<split>.txt)")
    ap.add_argument("--synthetic", type=int, default=0, help="run on this many synthetic scenes in a temporary root")
    ap.add_argument("--num_workers", type=int, default=4)
    args = ap.parse_args(argv)
    with open(args.config) as f:
        cfg = yaml.safe_load(f)
    if cfg["dataset"] not in SEGNETS:
        raise KeyError("Unrecognized dataset %r" % cfg["dataset"])
    device = torch.device("cuda")
    data = cfg.get("data") or {}

    torch.manual_seed(cfg.get("random_seed", 10))
    segnet = build_segnet(cfg).to(device)
    path = weight_path(cfg, args.round)
    if os.path.isfile(path):
        segnet.load_state_dict(torch.load(path, map_location="cpu")["model_state"])
        print("Loaded weights from %s" % path, flush=True)
    elif args.synthetic:
        print("No checkpoint at %s: random weights" % path, flush=True)
    else:
        raise FileNotFoundError("no checkpoint at %s" % path)
    segnet.eval()

    tmp, mapping = None, args.mapping
    if args.synthetic:
        from .utils.synthetic import LABELLED_LAYOUTS, write_labelled_root
        if cfg["dataset"] not in LABELLED_LAYOUTS:
            raise KeyError("--synthetic covers %s, not %r" % (", ".join(LABELLED_LAYOUTS), cfg["dataset"]))
        tmp = tempfile.mkdtemp(prefix="ogc_test_seg_") if not data.get("root") else None
        data_root = tmp if tmp is not None else data["root"]
        mapping, _ = write_labelled_root(data_root, cfg["dataset"], args.synthetic, data.get("n_points", cfg["segnet"]["n_point"]),
                                         data.get("n_objects", 6), split=args.split)
    else:
        data_root = data["root"]
    test_set, n_frame, ignore_npoint_thresh, data_root = build_test_set(cfg, args.split, data_root, mapping)

    batch_size = n_frame if args.curate_by_object > 0 else args.test_batch_size   # one scene per batch when curating
    if batch_size % n_frame != 0:
        raise ValueError("Frames of one scene should be in the same batch: test_batch_size %d, %d frames" % (batch_size, n_frame))
    saver, save_dir = None, os.path.join(data_root, "segm_preds", "OGC_R%d" % args.round)
    if args.save:
        os.makedirs(save_dir, exist_ok=True)
        print("Save segmentation predictions into %s ..." % save_dir, flush=True)

        def saver(hard, i):
            test_set._save_predsegm(hard, save_root=save_dir, batch_size=batch_size, n_frame=n_frame, offset=i)
    loader = torch.utils.data.DataLoader(test_set, batch_size=batch_size, shuffle=False, pin_memory=True,
                                         num_workers=args.num_workers)
    metrics = evaluate(segnet, loader, n_frame, ignore_npoint_thresh, curate_by_object=args.curate_by_object, saver=saver,
                       device=device)
    print("Evaluation on %s-%s:" % (cfg["dataset"], args.split), flush=True)
    print("AveragePrecision@50: %s" % metrics["AP"], flush=True)
    print("PanopticQuality@50: %s F1-score@50: %s Prec@50: %s Recall@50: %s"
          % (metrics["PQ"], metrics["F1"], metrics["Pre"], metrics["Rec"]), flush=True)
    print(json.dumps({k: v for k, v in metrics.items() if k.startswith("per_scan") or k.startswith("n_")}), flush=True)
    if args.save:
        metrics["save_dir"] = save_dir
        print("Saved to %s" % save_dir, flush=True)
    if tmp is not None and not args.save:   # saved predictions stay where the line above says
        shutil.rmtree(tmp, ignore_errors=True)
    return metrics


if __name__ == "__main__":
    main()

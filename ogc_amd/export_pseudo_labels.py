"""Pseudo-labels for self-training: the segmentations a trained MaskFormer3D predicts on a single-frame set AND the confidence
of every object in them, in the files `KITTIDetectionDataset(load_prediction=, load_confidence=True)` reads back.

    python -m ogc_amd.export_pseudo_labels CONFIG [--split train] [--round R] [--test_batch_size 64] [--mapping FILE]
                                           [--num_workers 4]

`dataset` of the config is kittidet or semantickitti — the sets with one segm.npy per id, whose reader can load predictions
back; argparse refuses any other.  Network, checkpoint, data set, ignore threshold and the evaluation loop are test_seg's own
functions, so `<root>/segm_preds/OGC_R<round>/<id>/segm.npy` is what `test_seg --save` writes and the metrics returned and
printed are its metrics.  Beside it goes `<id>/conf.npy`: one float32 per distinct label, in ascending label order, the mean of
the object's own mask column over its own points — per batch one launch of ogc_slot_confidence (metrics/seg_conf.py) on the
masks already on the device.  The reference reads that file (`load_confidence`, datasets/dataset_kittidet.py:63-70) and has no
writer of it.

This is a driver of its own, not a flag of test_seg, because test_seg.py is not edited: its `evaluate` hands a saver the hard
labels only, so the masks reach the saver through the network callable `evaluate` is given.  That pairing is checked, not
assumed: nothing is written unless the arg-max the kernel takes of the kept masks equals the hard labels handed over.
"""
import argparse
import os

import torch
import yaml

from . import test_seg
from .metrics.seg_conf import confidences_to_host, slot_confidence_batch

DATASETS = ("kittidet", "semantickitti")   # single-frame sets: one conf.npy beside the one segm.npy of an id


def export(segnet, test_set, loader, ignore_npoint_thresh, save_dir, batch_size, device="cuda"):
    """test_seg.evaluate over `loader` with a saver that writes <save_dir>/<id>/{segm,conf}.npy for every sample -> its metrics."""
    kept = []   # the masks of the batch in flight

    def network(pc1, pc2):
        mask = segnet(pc1, pc2)
        kept.append(mask)
        return mask

    def saver(hard, i):
        if len(kept) != 1:
            raise RuntimeError("batch %d: %d network calls since the last saved batch, expected one" % (i, len(kept)))
        res = slot_confidence_batch(kept.pop().detach().float())
        if res.hard.shape != hard.shape or not torch.equal(res.hard, hard.to(torch.int32)):
            raise RuntimeError("batch %d: the labels to be saved are not the arg-max of the masks the confidences come from" % i)
        test_set._save_predsegm(hard, save_root=save_dir, batch_size=batch_size, n_frame=1, offset=i,
                                conf=confidences_to_host(res))

    return test_seg.evaluate(network, loader, 1, ignore_npoint_thresh, saver=saver, device=device)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("config")
    ap.add_argument("--split", default="train", help="data set split")
    ap.add_argument("--round", type=int, default=0, help="trained segmentation model of which round")
    ap.add_argument("--test_batch_size", type=int, default=64)
    ap.add_argument("--mapping", default=None, help="kittidet: the split file (default data.<split>_mapping, then "
                                                    "<data.root>/<split>.txt)")
    ap.add_argument("--num_workers", type=int, default=4)
    args = ap.parse_args(argv)
    with open(args.config) as f:
        cfg = yaml.safe_load(f)
    if cfg["dataset"] not in DATASETS:
        ap.error("pseudo-labels are exported for %s, not %r" % (", ".join(DATASETS), cfg["dataset"]))
    device = torch.device("cuda")

    torch.manual_seed(cfg.get("random_seed", 10))
    segnet = test_seg.build_segnet(cfg).to(device)
    path = test_seg.weight_path(cfg, args.round)
    segnet.load_state_dict(torch.load(path, map_location="cpu")["model_state"])
    segnet.eval()
    test_set, _, ignore_npoint_thresh, data_root = test_seg.build_test_set(cfg, args.split, cfg["data"]["root"], args.mapping)
    save_dir = os.path.join(data_root, "segm_preds", "OGC_R%d" % args.round)
    os.makedirs(save_dir, exist_ok=True)
    loader = torch.utils.data.DataLoader(test_set, batch_size=args.test_batch_size, shuffle=False, pin_memory=True,
                                         num_workers=args.num_workers)
    metrics = export(segnet, test_set, loader, ignore_npoint_thresh, save_dir, args.test_batch_size, device=device)
    print("Evaluation on %s-%s: AP@50 %s PQ@50 %s F1@50 %s" % (cfg["dataset"], args.split, metrics["AP"], metrics["PQ"], metrics["F1"]),
          flush=True)
    metrics["save_dir"] = save_dir
    print("Saved labels and confidences to %s" % save_dir, flush=True)
    return metrics


if __name__ == "__main__":
    main()

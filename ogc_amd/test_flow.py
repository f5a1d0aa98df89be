"""Scene-flow prediction on SAPIEN and OGC-DR: the stage between a trained FlowStep3D and the first segmentation round on the two
four-frame data sets (counterpart of the reference's test_flow.py:30-105 on this package's operators).

    python -m ogc_amd.test_flow CONFIG --split S [--test_batch_size 48] [--test_model_iters 4] [--save] [--synthetic N]

The network runs over every ordered frame pair `VIEW_SELS` of every scene of the split; the last of its iterative predictions
is evaluated against the flow the data set computes from the objects' motions (`epe_norm_thresh` 0.01, as the reference sets for
both data sets) with ogc_amd.metrics.flow_eval: one launch of ogc_flow_eval and one (B, 4) device->host copy per batch, where
the reference copies both flow tensors to the host.  As in the reference the four batch values are appended to an AverageMeter,
so a smaller last batch weighs as much as a full one.  With `--save` the predictions go to
<root>/flow_preds/flowstep3d/<id>.npy (6, N, 3) with <root>/flow_preds/flowstep3d.json {"view_sel": [...]} — one device->host
copy per batch — which SapienDataset / OGCDynamicRoomDataset(predflow_path='flowstep3d') read back for `train_seg` and
`oa_icp_round`; the six pairs of a scene must then share a batch (test_batch_size % 6 == 0).

Config: the reference's flow schema (config/flow/{sapien,ogcdr}/*.yaml): dataset, save_path (the directory train_flow wrote
best.pth.tar into), data.root, flownet{...}.  For `sapien` the root is <data.root>/mbs-sapien for the split `test` and
<data.root>/mbs-shapepart otherwise.  `--synthetic N` writes N four-frame scenes in the data set's layout into a temporary root
(utils/synthetic.py) and runs on those; the checkpoint is optional there (random weights when save_path holds none).
`main` returns the metric dictionary.
"""
import argparse
import importlib
import json
import os
import shutil
import tempfile

import torch
import yaml

from .metrics.flow_eval import eval_flow_device
from .test_flow_kittisf import load_weights
from .utils.pytorch_util import AverageMeter

FLOWNETS = {"sapien": "flownet_sapien", "ogcdr": "flownet_ogcdr"}
VIEW_SELS = [[0, 1], [1, 0], [1, 2], [2, 1], [2, 3], [3, 2]]
EPE_NORM_THRESH = 0.01
PREDFLOW_NAME = "flowstep3d"


def evaluate(flownet, loader, device, epe_norm_thresh, iters, on_batch=None):
    """The reference's loop body (test_flow.py:85-101).  flownet: any callable (pc1, pc2, feat1, feat2, iters=) -> list of
    (B, N, 3) predictions on the device; loader yields (pcs, segms, flows, valids); on_batch(i, flow_pred) sees the evaluated
    prediction of batch i, a device tensor.  -> {'EPE', 'AccS', 'AccR', 'Outlier'}: means over the batches."""
    meter = AverageMeter()
    for i, batch in enumerate(loader):
        pcs, flows = batch[0], batch[2]
        pc1, pc2 = pcs[:, 0].contiguous().to(device), pcs[:, 1].contiguous().to(device)
        flow = flows[:, 0].contiguous().to(device)
        with torch.no_grad():
            flow_pred = flownet(pc1, pc2, pc1, pc2, iters=iters)[-1].detach()
        (epe, acc_strict, acc_relax, outlier), _ = eval_flow_device(flow, flow_pred, epe_norm_thresh=epe_norm_thresh)
        meter.append_loss({"EPE": epe, "AccS": acc_strict, "AccR": acc_relax, "Outlier": outlier})
        if on_batch is not None:
            on_batch(i, flow_pred)
    return meter.get_mean_loss_dict()


def build_test_set(dataset, split, data_root, predflow_path=None):
    """-> (data set over VIEW_SELS, the data root as the data set sees it) (test_flow.py:31-45, :61-64)."""
    from . import datasets
    if dataset == "sapien":
        data_root = os.path.join(data_root, "mbs-sapien" if split == "test" else "mbs-shapepart")
        cls = datasets.SapienDataset
    elif dataset == "ogcdr":
        cls = datasets.OGCDynamicRoomDataset
    else:
        raise KeyError("Unrecognized dataset %r" % dataset)
    return cls(data_root=data_root, split=split, view_sels=VIEW_SELS, predflow_path=predflow_path), data_root


def main(argv=None, on_batch=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("config")
    ap.add_argument("--split", default="val", help="data set split")
    ap.add_argument("--test_batch_size", type=int, default=48)
    ap.add_argument("--test_model_iters", type=int, default=4, help="FlowStep3D unrolling iterations")
    ap.add_argument("--save", action="store_true", help="write the predicted flows under <root>/flow_preds/flowstep3d")
    ap.add_argument("--synthetic", type=int, default=0, help="run on this many synthetic scenes in a temporary root")
    ap.add_argument("--num_workers", type=int, default=4)
    args = ap.parse_args(argv)
    with open(args.config) as f:
        cfg = yaml.safe_load(f)
    dataset = cfg["dataset"]
    if dataset not in FLOWNETS:
        raise KeyError("Unrecognized dataset %r" % dataset)
    n_frame, batch_size = len(VIEW_SELS), args.test_batch_size
    if args.save and batch_size % n_frame != 0:
        raise ValueError("--save needs the %d frame pairs of a scene in one batch: test_batch_size %d is no multiple of %d"
                         % (n_frame, batch_size, n_frame))
    device = torch.device("cuda")
    data = cfg.get("data") or {}

    fl = cfg["flownet"]
    FlowStep3D = importlib.import_module("ogc_amd.models." + FLOWNETS[dataset]).FlowStep3D
    torch.manual_seed(cfg.get("random_seed", 10))
    flownet = FlowStep3D(npoint=fl["npoint"], use_instance_norm=fl["use_instance_norm"], loc_flow_nn=fl["loc_flow_nn"],
                         loc_flow_rad=fl["loc_flow_rad"], k_decay_fact=0.5).to(device)
    loaded = load_weights(flownet, os.path.join(cfg["save_path"], "best.pth.tar"), required=not args.synthetic)
    flownet.eval()
    print("Loaded weights from %s" % loaded if loaded else "No checkpoint at %s: random weights" % cfg["save_path"], flush=True)

    tmp = None
    if args.synthetic:
        from .utils.synthetic import write_ogcdr_root, write_sapien_root
        tmp = tempfile.mkdtemp(prefix="ogc_test_flow_") if not data.get("root") else None
        data_root = tmp if tmp is not None else data["root"]
        n_points = data.get("n_points", fl["npoint"])
        if dataset == "sapien":
            write_sapien_root(os.path.join(data_root, "mbs-sapien" if args.split == "test" else "mbs-shapepart"), args.synthetic,
                              n_points, split=args.split)
        else:
            write_ogcdr_root(data_root, args.synthetic, n_points, split=args.split)
    else:
        data_root = data["root"]
    test_set, data_root = build_test_set(dataset, args.split, data_root)

    save_dir = os.path.join(data_root, "flow_preds", PREDFLOW_NAME)
    callbacks = [on_batch] if on_batch is not None else []
    if args.save:
        from .utils import flow_store
        os.makedirs(save_dir, exist_ok=True)
        flow_store.write_meta(save_dir, VIEW_SELS)

        def save(i, flow_pred):     # the data sets' writers make the one copy to the host
            test_set._save_predflow(flow_pred, save_root=save_dir, batch_size=batch_size, n_frame=n_frame, offset=i)
        callbacks.append(save)

    def each(i, flow_pred):
        for fn in callbacks:
            fn(i, flow_pred)
    loader = torch.utils.data.DataLoader(test_set, batch_size=batch_size, shuffle=False, pin_memory=True,
                                         num_workers=args.num_workers)
    metrics = evaluate(flownet, loader, device, EPE_NORM_THRESH, args.test_model_iters, on_batch=each if callbacks else None)
    print("Evaluation on %s-%s: %s" % (dataset, args.split, metrics), flush=True)
    if args.save:
        metrics["save_dir"] = save_dir
        print("Saved to %s" % save_dir, flush=True)
    if tmp is not None and not args.save:   # saved flows stay where the line above says
        shutil.rmtree(tmp, ignore_errors=True)
    return metrics


if __name__ == "__main__":
    main()

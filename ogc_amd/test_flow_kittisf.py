"""Scene-flow prediction on the full-resolution KITTI-SF scans: the stage that produces the flows the unsupervised segmentation
training starts from (counterpart of the reference's test_flow_kittisf.py:17-142 on this package's operators).

    python -m ogc_amd.test_flow_kittisf CONFIG --split {train,val} [--test_model_iters 4] [--save] [--synthetic N]

Per scene pair, in both directions (`view_sels = [[0, 1], [1, 0]]`), `predict_pair` does what the reference's loop body does
(:84-127), with its constants: points with y < -1.4 in BOTH frames are ground; the rest is centred (ICP only) and down-sampled
to `n_point_icp = 1024` points per frame with FPS; the camera's ego-motion is fitted with point-to-point ICP (50 iterations at
most, utils/icp_util.py -> ogc_rigid_icp); that transform, applied to the WHOLE first frame, is the ground's flow and the base
of everybody else's; the above-ground points, moved by it, go through FlowStep3D at `flownet.npoint` points and the predicted
residual flow is up-sampled with three-NN and added.  As in the reference the transform fitted on the centred clouds is
applied to the un-centred ones (:104-111).  The clouds stay on the device between the stages — the reference goes back to numpy
after every one; what the host sees is the scene on the way in, the number of above-ground points (a shape) and the flow on the
way out.  When fewer than `n_point_icp` points remain above the ground, all of them are used (the reference fails there).

`main` loops over the data set (KITTISceneFlowDataset, downsampled=False), evaluates against pc2 - pc1 (`eval_flow`,
epe_norm_thresh 0.05) and with `--save` writes <root>/flow_preds/flowstep3d/<id>/flow{1,2}.npy, which
KITTISceneFlowDataset(predflow_path='flowstep3d') reads back for `train_seg` and `oa_icp_round`.  It returns the mean
EPE / AccS / AccR / Outlier.

Config: the reference's schema (config/flow/kittisf/kittisf_unsup.yaml): save_path (a checkpoint file — {'state_dict': ...} with
the trainer's 'model.' prefix as the reference stores it, or this package's {'model_state': ...} — or a directory holding
best.pth.tar), data.root, flownet{...}.  The split file is `--mapping`, by default <data.root>/<split>.txt.
`--synthetic N` writes N small scenes in the "processed" layout into a temporary root (utils/synthetic.py) and runs on those; the
checkpoint is optional there (random weights when save_path holds none).
"""
import argparse
import json
import os
import shutil
import tempfile
from collections import OrderedDict

import torch
import yaml

from .datasets import KITTISceneFlowDataset
from .metrics.flow_metric import eval_flow
from .pointnet2.pointnet2 import furthest_point_sample
from .utils.data_util import upsample_feat
from .utils.icp_util import icp_batch, rigid_apply, rigid_flow
from .utils.pytorch_util import AverageMeter

GROUND_Y = -1.4
VIEW_SELS = [[0, 1], [1, 0]]
EPE_NORM_THRESH = 0.05


def _fps_points(pc, n_sample):
    """pc (M, 3) -> its min(n_sample, M) FPS samples (1, n, 3)."""
    idx = furthest_point_sample(pc[None].contiguous(), min(n_sample, pc.shape[0]))
    return pc[idx[0].long()][None].contiguous()


def predict_pair(flownet, pc1_org, pc2_org, n_point_icp=1024, max_icp_iters=50, iters=4, npoint=None):
    """pc1_org, pc2_org (N, 3) fp32 CUDA tensors, points in correspondence -> the flow of frame 1, (N, 3) fp32, on the device.
    npoint: points per frame given to the network (default: what `flownet` was built for)."""
    if npoint is None:
        npoint = 2 * flownet.encoder_loc.sa1.npoint
    with torch.no_grad():
        not_ground = torch.logical_not(torch.logical_and(pc1_org[:, 1] < GROUND_Y, pc2_org[:, 1] < GROUND_Y))
        pc1, pc2 = pc1_org[not_ground], pc2_org[not_ground]
        # ego-motion of the camera: ICP between FPS samples of the centred above-ground points
        center = torch.cat([pc1, pc2], 0).mean(0)
        T, _, _ = icp_batch(_fps_points(pc1 - center, n_point_icp), _fps_points(pc2 - center, n_point_icp),
                            max_iterations=max_icp_iters)
        flow_org = rigid_flow(pc1_org, T[0])
        # residual flow of the above-ground points after that motion, from the network
        pc1 = rigid_apply(pc1, T[0])
        pc1_fps, pc2_fps = _fps_points(pc1, npoint), _fps_points(pc2, npoint)
        flow_fps = flownet(pc1_fps, pc2_fps, pc1_fps, pc2_fps, iters=iters)[-1].detach()
        flow_org[not_ground] += upsample_feat(pc1[None], pc1_fps, flow_fps)[0]
    return flow_org


def load_weights(flownet, path, required=True):
    if os.path.isdir(path):
        path = os.path.join(path, "best.pth.tar")
    if not os.path.isfile(path):
        if required:
            raise FileNotFoundError("no checkpoint at %s" % path)
        return None
    stored = torch.load(path, map_location="cpu")
    if "state_dict" in stored:      # the reference's trainer wraps the network as `model` (test_flow_kittisf.py:42-44)
        weights = OrderedDict((k[6:], v) for k, v in stored["state_dict"].items())
    else:
        weights = stored["model_state"]
    flownet.load_state_dict(weights)
    return path


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("config")
    ap.add_argument("--split", choices=("train", "val"), default="val")
    ap.add_argument("--test_model_iters", type=int, default=4, help="FlowStep3D unrolling iterations")
    ap.add_argument("--save", action="store_true", help="write the predicted flows under <root>/flow_preds/flowstep3d")
    ap.add_argument("--synthetic", type=int, default=0, help="run on this many synthetic scenes in a temporary root")
    ap.add_argument("--mapping", default=None, help="the split file listing the scene ids (default <data.root>/<split>.txt)")
    ap.add_argument("--n_point_icp", type=int, default=1024)
    ap.add_argument("--max_icp_iters", type=int, default=50)
    args = ap.parse_args(argv)
    with open(args.config) as f:
        cfg = yaml.safe_load(f)
    device = torch.device("cuda")

    from .models.flownet_kitti import FlowStep3D
    fl = cfg["flownet"]
    torch.manual_seed(cfg.get("random_seed", 10))
    flownet = FlowStep3D(npoint=fl["npoint"], use_instance_norm=fl["use_instance_norm"], loc_flow_nn=fl["loc_flow_nn"],
                         loc_flow_rad=fl["loc_flow_rad"], k_decay_fact=0.5).to(device)
    loaded = load_weights(flownet, cfg["save_path"], required=not args.synthetic)
    flownet.eval()
    print("Loaded weights from %s" % loaded if loaded else "No checkpoint at %s: random weights" % cfg["save_path"], flush=True)

    tmp = None
    if args.synthetic:
        from .utils.synthetic import write_kitti_processed_root
        data_cfg = cfg.get("data") or {}
        tmp = tempfile.mkdtemp(prefix="ogc_kittisf_") if not data_cfg.get("root") else None
        data_root = tmp if tmp is not None else data_cfg["root"]
        mapping, _ = write_kitti_processed_root(data_root, args.synthetic, data_cfg.get("n_points", 4096), split=args.split)
    else:
        data_root = cfg["data"]["root"]
        mapping = args.mapping or os.path.join(data_root, args.split + ".txt")
    test_set = KITTISceneFlowDataset(data_root=data_root, mapping_path=mapping, downsampled=False, view_sels=VIEW_SELS)
    save_dir = os.path.join(data_root, "flow_preds", "flowstep3d")
    if args.save:
        os.makedirs(save_dir, exist_ok=True)

    meter = AverageMeter()
    for sid in range(len(test_set)):
        pcs, _, flows, _ = test_set[sid]
        pc1_org, pc2_org = torch.from_numpy(pcs[0]).to(device), torch.from_numpy(pcs[1]).to(device)
        flow_pred = predict_pair(flownet, pc1_org, pc2_org, n_point_icp=args.n_point_icp, max_icp_iters=args.max_icp_iters,
                                 iters=args.test_model_iters, npoint=fl["npoint"])[None]
        epe, acc_strict, acc_relax, outlier = eval_flow(torch.from_numpy(flows[0])[None].to(device), flow_pred,
                                                        epe_norm_thresh=EPE_NORM_THRESH)
        meter.append_loss({"EPE": epe, "AccS": acc_strict, "AccR": acc_relax, "Outlier": outlier})
        if args.save:
            test_set._save_predflow(flow_pred, save_root=save_dir, batch_size=1, n_frame=len(VIEW_SELS), offset=sid)
    metrics = meter.get_mean_loss_dict()
    print("Evaluation on kittisf-%s: %s" % (args.split, json.dumps({k: round(v, 5) for k, v in metrics.items()})), flush=True)
    if args.save:
        print("Saved to %s" % save_dir, flush=True)
    if tmp is not None and not args.save:   # saved flows stay where the line above says
        shutil.rmtree(tmp, ignore_errors=True)
    return metrics


if __name__ == "__main__":
    main()

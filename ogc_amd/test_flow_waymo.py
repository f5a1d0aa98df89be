"""Scene-flow prediction on the full-resolution Waymo scans: the stage that produces the flows round 1 of the unsupervised
segmentation training on Waymo starts from (counterpart of the reference's test_flow_waymo.py:18-318 on this package's operators).

    python -m ogc_amd.test_flow_waymo CONFIG --split {train,val} [--use_odometry] [--denoise] [--bound]
                                             [--test_model_iters 4] [--save] [--synthetic N]

Per sample (frame t towards frame t - 1; the frames are not in correspondence and differ in size) `predict_pair` does what the
reference's loop body does (:139-308), with its constants:
  ground      a point is ground when y < 0.3 OR it lies within 0.4 m of the plane fitted to `n_point_gpf = 2048` FPS samples of its
              frame (utils/gpf_util.py -> ogc_ground_plane_fit: seed from the 50 lowest samples, 5 fits).  Both frames are fitted in
              ONE launch when both have at least `n_point_gpf` points, otherwise in one launch each.
  ego-motion  from the two sensor poses with `--use_odometry` (`ego_motion_from_poses`), otherwise point-to-point ICP (50
              iterations at most, utils/icp_util.py -> ogc_rigid_icp) between `n_point_icp = 1024` FPS samples per frame of the
              centred above-ground points.  That transform, applied to the WHOLE first frame, is the ground's flow and the base of
              everybody else's.
  bounding    `register_bound`: with `--bound` only points that land in the front view of the other frame (z > |x|, range < 60 m,
              |x| < 50 m, z < 35 m) go to the network — forward for frame 1, with the inverse transform for frame 2.  As in the
              reference the test moves the points it is given, and frame 1 arrives already moved (:225-229).
  network     the selected above-ground points, frame 1 moved by the ego-motion, go through FlowStep3D at `flownet.npoint` FPS
              samples; the residual flow is up-sampled with three-NN, with `--denoise` zeroed where its norm exceeds 2.5 m, and
              scattered back through the bound mask and the not-ground mask onto the rigid flow.
The clouds stay on the device between the stages — the reference goes back to numpy after every one; what the host sees is the
scene on the way in, the numbers of selected points (shapes) and the flow on the way out.  Degenerate scenes: an empty frame
gives a zero flow of frame 1's shape and launches nothing; when nothing is left after ground removal and bounding the result
is the rigid flow alone; when fewer points than a sample size remain, all of them are used (ICP: the smaller frame's number for
both, identity below 3 points); a frame with no more than `n_gpf_lpr` points gets no plane, as the reference ends up giving it.

`main` loops over the data set (WaymoOpenDataset, downsampled=False), evaluates against the stored backward flow (`eval_flow`,
epe_norm_thresh 0.05) over all points, the ground points and the above-ground points, prints the three dictionaries and returns
the first.  With `--save` it writes <root>/flow_preds/flowstep3d_gpf[_odo][_bound][_denoise]/<sequence>/flow_%04d_%04d.npy, which
WaymoOpenDataset(predflow_path=...) reads back.

Config: the reference's schema (config/flow/waymo/waymo_unsup.yaml): save_path, data.root, flownet{...}; checkpoints as in
test_flow_kittisf.  The split file is `--mapping`, by default <data.root>/<split>.txt.  `--synthetic N` writes N small sequences
(utils/synthetic.py::write_waymo_root) into a temporary root and runs on those; the checkpoint is optional there.
"""
import argparse
import json
import os
import shutil
import tempfile

import numpy as np
import torch
import yaml

from .datasets import WaymoOpenDataset
from .metrics.flow_metric import eval_flow
from .test_flow_kittisf import _fps_points, load_weights
from .utils.data_util import upsample_feat
from .utils.gpf_util import ground_plane_fit_batch, plane_mask
from .utils.icp_util import icp_batch, rigid_apply, rigid_flow
from .utils.pytorch_util import AverageMeter

GROUND_Y = 0.3
EPE_NORM_THRESH = 0.05
THRESH_FLOW_NORM = 2.5
SAVE_NAME = "flowstep3d_gpf"


def ego_motion_from_poses(pose1, pose2):
    """Sensor-to-world poses (4, 4) of frame 1 and frame 2 -> the (4, 4) float64 tensor that takes frame-1 coordinates to
    frame-2 coordinates for a static world: rot2^T rot1, rot2^T (t1 - t2) (test_flow_waymo.py:189-196)."""
    pose1, pose2 = torch.as_tensor(pose1, dtype=torch.float64), torch.as_tensor(pose2, dtype=torch.float64)
    T = torch.eye(4, dtype=torch.float64, device=pose1.device)
    T[:3, :3] = pose2[:3, :3].T @ pose1[:3, :3]
    T[:3, 3] = pose2[:3, :3].T @ (pose1[:3, 3] - pose2[:3, 3])
    return T


def register_bound(pc1, pc2, rot, transl, bound=True):
    """Which points of pc1 (N, 3), moved by rot (3, 3), transl (3,) in float64, land inside the other frame's field of view
    (test_flow_waymo.py:18-46) -> (N,) bool on pc1's device; all True without `bound`.  pc2 is not looked at (the reference's
    bounding-box variant is commented out)."""
    if not bound:
        return torch.ones(pc1.shape[0], dtype=torch.bool, device=pc1.device)
    rot = torch.as_tensor(rot, dtype=torch.float64, device=pc1.device)
    transl = torch.as_tensor(transl, dtype=torch.float64, device=pc1.device)
    moved = pc1.to(torch.float64) @ rot.T + transl
    x, z = moved[:, 0], moved[:, 2]
    return (z > x.abs()) & (moved.square().sum(1) < 60.0 * 60.0) & (x.abs() < 50.0) & (z < 35.0)


def ground_masks(pc1_org, pc2_org, n_point_gpf=2048, n_gpf_iter=5, n_gpf_lpr=50, thresh_seed=0.4, thresh_dist=0.4):
    """The ground labels of both frames, [(N1,) bool, (N2,) bool]: the height threshold OR the fitted plane (:157-174)."""
    frames = (pc1_org, pc2_org)
    kw = dict(n_iter=n_gpf_iter, n_lpr=n_gpf_lpr, thresh_seed=thresh_seed, thresh_dist=thresh_dist)
    fit = [pc.shape[0] >= 3 and pc.shape[0] > n_gpf_lpr for pc in frames]
    if all(fit) and min(pc.shape[0] for pc in frames) >= n_point_gpf:
        planes = ground_plane_fit_batch(torch.cat([_fps_points(pc, n_point_gpf) for pc in frames], 0), **kw)[0]
    else:
        planes = [ground_plane_fit_batch(_fps_points(pc, n_point_gpf), **kw)[0][0] if ok else None for pc, ok in zip(frames, fit)]
    masks = []
    for pc, plane in zip(frames, planes):
        by_height = pc[:, 1] < GROUND_Y
        masks.append(by_height if plane is None else torch.logical_or(by_height, plane_mask(pc, plane, thresh_dist)))
    return masks


def predict_pair(flownet, pc1_org, pc2_org, pose=None, bound=False, denoise=False, n_point_gpf=2048, n_gpf_iter=5, n_gpf_lpr=50,
                 thresh_seed=0.4, thresh_dist=0.4, n_point_icp=1024, max_icp_iters=50, iters=4, npoint=None, return_ground=False):
    """pc1_org (N1, 3), pc2_org (N2, 3) fp32 CUDA tensors -> the flow of frame 1 towards frame 2, (N1, 3) fp32, on the device
    (with `return_ground` also frame 1's ground mask, (N1,) bool).  pose: None, or the two sensor poses (pose1, pose2) to take
    the ego-motion from.  npoint: points per frame given to the network (default: what `flownet` was built for)."""
    with torch.no_grad():
        if min(pc1_org.shape[0], pc2_org.shape[0]) < 1:       # an empty frame: nothing to launch on
            flow_org = torch.zeros_like(pc1_org)
            return (flow_org, torch.zeros(pc1_org.shape[0], dtype=torch.bool, device=pc1_org.device)) if return_ground else flow_org
        if npoint is None:
            npoint = 2 * flownet.encoder_loc.sa1.npoint
        is_ground1, is_ground2 = ground_masks(pc1_org, pc2_org, n_point_gpf, n_gpf_iter, n_gpf_lpr, thresh_seed, thresh_dist)
        not_ground1 = torch.logical_not(is_ground1)
        pc1, pc2 = pc1_org[not_ground1], pc2_org[torch.logical_not(is_ground2)]
        if pose is not None:
            T = ego_motion_from_poses(*pose).to(pc1_org.device)
        else:
            n_icp = min(n_point_icp, pc1.shape[0], pc2.shape[0])
            if n_icp >= 3:   # ICP between FPS samples of the centred above-ground points
                center = torch.cat([pc1, pc2], 0).mean(0)
                T = icp_batch(_fps_points(pc1 - center, n_icp), _fps_points(pc2 - center, n_icp), max_iterations=max_icp_iters)[0][0]
            else:
                T = torch.eye(4, dtype=torch.float64, device=pc1_org.device)
        flow_org = rigid_flow(pc1_org, T)
        # residual flow of the above-ground points that both frames see, after that motion, from the network
        pc1 = rigid_apply(pc1, T)
        rot, transl = T[:3, :3], T[:3, 3]
        select1 = register_bound(pc1, pc2, rot, transl, bound)
        pc1_sel = pc1[select1]
        select2 = register_bound(pc2, pc1_sel, rot.T, -(rot.T @ transl), bound)
        pc2_sel = pc2[select2]
        if min(pc1_sel.shape[0], pc2_sel.shape[0]) > 0:
            pc1_fps, pc2_fps = _fps_points(pc1_sel, npoint), _fps_points(pc2_sel, npoint)
            flow_fps = flownet(pc1_fps, pc2_fps, pc1_fps, pc2_fps, iters=iters)[-1].detach()
            flow_sel = upsample_feat(pc1_sel[None].contiguous(), pc1_fps, flow_fps)[0]
            if denoise:
                flow_sel = torch.where(flow_sel.norm(dim=1, keepdim=True) > THRESH_FLOW_NORM, torch.zeros_like(flow_sel), flow_sel)
            flow = torch.zeros_like(pc1)
            flow[select1] = flow_sel
            flow_org[not_ground1] += flow
    return (flow_org, is_ground1) if return_ground else flow_org


def save_name(use_odometry=False, bound=False, denoise=False):
    return SAVE_NAME + ("_odo" if use_odometry else "") + ("_bound" if bound else "") + ("_denoise" if denoise else "")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("config")
    ap.add_argument("--split", choices=("train", "val"), default="val")
    ap.add_argument("--use_odometry", action="store_true", help="take the ego-motion from the stored sensor poses, not from ICP")
    ap.add_argument("--denoise", action="store_true", help="zero predicted residual flows longer than 2.5 m")
    ap.add_argument("--bound", action="store_true", help="give the network only points inside the other frame's field of view")
    ap.add_argument("--test_model_iters", type=int, default=4, help="FlowStep3D unrolling iterations")
    ap.add_argument("--save", action="store_true", help="write the predicted flows under <root>/flow_preds/flowstep3d_gpf...")
    ap.add_argument("--synthetic", type=int, default=0, help="run on this many synthetic sequences in a temporary root")
    ap.add_argument("--mapping", default=None, help="the split file listing the sequences (default <data.root>/<split>.txt)")
    ap.add_argument("--n_point_gpf", type=int, default=2048)
    ap.add_argument("--n_gpf_lpr", type=int, default=50)
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
        from .utils.synthetic import write_waymo_root
        data_cfg = cfg.get("data") or {}
        tmp = tempfile.mkdtemp(prefix="ogc_waymo_") if not data_cfg.get("root") else None
        data_root = tmp if tmp is not None else data_cfg["root"]
        mapping, _ = write_waymo_root(data_root, args.synthetic, data_cfg.get("n_frames", 3), data_cfg.get("n_points", 8192),
                                      split=args.split)
    else:
        data_root = cfg["data"]["root"]
        mapping = args.mapping or os.path.join(data_root, args.split + ".txt")
    test_set = WaymoOpenDataset(data_root=data_root, mapping_path=mapping, downsampled=False)
    save_dir = os.path.join(data_root, "flow_preds", save_name(args.use_odometry, args.bound, args.denoise))
    if args.save:
        os.makedirs(save_dir, exist_ok=True)

    meters = {"all": AverageMeter(), "ground": AverageMeter(), "above": AverageMeter()}
    for sid in range(len(test_set)):
        name, view1, view2 = test_set.data_ids[sid]
        pcs, _, flows, _ = test_set[sid]
        pc1_org, pc2_org = torch.from_numpy(pcs[0]).to(device), torch.from_numpy(pcs[1]).to(device)
        pose = None
        if args.use_odometry:
            pose = [np.load(os.path.join(data_root, "data", name, "pose_%04d.npy" % v)) for v in (view1, view2)]
        flow_pred, is_ground = predict_pair(flownet, pc1_org, pc2_org, pose=pose, bound=args.bound, denoise=args.denoise,
                                            n_point_gpf=args.n_point_gpf, n_gpf_lpr=args.n_gpf_lpr, n_point_icp=args.n_point_icp,
                                            max_icp_iters=args.max_icp_iters, iters=args.test_model_iters, npoint=fl["npoint"],
                                            return_ground=True)
        if args.save:
            test_set._save_predflow(flow_pred[None], save_root=save_dir, batch_size=1, n_frame=1, offset=sid)
        if min(pc1_org.shape[0], pc2_org.shape[0]) < 1:      # the reference does not score empty frames either
            continue
        flow_gt = torch.from_numpy(flows[0]).to(device)
        for key, sel in (("all", None), ("ground", is_ground), ("above", torch.logical_not(is_ground))):
            gt, pred = (flow_gt, flow_pred) if sel is None else (flow_gt[sel], flow_pred[sel])
            if gt.shape[0] > 0:
                epe, acc_strict, acc_relax, outlier = eval_flow(gt[None], pred[None], epe_norm_thresh=EPE_NORM_THRESH)
                meters[key].append_loss({"EPE": epe, "AccS": acc_strict, "AccR": acc_relax, "Outlier": outlier})
    metrics = {key: meter.get_mean_loss_dict() for key, meter in meters.items()}
    for key, title in (("all", "Evaluation on waymo-%s:" % args.split), ("ground", "Ground points:"), ("above", "Above ground points:")):
        print(title, json.dumps({k: round(v, 5) for k, v in metrics[key].items()}), flush=True)
    if args.save:
        print("Saved to %s" % save_dir, flush=True)
    if tmp is not None and not args.save:   # saved flows stay where the line above says
        shutil.rmtree(tmp, ignore_errors=True)
    return metrics["all"]


if __name__ == "__main__":
    main()

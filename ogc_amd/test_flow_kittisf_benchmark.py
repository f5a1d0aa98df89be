"""The "FlowStep3D vs. ours" table on the KITTI-SF scenes (counterpart of the reference's test_flow_kittisf_benchmark.py:14-140).

    python -m ogc_amd.test_flow_kittisf_benchmark CONFIG [--predflow NAME] [--mapping FILE] [--synthetic N]

Per scene, in the forward direction only, two flows are evaluated on the SAME points at `epe_norm_thresh` 0.05:

  FlowStep3D   the full-resolution pair goes through the reference's `preproc` — points with y < -1.4 in BOTH frames are
               ground and leave; `n_sample_point` (8192) of the rest are drawn per frame with the host's numpy generator,
               seeded 18 once, two `np.random.choice` calls per scene (without replacement; with it when too few points
               remain), different indices for the two frames — and then through the network at `iters = 5`;
  Ours         the flow stored for the down-sampled scan, <data.root>_downsampled/flow_preds/<--predflow> (what `oa_icp_round`
               left there), without that scan's ground (y < -1.4), three-NN up-sampled onto the sampled points of frame 1.

The sampling indices are the host's (they ARE the protocol); everything after them stays on the device: indexing, the network,
`upsample_feat`, and the metrics — one launch of ogc_flow_eval and one four-number copy per evaluation (metrics/flow_eval.py),
where the reference copies both flows to the host.  Two AverageMeters; `main` prints the reference's two lines and returns
{"FlowStep3D": {...}, "Ours": {...}}.

Config: the reference's schema: save_path (a checkpoint FILE, {'state_dict': ...} with the trainer's 'model.' prefix, or this
package's {'model_state': ...}), data.root, flownet{...}; optional data.n_sample_point.  The split file is `--mapping`, by
default <data.root>/kitti142.txt.  `--synthetic N` writes N scans (utils/synthetic.py: write_kitti_processed_root) and their
down-sampled twins, whose own ground-truth flow is stored as the "predicted" one, into a temporary root; the checkpoint is
optional there.
"""
import argparse
import json
import os
import shutil
import tempfile

import numpy as np
import torch
import yaml

from .datasets import KITTISceneFlowDataset
from .metrics.flow_eval import eval_flow_device
from .test_flow_kittisf import load_weights
from .utils.data_util import upsample_feat
from .utils.pytorch_util import AverageMeter

GROUND_Y = -1.4
VIEW_SELS = [[0, 1], [1, 0]]
EPE_NORM_THRESH = 0.05
N_SAMPLE_POINT = 8192
MODEL_ITERS = 5
NUMPY_SEED = 18
DEFAULT_PREDFLOW = "flowstep3d_for-benchmark_R2"
KEYS = ("EPE", "AccS", "AccR", "Outlier")


def sample_indices(pc1, pc2, n_sample_point=N_SAMPLE_POINT):
    """pc1, pc2 (N, 3) numpy -> (not_ground (N,) bool, idx1, idx2 into the points that are left): the reference's `preproc`
    (:25-41) up to the indexing, consuming numpy's GLOBAL generator exactly as it does."""
    not_ground = np.logical_not(np.logical_and(pc1[:, 1] < GROUND_Y, pc2[:, 1] < GROUND_Y))
    n = int(not_ground.sum())
    try:
        idx1 = np.random.choice(n, size=n_sample_point, replace=False, p=None)
        idx2 = np.random.choice(n, size=n_sample_point, replace=False, p=None)
    except ValueError:   # fewer points than samples: replicate some
        idx1 = np.random.choice(n, size=n_sample_point, replace=True, p=None)
        idx2 = np.random.choice(n, size=n_sample_point, replace=True, p=None)
    return not_ground, idx1, idx2


def evaluate_scene(flownet, pcs_org, pc_down, flow_down, device, n_sample_point=N_SAMPLE_POINT, iters=MODEL_ITERS,
                   epe_norm_thresh=EPE_NORM_THRESH):
    """pcs_org (2, N, 3) the full-resolution pair (points in correspondence), pc_down (M, 3) / flow_down (M, 3) frame 1 of the
    down-sampled scan and the flow stored for it, all numpy -> (FlowStep3D's four metrics, ours), two tuples of floats."""
    not_ground, idx1, idx2 = sample_indices(pcs_org[0], pcs_org[1], n_sample_point)
    keep = torch.from_numpy(not_ground).to(device)
    idx1, idx2 = torch.from_numpy(idx1).to(device), torch.from_numpy(idx2).to(device)
    pc1_all, pc2_all = torch.from_numpy(pcs_org[0]).to(device)[keep], torch.from_numpy(pcs_org[1]).to(device)[keep]
    pc1, pc2 = pc1_all[idx1][None].contiguous(), pc2_all[idx2][None].contiguous()
    flow = (pc2_all - pc1_all)[idx1][None].contiguous()
    with torch.no_grad():
        flow_fs3d = flownet(pc1, pc2, pc1, pc2, iters=iters)[-1].detach()
    fs3d, _ = eval_flow_device(flow, flow_fs3d, epe_norm_thresh=epe_norm_thresh)
    pc_down, flow_down = torch.from_numpy(pc_down).to(device), torch.from_numpy(flow_down).to(device)
    above = torch.logical_not(pc_down[:, 1] < GROUND_Y)
    flow_ours = upsample_feat(pc1, pc_down[above][None].contiguous(), flow_down[above][None].contiguous())
    ours, _ = eval_flow_device(flow, flow_ours.contiguous(), epe_norm_thresh=epe_norm_thresh)
    return fs3d, ours


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("config")
    ap.add_argument("--predflow", default=DEFAULT_PREDFLOW, help="the stored flows: <data.root>_downsampled/flow_preds/<name>")
    ap.add_argument("--mapping", default=None, help="the split file listing the scene ids (default <data.root>/kitti142.txt)")
    ap.add_argument("--synthetic", type=int, default=0, help="run on this many synthetic scenes in a temporary root")
    args = ap.parse_args(argv)
    with open(args.config) as f:
        cfg = yaml.safe_load(f)
    device = torch.device("cuda")
    data = cfg.get("data") or {}
    n_sample_point = int(data.get("n_sample_point", N_SAMPLE_POINT))

    np.random.seed(NUMPY_SEED)      # the same seeds as FlowStep3D's own evaluation (:57-59)
    torch.manual_seed(NUMPY_SEED)

    from .models.flownet_kitti import FlowStep3D
    fl = cfg["flownet"]
    flownet = FlowStep3D(npoint=fl["npoint"], use_instance_norm=fl["use_instance_norm"], loc_flow_nn=fl["loc_flow_nn"],
                         loc_flow_rad=fl["loc_flow_rad"], k_decay_fact=0.5).to(device)
    loaded = load_weights(flownet, cfg["save_path"], required=not args.synthetic)
    flownet.eval()
    print("Loaded weights from %s" % loaded if loaded else "No checkpoint at %s: random weights" % cfg["save_path"], flush=True)

    tmp = None
    if args.synthetic:
        from .utils.synthetic import write_kitti_downsampled_root, write_kitti_processed_root
        tmp = tempfile.mkdtemp(prefix="ogc_flow_benchmark_") if not data.get("root") else None
        data_root = os.path.join(tmp, "kittisf") if tmp is not None else data["root"]
        n_points = data.get("n_points", 4096)
        mapping, _ = write_kitti_processed_root(data_root, args.synthetic, n_points, split="kitti142")
        mapping_down, _ = write_kitti_downsampled_root(data_root, data_root + "_downsampled", data.get("n_points_downsampled", n_points // 2),
                                                       predflow=args.predflow, split="kitti142")
    else:
        data_root = data["root"]
        mapping = mapping_down = args.mapping or os.path.join(data_root, "kitti142.txt")
    test_set = KITTISceneFlowDataset(data_root=data_root, mapping_path=mapping, downsampled=False, view_sels=VIEW_SELS)
    test_set_predflow = KITTISceneFlowDataset(data_root=data_root + "_downsampled", mapping_path=mapping_down, downsampled=True,
                                              view_sels=VIEW_SELS, predflow_path=args.predflow)

    meter_fs3d, meter = AverageMeter(), AverageMeter()
    for sid in range(len(test_set) // 2):       # the forward direction only
        pcs_org = test_set[sid * 2][0]
        pcs, _, flow_preds, _ = test_set_predflow[sid * 2]
        fs3d, ours = evaluate_scene(flownet, pcs_org, pcs[0], flow_preds[0], device, n_sample_point=n_sample_point)
        meter_fs3d.append_loss(dict(zip(KEYS, fs3d)))
        meter.append_loss(dict(zip(KEYS, ours)))
    result = {"FlowStep3D": meter_fs3d.get_mean_loss_dict(), "Ours": meter.get_mean_loss_dict()}
    print("FlowStep3D:", json.dumps(result["FlowStep3D"]), flush=True)
    print("Ours:", json.dumps(result["Ours"]), flush=True)
    if tmp is not None:
        shutil.rmtree(tmp, ignore_errors=True)
    return result


if __name__ == "__main__":
    main()

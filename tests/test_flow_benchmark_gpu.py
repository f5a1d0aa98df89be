"""ogc_amd.test_flow_kittisf_benchmark on the MI355X: `main --synthetic 3` at 4096 points per scan (2048 stored for the
down-sampled twin, 2048 drawn per frame for the network, random weights).

The stored "predicted" flow is the down-sampled scan's own ground truth: one rigid ego-motion of at most 0.04 rad, so three-NN
up-sampling over neighbours a few decimetres away errs by about a centimetre — the "Ours" EPE must lie below epe_norm_thresh
(0.05).  Both rows must equal a straight composition of the existing functions (flow_metrics, upsample_feat) under the same
numpy seed: rates within 2**-23 relative when the counts agree — they are compared as integers first — and EPE within 1e-6
relative (flow_metrics sums 2048 fp32 norms in fp32)."""
import os
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = os.path.join(ROOT, "config", "kittisf_flow_benchmark_synthetic.yaml")
N_SCENES, N_SAMPLE = 3, 2048
RATE_RTOL, EPE_RTOL = 2.0 ** -23, 1e-6
KEYS = ("EPE", "AccS", "AccR", "Outlier")


@pytest.fixture(scope="module")
def first_run():
    from ogc_amd.test_flow_kittisf_benchmark import main
    return main([CONFIG, "--synthetic", str(N_SCENES), "--predflow", "stored"])


def _straight_composition(tmp):
    """The reference's loop on the existing functions: numpy preproc, the network, flow_metrics, upsample_feat."""
    import yaml
    from ogc_amd.datasets import KITTISceneFlowDataset
    from ogc_amd.metrics.flow_metric import flow_metrics
    from ogc_amd.models.flownet_kitti import FlowStep3D
    from ogc_amd.utils.data_util import upsample_feat
    from ogc_amd.utils.pytorch_util import AverageMeter
    from ogc_amd.utils.synthetic import write_kitti_downsampled_root, write_kitti_processed_root
    cfg = yaml.safe_load(open(CONFIG))
    root = os.path.join(tmp, "kittisf")
    mapping, _ = write_kitti_processed_root(root, N_SCENES, cfg["data"]["n_points"], split="kitti142")
    mapping_down, _ = write_kitti_downsampled_root(root, root + "_downsampled", cfg["data"]["n_points_downsampled"], predflow="stored",
                                                   split="kitti142")
    np.random.seed(18)
    torch.manual_seed(18)
    fl = cfg["flownet"]
    flownet = FlowStep3D(npoint=fl["npoint"], use_instance_norm=fl["use_instance_norm"], loc_flow_nn=fl["loc_flow_nn"],
                         loc_flow_rad=fl["loc_flow_rad"], k_decay_fact=0.5).cuda().eval()
    full = KITTISceneFlowDataset(root, mapping, downsampled=False, view_sels=[[0, 1], [1, 0]])
    down = KITTISceneFlowDataset(root + "_downsampled", mapping_down, downsampled=True, view_sels=[[0, 1], [1, 0]], predflow_path="stored")
    meters = {"FlowStep3D": AverageMeter(), "Ours": AverageMeter()}
    for sid in range(N_SCENES):
        pcs_org, _, flows_org, _ = full[2 * sid]
        pcs, _, flow_preds, _ = down[2 * sid]
        pc1, pc2, flow = pcs_org[0], pcs_org[1], flows_org[0]
        keep = np.logical_not(np.logical_and(pc1[:, 1] < -1.4, pc2[:, 1] < -1.4))
        pc1, pc2, flow = pc1[keep], pc2[keep], flow[keep]
        assert pc1.shape[0] > N_SAMPLE                         # the path without replacement
        i1 = np.random.choice(pc1.shape[0], size=N_SAMPLE, replace=False, p=None)
        i2 = np.random.choice(pc1.shape[0], size=N_SAMPLE, replace=False, p=None)
        pc1, pc2, flow = (torch.from_numpy(a)[None].cuda() for a in (pc1[i1], pc2[i2], flow[i1]))
        with torch.no_grad():
            pred = flownet(pc1, pc2, pc1, pc2, iters=5)[-1]
        meters["FlowStep3D"].append_loss(dict(zip(KEYS, flow_metrics(flow, pred, 0.05).tolist())))
        above = np.logical_not(pcs[0][:, 1] < -1.4)
        ours = upsample_feat(pc1, torch.from_numpy(pcs[0][above])[None].cuda(), torch.from_numpy(flow_preds[0][above])[None].cuda())
        meters["Ours"].append_loss(dict(zip(KEYS, flow_metrics(flow, ours, 0.05).tolist())))
    return {k: m.get_mean_loss_dict() for k, m in meters.items()}


def test_ours_row_is_accurate_and_both_rows_equal_the_existing_functions(first_run, tmp_path):
    from ogc_amd.test_flow_kittisf_benchmark import EPE_NORM_THRESH
    assert set(first_run) == {"FlowStep3D", "Ours"} and all(set(row) == set(KEYS) for row in first_run.values())
    want = _straight_composition(str(tmp_path))
    for row in ("FlowStep3D", "Ours"):
        print("FLOW_BENCHMARK %s " % row + " ".join("%s %.8f (want %.8f)" % (k, first_run[row][k], want[row][k]) for k in KEYS))
    assert first_run["Ours"]["EPE"] < EPE_NORM_THRESH
    for row in ("FlowStep3D", "Ours"):
        got = first_run[row]
        for key in ("AccS", "AccR", "Outlier"):
            # a mean over 3 scenes of counts / 2048: the same integers on both paths
            assert round(got[key] * N_SCENES * N_SAMPLE) == round(want[row][key] * N_SCENES * N_SAMPLE), (row, key)
            assert abs(got[key] - want[row][key]) <= RATE_RTOL * want[row][key]
        assert abs(got["EPE"] - want[row]["EPE"]) <= EPE_RTOL * want[row]["EPE"]


def test_two_runs_give_identical_numbers(first_run):
    from ogc_amd.test_flow_kittisf_benchmark import main
    again = main([CONFIG, "--synthetic", str(N_SCENES), "--predflow", "stored"])
    assert again == first_run

"""The KITTI-SF flow-prediction driver (ogc_amd/test_flow_kittisf.py) on two synthetic full-resolution scenes: a static world
above a ground sheet below -1.4 m, seen under a known ego-motion (ogc_amd/utils/synthetic.py::make_kitti_raw_scene).

Network: flownet_kitti with npoint = 1024, loc_flow_nn = 16, loc_flow_rad = 1.5, seeded random weights, two unrolling
iterations; ICP on 256 points per frame."""
import os
import sys

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
N_POINTS, N_ICP, NPOINT, ITERS = 3000, 256, 1024, 2


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    from ogc_amd.utils.synthetic import write_kitti_processed_root
    root = str(tmp_path_factory.mktemp("kittisf"))
    mapping, motions = write_kitti_processed_root(root, 2, N_POINTS, seed=1000, split="val")
    return root, mapping, motions


@pytest.fixture(scope="module")
def flownet():
    from ogc_amd.models.flownet_kitti import FlowStep3D
    torch.manual_seed(10)
    return FlowStep3D(npoint=NPOINT, use_instance_norm=False, loc_flow_nn=16, loc_flow_rad=1.5, k_decay_fact=0.5).cuda().eval()


def _pair(root, sid):
    d = os.path.join(root, "processed", "%06d" % sid)
    return np.load(os.path.join(d, "pc1.npy")), np.load(os.path.join(d, "pc2.npy"))


def test_predict_pair_is_the_composition_of_the_public_stages(scenes, flownet):
    from ogc_amd.pointnet2.pointnet2 import furthest_point_sample
    from ogc_amd.test_flow_kittisf import predict_pair
    from ogc_amd.utils.data_util import upsample_feat
    from ogc_amd.utils.icp_util import icp_batch, rigid_apply, rigid_flow
    pc1_np, pc2_np = _pair(scenes[0], 0)
    pc1_org, pc2_org = torch.from_numpy(pc1_np).cuda(), torch.from_numpy(pc2_np).cuda()
    got = predict_pair(flownet, pc1_org, pc2_org, n_point_icp=N_ICP, max_icp_iters=50, iters=ITERS)
    assert got.shape == (N_POINTS, 3) and got.dtype == torch.float32 and got.is_cuda

    def fps(pc, k):
        return pc[furthest_point_sample(pc[None].contiguous(), k)[0].long()][None].contiguous()

    with torch.no_grad():
        keep = ~((pc1_org[:, 1] < -1.4) & (pc2_org[:, 1] < -1.4))
        assert 0 < int(keep.sum()) < N_POINTS and int(keep.sum()) >= NPOINT
        pc1, pc2 = pc1_org[keep], pc2_org[keep]
        center = torch.cat([pc1, pc2], 0).mean(0)
        T, _, _ = icp_batch(fps(pc1 - center, N_ICP), fps(pc2 - center, N_ICP), max_iterations=50)
        want = rigid_flow(pc1_org, T[0])
        pc1 = rigid_apply(pc1, T[0])
        pc1_fps, pc2_fps = fps(pc1, NPOINT), fps(pc2, NPOINT)
        flow_fps = flownet(pc1_fps, pc2_fps, pc1_fps, pc2_fps, iters=ITERS)[-1]
        want[keep] += upsample_feat(pc1[None], pc1_fps, flow_fps)[0]
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_icp_part_of_the_flow_beats_the_zero_flow(scenes):
    """... on the device, and in the float64 numpy ICP of the fixture generator on the same FPS samples."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from make_icp_golden import icp_trace
    from ogc_amd.pointnet2.pointnet2 import furthest_point_sample
    from ogc_amd.utils.icp_util import icp_batch, rigid_flow
    for sid in range(2):
        pc1_np, pc2_np = _pair(scenes[0], sid)
        truth = scenes[2][sid]
        rigid = (pc1_np.astype(np.float64) @ truth[:3, :3].T + truth[:3, 3] - pc1_np).astype(np.float32)
        assert np.abs(rigid - (pc2_np - pc1_np)).max() < 1e-4       # the scene's flow IS the rigid flow of the ego-motion
        keep = ~((pc1_np[:, 1] < -1.4) & (pc2_np[:, 1] < -1.4))
        center = np.concatenate([pc1_np[keep], pc2_np[keep]], 0).mean(0)
        a, b = torch.from_numpy(pc1_np[keep] - center).cuda(), torch.from_numpy(pc2_np[keep] - center).cuda()
        a = a[furthest_point_sample(a[None].contiguous(), N_ICP)[0].long()][None].contiguous()
        b = b[furthest_point_sample(b[None].contiguous(), N_ICP)[0].long()][None].contiguous()
        T, _, _ = icp_batch(a, b, max_iterations=50)
        zero_epe = float(np.linalg.norm(rigid, axis=1).mean())
        gpu_flow = rigid_flow(torch.from_numpy(pc1_np).cuda(), T[0]).cpu().numpy()
        gpu_epe = float(np.linalg.norm(gpu_flow - rigid, axis=1).mean())
        T64 = icp_trace(a[0].cpu().numpy(), b[0].cpu().numpy(), max_iterations=50)[0]
        cpu_flow = pc1_np.astype(np.float64) @ T64[:3, :3].T + T64[:3, 3] - pc1_np
        cpu_epe = float(np.linalg.norm(cpu_flow - rigid, axis=1).mean())
        print("FLOW_PREDICT scene %d zero-flow EPE %.4f ICP EPE gpu %.4f numpy %.4f" % (sid, zero_epe, gpu_epe, cpu_epe))
        assert cpu_epe < zero_epe
        assert gpu_epe < zero_epe


def test_main_saves_flows_the_reader_returns(scenes, tmp_path):
    from ogc_amd.datasets import KITTISceneFlowDataset
    from ogc_amd.test_flow_kittisf import main
    root, mapping, _ = scenes
    cfg = {"dataset": "kittisf", "save_path": str(tmp_path / "no_checkpoint"), "random_seed": 10, "data": {"root": root},
           "flownet": {"npoint": NPOINT, "use_instance_norm": False, "loc_flow_nn": 16, "loc_flow_rad": 1.5, "k_decay_fact": 1.0}}
    path = str(tmp_path / "cfg.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    with pytest.raises(FileNotFoundError):      # a real run needs its checkpoint
        main([path, "--split", "val", "--mapping", mapping])
    from ogc_amd.models.flownet_kitti import FlowStep3D
    torch.manual_seed(3)
    net = FlowStep3D(npoint=NPOINT, use_instance_norm=False, loc_flow_nn=16, loc_flow_rad=1.5, k_decay_fact=0.5)
    os.makedirs(cfg["save_path"])
    torch.save({"model_state": net.state_dict()}, os.path.join(cfg["save_path"], "best.pth.tar"))
    metrics = main([path, "--split", "val", "--mapping", mapping, "--test_model_iters", str(ITERS), "--n_point_icp", str(N_ICP),
                    "--save"])
    assert set(metrics) == {"EPE", "AccS", "AccR", "Outlier"} and all(np.isfinite(v) for v in metrics.values())
    stored = {}
    for sid in range(2):
        for k in (1, 2):
            flow = np.load(os.path.join(root, "flow_preds", "flowstep3d", "%06d" % sid, "flow%d.npy" % k))
            assert flow.shape == (N_POINTS, 3) and flow.dtype == np.float32
            stored[sid, k] = flow
    reader = KITTISceneFlowDataset(data_root=root, mapping_path=mapping, downsampled=False, view_sels=[[0, 1], [1, 0]],
                                   predflow_path="flowstep3d")
    for sid in range(2):
        for v in range(2):
            _, _, flows, _ = reader[2 * sid + v]
            assert np.array_equal(flows[0], stored[sid, 1 + v]) and np.array_equal(flows[1], stored[sid, 2 - v])

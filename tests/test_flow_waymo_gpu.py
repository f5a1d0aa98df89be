"""The Waymo flow-prediction driver (ogc_amd/test_flow_waymo.py) on one synthetic sequence of three frames of about 6000 points
with unequal counts: a static world of boxes on a tilted ground sheet, seen under known poses
(ogc_amd/utils/synthetic.py::make_waymo_sequence).

Network: flownet_kitti with npoint = 1024, loc_flow_nn = 16, loc_flow_rad = 1.5, seeded random weights, two unrolling
iterations; ICP on 256 points per frame, ground-plane fitting on 1024 points per frame with n_lpr = 50."""
import collections
import os
import shutil

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu
N_POINTS, N_GPF, N_LPR, N_ICP, NPOINT, ITERS = 6000, 1024, 50, 256, 1024, 2
SEQ = "seq_0000"


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    from ogc_amd.utils.synthetic import write_waymo_root
    root = str(tmp_path_factory.mktemp("waymo"))
    mapping, poses = write_waymo_root(root, 1, 3, N_POINTS, seed=2000, split="val")
    return root, mapping, poses[SEQ]


@pytest.fixture(scope="module")
def flownet():
    from ogc_amd.models.flownet_kitti import FlowStep3D
    torch.manual_seed(10)
    return FlowStep3D(npoint=NPOINT, use_instance_norm=False, loc_flow_nn=16, loc_flow_rad=1.5, k_decay_fact=0.5).cuda().eval()


def _load(root, t, what="pc"):
    return np.load(os.path.join(root, "data", SEQ, "%s_%04d.npy" % (what, t)))


@pytest.mark.parametrize("bound,denoise", ((False, False), (True, True)))
def test_predict_pair_is_the_composition_of_the_public_stages(scene, flownet, bound, denoise):
    from ogc_amd.pointnet2.pointnet2 import furthest_point_sample
    from ogc_amd.test_flow_waymo import predict_pair, register_bound
    from ogc_amd.utils.data_util import upsample_feat
    from ogc_amd.utils.gpf_util import ground_plane_fit_batch, plane_mask
    from ogc_amd.utils.icp_util import icp_batch, rigid_apply, rigid_flow
    pc1_org, pc2_org = torch.from_numpy(_load(scene[0], 1)).cuda(), torch.from_numpy(_load(scene[0], 0)).cuda()
    assert pc1_org.shape[0] != pc2_org.shape[0] and min(pc1_org.shape[0], pc2_org.shape[0]) >= N_GPF
    got = predict_pair(flownet, pc1_org, pc2_org, bound=bound, denoise=denoise, n_point_gpf=N_GPF, n_gpf_lpr=N_LPR,
                       n_point_icp=N_ICP, max_icp_iters=50, iters=ITERS)
    assert got.shape == pc1_org.shape and got.dtype == torch.float32 and got.is_cuda

    def fps(pc, k):
        return pc[furthest_point_sample(pc[None].contiguous(), k)[0].long()][None].contiguous()

    with torch.no_grad():
        planes, _, attempts = ground_plane_fit_batch(torch.cat([fps(pc1_org, N_GPF), fps(pc2_org, N_GPF)], 0), n_iter=5,
                                                     n_lpr=N_LPR, thresh_seed=0.4, thresh_dist=0.4)
        assert attempts.tolist() == [1, 1]
        keep1 = ~((pc1_org[:, 1] < 0.3) | plane_mask(pc1_org, planes[0], 0.4))
        keep2 = ~((pc2_org[:, 1] < 0.3) | plane_mask(pc2_org, planes[1], 0.4))
        pc1, pc2 = pc1_org[keep1], pc2_org[keep2]
        center = torch.cat([pc1, pc2], 0).mean(0)
        T = icp_batch(fps(pc1 - center, N_ICP), fps(pc2 - center, N_ICP), max_iterations=50)[0][0]
        want = rigid_flow(pc1_org, T)
        pc1 = rigid_apply(pc1, T)
        sel1 = register_bound(pc1, pc2, T[:3, :3], T[:3, 3], bound)
        pc1_sel = pc1[sel1]
        sel2 = register_bound(pc2, pc1_sel, T[:3, :3].T, -(T[:3, :3].T @ T[:3, 3]), bound)
        pc2_sel = pc2[sel2]
        if bound:
            assert 0 < int(sel1.sum()) < pc1.shape[0] and 0 < int(sel2.sum()) < pc2.shape[0]
        else:
            assert bool(sel1.all()) and bool(sel2.all())
        assert min(pc1_sel.shape[0], pc2_sel.shape[0]) >= NPOINT // 2
        pc1_fps, pc2_fps = fps(pc1_sel, min(NPOINT, pc1_sel.shape[0])), fps(pc2_sel, min(NPOINT, pc2_sel.shape[0]))
        flow_fps = flownet(pc1_fps, pc2_fps, pc1_fps, pc2_fps, iters=ITERS)[-1]
        flow_sel = upsample_feat(pc1_sel[None].contiguous(), pc1_fps, flow_fps)[0]
        if denoise:
            flow_sel = flow_sel.clone()
            flow_sel[flow_sel.norm(dim=1) > 2.5] = 0
        flow = torch.zeros_like(pc1)
        flow[sel1] = flow_sel
        want[keep1] += flow
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert not torch.equal(got, rigid_flow(pc1_org, T))          # the network's residual is in it


def test_ground_mask_equals_the_labels_where_the_height_threshold_does_not(scene):
    from ogc_amd.test_flow_waymo import ground_masks, predict_pair
    for t in (1, 2):
        pc1_np, pc2_np = _load(scene[0], t), _load(scene[0], t - 1)
        labels1, labels2 = _load(scene[0], t, "ground").astype(bool), _load(scene[0], t - 1, "ground").astype(bool)
        masks = ground_masks(torch.from_numpy(pc1_np).cuda(), torch.from_numpy(pc2_np).cuda(), n_point_gpf=N_GPF, n_gpf_lpr=N_LPR)
        by_height = pc1_np[:, 1] < 0.3
        print("WAYMO_GROUND frame %d: labels %d, driver differs at %d, height threshold alone differs at %d"
              % (t, int(labels1.sum()), int((masks[0].cpu().numpy() != labels1).sum()), int((by_height != labels1).sum())))
        assert masks[0].dtype == torch.bool and np.array_equal(masks[0].cpu().numpy(), labels1)
        assert np.array_equal(masks[1].cpu().numpy(), labels2)
        assert not np.array_equal(by_height, labels1)           # the reason the stage exists
    # a frame below n_point_gpf points takes the one-launch-per-frame path and all its points: the same labels
    small = torch.from_numpy(pc2_np[:800]).cuda()
    masks = ground_masks(torch.from_numpy(pc1_np).cuda(), small, n_point_gpf=N_GPF, n_gpf_lpr=N_LPR)
    assert np.array_equal(masks[0].cpu().numpy(), labels1) and np.array_equal(masks[1].cpu().numpy(), labels2[:800])
    flow, ground = predict_pair(None, torch.from_numpy(pc1_np).cuda(), torch.zeros(0, 3, device="cuda"), return_ground=True)
    assert flow.shape == pc1_np.shape and not flow.any() and ground.shape == labels1.shape and not ground.any()


def test_odometry_gives_the_stored_rigid_flow(scene, flownet):
    from ogc_amd.test_flow_waymo import ego_motion_from_poses, predict_pair
    from ogc_amd.utils.icp_util import rigid_flow
    root, _, poses = scene
    pc1_org, pc2_org = torch.from_numpy(_load(root, 2)).cuda(), torch.from_numpy(_load(root, 1)).cuda()
    stored = np.load(os.path.join(root, "data", SEQ, "flow_0002_0001.npy"))
    rigid = rigid_flow(pc1_org, ego_motion_from_poses(poses[2], poses[1]).cuda()).cpu().numpy()
    flow, ground = predict_pair(flownet, pc1_org, pc2_org, pose=(poses[2], poses[1]), n_point_gpf=N_GPF, n_gpf_lpr=N_LPR,
                                iters=ITERS, return_ground=True)
    flow, ground = flow.cpu().numpy(), ground.cpu().numpy()
    print("WAYMO_ODOMETRY rigid flow vs stored %.3e, ground part of the prediction vs stored %.3e"
          % (np.abs(rigid - stored).max(), np.abs(flow[ground] - stored[ground]).max()))
    assert np.abs(rigid - stored).max() < 1e-4                  # a static world: the stored flow IS the ego-motion's
    assert ground.any() and np.abs(flow[ground] - stored[ground]).max() < 1e-4
    assert np.array_equal(flow[ground], rigid[ground])          # the network adds nothing on the ground


def _config(tmp_path, root):
    cfg = {"dataset": "waymo", "save_path": str(tmp_path / "no_checkpoint"), "random_seed": 10, "data": {"root": root},
           "flownet": {"npoint": NPOINT, "use_instance_norm": False, "loc_flow_nn": 16, "loc_flow_rad": 1.5, "k_decay_fact": 1.0}}
    path = str(tmp_path / "cfg.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    return cfg, path


def _checkpoint(cfg):
    from ogc_amd.models.flownet_kitti import FlowStep3D
    torch.manual_seed(3)
    net = FlowStep3D(npoint=NPOINT, use_instance_norm=False, loc_flow_nn=16, loc_flow_rad=1.5, k_decay_fact=0.5)
    os.makedirs(cfg["save_path"])
    torch.save({"model_state": net.state_dict()}, os.path.join(cfg["save_path"], "best.pth.tar"))


SMALL = ["--test_model_iters", str(ITERS), "--n_point_gpf", str(N_GPF), "--n_gpf_lpr", str(N_LPR), "--n_point_icp", str(N_ICP)]


def test_main_saves_flows_the_reader_returns(scene, tmp_path, capsys):
    from ogc_amd.datasets import WaymoOpenDataset
    from ogc_amd.test_flow_waymo import main
    root, mapping, _ = scene
    cfg, path = _config(tmp_path, root)
    with pytest.raises(FileNotFoundError):      # a real run needs its checkpoint
        main([path, "--split", "val"])
    _checkpoint(cfg)
    metrics = main([path, "--split", "val", "--save"] + SMALL)       # the mapping is <root>/val.txt by default
    assert set(metrics) == {"EPE", "AccS", "AccR", "Outlier"} and all(np.isfinite(v) for v in metrics.values())
    out = capsys.readouterr().out
    assert "Evaluation on waymo-val:" in out and "Ground points:" in out and "Above ground points:" in out
    reader = WaymoOpenDataset(root, mapping, predflow_path="flowstep3d_gpf")
    assert reader.data_ids == [(SEQ, 1, 0), (SEQ, 2, 1)]
    for sid, (_, t, u) in enumerate(reader.data_ids):
        flow = np.load(os.path.join(root, "flow_preds", "flowstep3d_gpf", SEQ, "flow_%04d_%04d.npy" % (t, u)))
        assert flow.shape == _load(root, t).shape and flow.dtype == np.float32 and np.isfinite(flow).all()
        _, _, flows, _ = reader[sid]
        assert np.array_equal(flows[0], flow) and np.array_equal(flows[1], flow)
    metrics = main([path, "--split", "val", "--mapping", mapping, "--save", "--use_odometry", "--bound"] + SMALL)
    assert all(np.isfinite(v) for v in metrics.values())
    for t, u in ((1, 0), (2, 1)):
        flow = np.load(os.path.join(root, "flow_preds", "flowstep3d_gpf_odo_bound", SEQ, "flow_%04d_%04d.npy" % (t, u)))
        assert flow.shape == _load(root, t).shape and flow.dtype == np.float32
    assert sorted(os.listdir(os.path.join(root, "flow_preds"))) == ["flowstep3d_gpf", "flowstep3d_gpf_odo_bound"]


def test_empty_frame_yields_zero_flows_and_launches_nothing(scene, tmp_path):
    from ogc_amd import _lib
    from ogc_amd.test_flow_waymo import main
    root = str(tmp_path / "root")
    shutil.copytree(os.path.join(scene[0], "data"), os.path.join(root, "data"))
    shutil.copy(scene[1], os.path.join(root, "val.txt"))
    d = os.path.join(root, "data", SEQ)
    np.save(os.path.join(d, "pc_0001.npy"), np.zeros((0, 3), np.float32))
    np.save(os.path.join(d, "segm_0001.npy"), np.zeros((0,), np.int32))
    np.save(os.path.join(d, "semantic_segm_0001.npy"), np.zeros((0,), np.int32))
    np.save(os.path.join(d, "flow_0001_0000.npy"), np.zeros((0, 3), np.float32))
    cfg, path = _config(tmp_path, root)
    _checkpoint(cfg)
    _lib.CALL_COUNTS = collections.Counter()
    try:
        main([path, "--split", "val", "--save"] + SMALL)        # every sample of this sequence touches the empty frame
        calls = dict(_lib.CALL_COUNTS)
    finally:
        _lib.CALL_COUNTS = None
    assert calls == {}, "an empty frame must not reach the kernels"
    first = np.load(os.path.join(root, "flow_preds", "flowstep3d_gpf", SEQ, "flow_0001_0000.npy"))
    second = np.load(os.path.join(root, "flow_preds", "flowstep3d_gpf", SEQ, "flow_0002_0001.npy"))
    assert first.shape == (0, 3) and first.dtype == np.float32
    assert second.shape == _load(root, 2).shape and second.dtype == np.float32 and not second.any()

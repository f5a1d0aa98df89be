"""The voting driver on data-set roots (`python -m ogc_amd.vote CONFIG --split S ...`, reference vote.py:134-353), the
restructured voting sweep that feeds the fused correspondence kernel, and the kernel's place in the C ABI — on the CPU, with
the oracle's operators under the network."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEGNET = {"n_slot": 4, "n_point": 256, "use_xyz": True, "n_transformer_layer": 1, "transformer_embed_dim": 32,
          "transformer_input_pos_enc": False}
KEYS = {"AP", "PQ", "F1", "Pre", "Rec", "per_scan_iou_avg", "per_scan_iou_std", "per_scan_ri_avg", "per_scan_ri_std"}


@pytest.fixture()
def cpu_ops(monkeypatch, oracle):
    import ogc_amd.pointnet2.pointnet2 as api
    monkeypatch.setattr(api, "_native", oracle.Pointnet2CudaCPU())
    return api


def _config(tmp_path, dataset, n_point, **extra):
    """A config, its data root and a checkpoint of random weights (so that the driver and the test load the same network)."""
    from ogc_amd import test_seg
    root = str(tmp_path / "data")
    os.makedirs(root, exist_ok=True)
    cfg = dict({"dataset": dataset, "save_path": str(tmp_path / "ckpt" / "seg"), "random_seed": 10,
                "data": {"root": root, "decentralize": dataset != "sapien", "n_objects": 3},
                "segnet": dict(SEGNET, n_point=n_point)}, **extra)
    path = str(tmp_path / "cfg.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    torch.manual_seed(5)
    os.makedirs(cfg["save_path"], exist_ok=True)
    torch.save({"model_state": test_seg.build_segnet(cfg).state_dict()}, os.path.join(cfg["save_path"], "best.pth.tar"))
    return cfg, path, root


def _reference_shaped(cfg, root, window, predflow=None, mapping=None):
    """The reference's loop, scene by scene: network, mask_voting, accumulate_eval_results / ClusteringMetrics / calculate_*
    of metrics/seg_metric.py (vote.py:299-353) -> (metrics of the voted masks, metrics of the raw masks)."""
    from ogc_amd import test_seg, vote
    from ogc_amd.metrics.seg_metric import ClusteringMetrics, accumulate_eval_results, calculate_AP, calculate_PQ_F1
    segnet = test_seg.build_segnet(cfg)
    segnet.load_state_dict(torch.load(test_seg.weight_path(cfg, 0), map_location="cpu")["model_state"])
    segnet.eval()
    test_set, n_frame, thresh, _ = vote.build_vote_set(cfg, "val", root, mapping, predflow_path=predflow)
    out = []
    for use_vote in (True, False):
        iou, matched, conf, n_gt, rows = [], [], [], 0, []
        for sid in range(len(test_set) // n_frame):
            samples = [test_set[n_frame * sid + k] for k in range(n_frame)]
            pc = torch.stack([torch.as_tensor(s[0][0]) for s in samples])
            segm = torch.stack([torch.as_tensor(s[1][0]) for s in samples])
            flows = torch.stack([torch.as_tensor(s[2]) for s in samples])[:n_frame - 1].contiguous()
            with torch.no_grad():
                mask = segnet(pc, pc).detach()
            if use_vote:
                mask = vote.mask_voting(pc, mask, flows, time_window_size=window)
            a, b, c, d = accumulate_eval_results(segm, mask, thresh)
            iou.append(a); matched.append(b); conf.append(c); n_gt += d
            scan = ClusteringMetrics()(mask, segm.long(), thresh)
            rows.append([np.mean(scan["iou"]), np.std(scan["iou"]), np.mean(scan["ri"]), np.std(scan["ri"])])
        iou, matched, conf = np.concatenate(iou), np.concatenate(matched), np.concatenate(conf)
        pq, f1, pre, rec = calculate_PQ_F1(iou, matched, n_gt)
        rows = np.mean(np.array(rows), 0)
        out.append({"AP": calculate_AP(matched, conf, n_gt), "PQ": pq, "F1": f1, "Pre": pre, "Rec": rec,
                    "per_scan_iou_avg": rows[0], "per_scan_iou_std": rows[1], "per_scan_ri_avg": rows[2],
                    "per_scan_ri_std": rows[3]})
    return out


def _same(got, want):
    assert set(got) == KEYS
    for k in KEYS:
        assert math.isfinite(got[k]) and got[k] == pytest.approx(float(want[k]), rel=1e-6, abs=1e-9), (k, got[k], want[k])


def test_driver_on_an_ogcdr_root(cpu_ops, tmp_path, capsys):
    from ogc_amd import vote
    cfg, path, root = _config(tmp_path, "ogcdr", 256)
    res = vote.main([path, "--split", "val", "--synthetic", "2", "--use_gt_flow", "--save", "--device", "cpu",
                     "--test_batch_size", "8", "--num_workers", "0"])
    save_dir = os.path.join(root, "segm_preds", "Vote_T3")
    assert res["save_dir"] == save_dir
    for scene in ("00000000", "00000001"):
        for k in range(4):
            lab = np.load(os.path.join(save_dir, scene, "segm_%02d.npy" % k))
            assert lab.shape == (256,) and lab.dtype == np.int64 and 0 <= lab.min() and lab.max() < 4
    voted, raw = _reference_shaped(cfg, root, 3)
    _same(res["voted"], voted)
    _same(res["raw"], raw)
    out = capsys.readouterr().out
    assert "Evaluation on ogcdr-val:" in out and "AveragePrecision@50:" in out and "PanopticQuality@50:" in out
    assert "Without voting:" in out and "Loaded weights from" in out


def test_driver_on_a_kittisf_root_reads_predicted_flows(cpu_ops, tmp_path):
    from ogc_amd import vote
    cfg, path, root = _config(tmp_path, "kittisf", 512, predflow_path="flowstep3d")
    res = vote.main([path, "--split", "val", "--synthetic", "2", "--save", "--device", "cpu", "--test_batch_size", "4",
                     "--time_window_size", "2", "--num_workers", "0"])
    assert os.path.isdir(os.path.join(root, "flow_preds", "flowstep3d"))
    for scene in ("000000", "000001"):
        for k in (1, 2):
            assert np.load(os.path.join(root, "segm_preds", "Vote_T2", scene, "segm%d.npy" % k)).shape == (512,)
    voted, raw = _reference_shaped(cfg, root, 2, predflow="flowstep3d", mapping=os.path.join(root, "val.txt"))
    _same(res["voted"], voted)
    _same(res["raw"], raw)


def test_driver_on_single_frames(cpu_ops, tmp_path):
    from ogc_amd import vote
    cfg, path, root = _config(tmp_path, "kittidet", 512)
    res = vote.main([path, "--split", "val", "--synthetic", "3", "--use_gt_flow", "--save", "--device", "cpu",
                     "--test_batch_size", "2", "--num_workers", "0"])
    for scene in ("000000", "000001", "000002"):
        assert np.load(os.path.join(root, "segm_preds", "Vote_T3", scene, "segm.npy")).shape == (512,)
    _same(res["voted"], res["raw"])            # one frame: the voted mask is the row-normalised mask
    voted, _ = _reference_shaped(cfg, root, 3, mapping=os.path.join(root, "val.txt"))
    _same(res["voted"], voted)


def test_argument_errors(cpu_ops, tmp_path):
    from ogc_amd import vote
    cfg, path, root = _config(tmp_path, "ogcdr", 256)
    with pytest.raises(ValueError, match="predflow_path"):
        vote.main([path, "--split", "val", "--synthetic", "1", "--device", "cpu"])
    with pytest.raises(ValueError, match="Frames of one scene should be in the same batch"):
        vote.main([path, "--split", "val", "--synthetic", "1", "--use_gt_flow", "--device", "cpu", "--test_batch_size", "6"])


def test_without_split_the_old_mode_stands(cpu_ops, tmp_path):
    from ogc_amd import train_seg, vote
    cfg, path, root = _config(tmp_path, "sapien", 128)
    os.makedirs(cfg["save_path"] + "_R0", exist_ok=True)
    torch.save({"model_state": train_seg.build_segnet(cfg).state_dict()}, os.path.join(cfg["save_path"] + "_R0", "best.pth.tar"))
    res = vote.main([path, "--n_sequence", "1", "--n_frame", "3", "--device", "cpu"])
    assert set(res) == {"raw", "voted"}
    for key in ("raw", "voted"):
        assert set(res[key]) == {"AP", "PQ", "F1", "Pre", "Rec", "mIoU", "RI"}


def _dense_soft_carry(b, n1, n2, c, temperature, p1, p2, x, out):
    """What ogc_soft_carry computes, with the (n1, n2) matrix."""
    assert p1.shape == (b, n1, 3) and p2.shape == (b, n2, 3) and x.shape == (b, n2, c) and out.shape == (b, n1, c)
    out.copy_((-torch.cdist(p1, p2) / temperature).softmax(-1) @ x)


@pytest.mark.parametrize("T,window", [(2, 3), (3, 1), (5, 2), (5, 4), (1, 3)])
def test_restructured_sweep_equals_dense_chains(cpu_ops, T, window):
    """_vote_scenes (every adjacency once, all spans side by side, one assignment call) with the kernel replaced by its dense
    definition, against the reference's voting on collect_correspondences."""
    from test_vote_cpu import _dense_voting
    from ogc_amd import vote
    from ogc_amd.utils.synthetic import make_sequence
    calls = []

    def counted(*args):
        calls.append(args[3])
        _dense_soft_carry(*args)
    cpu_ops._native.soft_carry_wrapper = counted
    carry = vote._native_carry()
    assert carry is not None
    got, want = [], []
    seqs = [make_sequence(max(T, 2), 96, 4, seed=T * 10 + window + s, outdoor=False) for s in range(2)]
    seqs = [(pc[:T], segm[:T], flows[:T - 1]) for pc, segm, flows in seqs]       # (a single frame: no flows)
    g = torch.Generator().manual_seed(1)
    masks = [(3.0 * torch.eye(4)[segm] + torch.randn(T, 96, 4, generator=g)).softmax(-1) for _, segm, _ in seqs]
    got = vote._vote_scenes(torch.stack([s[0] for s in seqs]), torch.stack(masks), torch.stack([s[2] for s in seqs]), window, carry)
    assert got.shape == (2, T, 96, 4)
    for i, (pc, _, flows) in enumerate(seqs):
        want = _dense_voting(vote, pc, masks[i], flows, window)
        assert torch.allclose(got[i], want, rtol=1e-4, atol=1e-6)
    assert torch.allclose(got.sum(-1), torch.ones(2, T, 96), atol=1e-5)
    assert len(calls) == 2 * (T - 1)                       # one call per adjacency and direction, whatever the scenes
    if (T, window) == (5, 4):
        assert max(calls) == 4 + 5 + 6 + 7                 # adjacency (0, 1) carries the spans to frames 1 .. 4


def test_cpu_inputs_keep_the_dense_path(cpu_ops):
    """A native with the kernel does not send CPU tensors to it."""
    from ogc_amd import vote
    from ogc_amd.utils.synthetic import make_sequence

    def refuse(*args):
        raise AssertionError("the kernel was called on CPU tensors")
    cpu_ops._native.soft_carry_wrapper = refuse
    pc, segm, flows = make_sequence(3, 64, 3, seed=3, outdoor=False)
    mask = torch.rand(3, 64, 3).softmax(-1)
    assert vote.mask_voting(pc, mask, flows).shape == (3, 64, 3)
    assert vote.vote_batch(pc, mask, torch.cat([flows, flows[:1]]), n_frame=3).shape == (3, 64, 3)


def test_library_exports_the_entry_point():
    from ogc_amd import _lib, pointnet2_cuda
    from ogc_amd.csrc import build as b
    lib = ctypes.CDLL(b.build())
    assert hasattr(lib, "ogc_soft_carry")
    assert "soft_carry.hip" in b.SOURCES
    f, i, p = ctypes.c_float, ctypes.c_int, ctypes.c_void_p
    assert _lib.SIGNATURES["ogc_soft_carry"] == [i, i, i, i, f, p, p, p, p, p]
    assert callable(pointnet2_cuda.soft_carry_wrapper)
    header = open(os.path.join(ROOT, "include", "ogc_ops.h")).read()
    proto = re.search(r"int ogc_soft_carry\(([^)]*)\);", header)
    assert proto is not None
    kinds = [("p" if "*" in a or "ogc_stream_t" in a else "f" if "float" in a else "i") for a in proto.group(1).split(",")]
    assert "".join(kinds) == "iiiifppppp"
    assert int(re.search(r"#define OGC_VERSION (\d+)", header).group(1)) == _lib.HEADER_VERSION

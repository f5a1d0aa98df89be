"""ogc_soft_carry (csrc/soft_carry.hip) — out = softmax_rows(-cdist(p1, p2) / temperature) @ x without the (n1, n2) matrix — and
the voting built on it: the kernel against the op sequence in fp64 with torch's own fp32 as the yardstick, its memory contract
(guard bands, batch independence), voting on inputs whose slot alignment is decided, the batch over scenes, the memory peak
and the data-set driver on the device."""
import itertools
import math
import os

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAU = 0.01


def _inputs(shape, scale, seed=None):
    """Queries are noisy copies (sigma = 0.02) of candidates; x holds softmax rows and a last column of ones."""
    B, N1, N2, C = shape
    g = torch.Generator().manual_seed(sum(shape) + int(scale) if seed is None else seed)
    p2 = ((torch.rand(B, N2, 3, generator=g) - 0.5) * scale).cuda()
    src = torch.randint(0, N2, (B, N1), generator=g).cuda()
    p1 = torch.gather(p2, 1, src.unsqueeze(-1).expand(-1, -1, 3)) + 0.02 * torch.randn(B, N1, 3, generator=g).cuda()
    soft = torch.randn(B, N2, max(C - 1, 1), generator=g).cuda().mul(3).softmax(-1)[:, :, :C - 1]
    x = torch.cat([soft, torch.ones(B, N2, 1, device="cuda")], -1)
    return p1.contiguous(), p2.contiguous(), x.contiguous()


def _ref(p1, p2, x, dtype):
    return (-torch.cdist(p1.to(dtype), p2.to(dtype)) / TAU).softmax(-1) @ x.to(dtype)


def _run(p1, p2, x):
    from ogc_amd import pointnet2_cuda as nat
    B, N1, N2, C = p1.shape[0], p1.shape[1], p2.shape[1], x.shape[2]
    out = torch.full((B, N1, C), float("nan"), device="cuda")
    nat.soft_carry_wrapper(B, N1, N2, C, TAU, p1, p2, x, out)
    return out


# every operand width of the kernel (16 / 32 / 48 / 64 columns) from both sides, ragged sizes, one tile of candidates, and the
# column split of the wrapper (100 columns); the entry point has no size threshold
SHAPES = [(2, 300, 257, 6), (1, 1024, 1500, 11), (3, 64, 64, 16), (3, 64, 64, 17), (2, 700, 90, 33), (1, 130, 2049, 48),
          (1, 130, 2049, 49), (1, 33, 1000, 64), (1, 17, 16, 1), (2, 200, 300, 100)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("scale", [1.0, 40.0])
def test_kernel_against_the_op_sequence(shape, scale):
    p1, p2, x = _inputs(shape, scale)
    out = _run(p1, p2, x)
    exact, single = _ref(p1, p2, x, torch.float64), _ref(p1, p2, x, torch.float32)
    err_kernel = (out.double() - exact).abs().max().item()
    err_torch = (single.double() - exact).abs().max().item()
    ones = (out[..., -1] - 1.0).abs().max().item()
    print("soft carry %s scale %g: max |kernel - fp64| %.3e, max |torch fp32 - fp64| %.3e, ones column off by %.3e"
          % (shape, scale, err_kernel, err_torch, ones))
    assert err_kernel <= max(4.0 * err_torch, 1e-5 * x.abs().max().item()), (err_kernel, err_torch)
    assert ones <= 1e-5


def test_guard_bands():
    """The last sample's buffers end inside larger allocations: behind p2 lie points that coincide with queries, behind x lies
    1e6, behind out a sentinel.  A read or write past the end changes the result or the sentinel."""
    from ogc_amd import pointnet2_cuda as nat
    B, N1, N2, C, PAD = 2, 203, 149, 21, 97
    p1, p2, x = _inputs((B, N1, N2, C), 1.0, seed=77)
    want = _run(p1, p2, x)
    big_p1 = torch.full((B * N1 + PAD, 3), 7.0, device="cuda")
    big_p2 = torch.empty(B * N2 + PAD, 3, device="cuda")
    big_x = torch.full((B * N2 + PAD, C), 1e6, device="cuda")
    big_out = torch.full((B * N1 + PAD, C), -12345.0, device="cuda")
    big_p1[:B * N1] = p1.reshape(-1, 3)
    big_p2[:B * N2] = p2.reshape(-1, 3)
    big_p2[B * N2:] = p1[-1, :PAD]                       # candidates that would win if they were read
    big_x[:B * N2] = x.reshape(-1, C)
    nat.soft_carry_wrapper(B, N1, N2, C, TAU, big_p1[:B * N1].view(B, N1, 3), big_p2[:B * N2].view(B, N2, 3),
                           big_x[:B * N2].view(B, N2, C), big_out[:B * N1].view(B, N1, C))
    torch.cuda.synchronize()
    assert torch.equal(big_out[:B * N1].view(B, N1, C), want)
    assert bool((big_out[B * N1:] == -12345.0).all())


def test_batch_independence():
    p1, p2, x = _inputs((5, 131, 277, 27), 1.0, seed=5)
    together = _run(p1, p2, x)
    for i in range(5):
        alone = _run(p1[i:i + 1].contiguous(), p2[i:i + 1].contiguous(), x[i:i + 1].contiguous())
        assert torch.equal(alone[0], together[i]), i


# ---- voting -----------------------------------------------------------------------------------------------------------------
CASES = [(4, 300, 5, 11), (4, 300, 5, 12), (2, 257, 6, 13), (5, 200, 4, 14), (3, 333, 6, 15)]
WINDOW = 3


def _scene(T, N, K, seed):
    """A sequence whose masks are three logits clear of noise, every frame's slots in an order of its own."""
    from ogc_amd.utils.synthetic import make_sequence
    pc, segm, flows = make_sequence(T, N, K, seed=seed, outdoor=False)
    g = torch.Generator().manual_seed(seed + 1)
    mask = (3.0 * torch.eye(K)[segm] + torch.randn(T, N, K, generator=g)).softmax(-1)
    mask = torch.stack([mask[t][:, torch.randperm(K, generator=g)] for t in range(T)])
    return pc.cuda(), mask.cuda().contiguous(), flows.cuda()


def _dense_voting(pc, mask, flows, window, dtype):
    """The reference's voting on collect_correspondences in `dtype`, the assignment by enumeration -> (voted masks,
    {(t, v): chosen columns}, {(t, v): second-best minus best total cost}) — the margins over ALL frame pairs."""
    from ogc_amd import vote
    pc, mask, flows = pc.to(dtype), mask.to(dtype), flows.to(dtype)
    T, N, K = mask.shape
    corrs = vote.collect_correspondences(pc, flows)
    perms = torch.tensor(list(itertools.permutations(range(K))), device=pc.device)
    rows = torch.arange(K, device=pc.device)
    chosen, margin, voted = {}, {}, []
    for t in range(T):
        votes = []
        for v in range(T):
            if v == t:
                votes.append(mask[t])
                continue
            other = corrs["%d_%d" % (t, v)][0].to(dtype) @ mask[v]
            cost = -(torch.log(mask[t]).clamp_min(-100.0).t() @ other + torch.log1p(-mask[t]).clamp_min(-100.0).t() @ (1.0 - other)) / N
            total = cost[rows, perms].sum(-1)
            best = torch.argsort(total)
            chosen[(t, v)] = perms[best[0]].tolist()
            margin[(t, v)] = (total[best[1]] - total[best[0]]).item()
            if abs(t - v) <= window:
                votes.append(other[:, perms[best[0]]])
        m = torch.stack(votes).mean(0)
        voted.append(m / m.sum(-1, keepdim=True).clamp(1e-10))
    return torch.stack(voted), chosen, margin


@pytest.mark.parametrize("T,N,K,seed", CASES)
def test_voting_on_decided_inputs(T, N, K, seed, monkeypatch):
    from ogc_amd import vote
    pc, mask, flows = _scene(T, N, K, seed)
    exact, chosen, margin = _dense_voting(pc, mask, flows, WINDOW, torch.float64)
    print("voting (T %d, N %d, K %d, seed %d): smallest assignment margin in fp64 %.4f" % (T, N, K, seed, min(margin.values())))
    assert min(margin.values()) >= 0.01, margin          # decided: no pair's alignment is a coin toss
    single, _, _ = _dense_voting(pc, mask, flows, WINDOW, torch.float32)
    seen = []
    assign = vote._assign_columns
    monkeypatch.setattr(vote, "_assign_columns", lambda score: seen.append(assign(score)) or seen[-1])
    got = vote.mask_voting(pc, mask, flows, time_window_size=WINDOW)
    assert len(seen) == 1                                # one assignment launch for the whole call
    pairs = sorted((t, v) for t in range(T) for v in range(T) if v != t and abs(t - v) <= WINDOW)
    assert seen[0].shape == (1, len(pairs), K)
    for i, p in enumerate(pairs):
        assert seen[0][0, i].tolist() == chosen[p], (p, seen[0][0, i].tolist(), chosen[p])
    err_fused = (got.double() - exact).abs().max().item()
    err_dense = (single.double() - exact).abs().max().item()
    print("    max |fused - fp64| %.3e, max |dense fp32 - fp64| %.3e" % (err_fused, err_dense))
    assert err_fused <= max(4.0 * err_dense, 1e-5), (err_fused, err_dense)
    assert torch.allclose(got.sum(-1), torch.ones(T, N, device="cuda"), atol=1e-5)


def test_vote_batch_over_scenes_equals_the_single_calls():
    from ogc_amd import vote
    scenes = [_scene(4, 300, 5, seed) for seed in (11, 12, 16)]
    pc = torch.cat([s[0] for s in scenes])
    mask = torch.cat([s[1] for s in scenes])
    # the loader's flows: one (forward, backward) entry per frame, the last of every scene redundant
    flows = torch.cat([torch.cat([s[2], torch.full_like(s[2][:1], 9.0)]) for s in scenes])
    got = vote.vote_batch(pc, mask, flows, n_frame=4, time_window_size=WINDOW)
    assert got.shape == (12, 300, 5)
    for i, (p, m, f) in enumerate(scenes):
        assert torch.equal(got[4 * i:4 * i + 4], vote.mask_voting(p, m, f, time_window_size=WINDOW)), i


def test_no_n_by_n_tensor():
    """Two frames of 8192 points, 10 slots (KITTI-SF): the peak stays within an eighth of ONE 8192 x 8192 fp32 matrix."""
    from ogc_amd import vote
    from ogc_amd.utils.synthetic import make_sequence
    pc, segm, flows = make_sequence(2, 8192, 10, seed=31, outdoor=True, device="cuda")
    mask = (3.0 * torch.eye(10, device="cuda")[segm] + torch.randn(2, 8192, 10, device="cuda")).softmax(-1)
    vote.mask_voting(pc[:, :64].contiguous(), mask[:, :64].contiguous(), flows[:, :, :64].contiguous())   # (library handles)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    voted = vote.mask_voting(pc, mask, flows, time_window_size=3)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    print("mask_voting at 2 x 8192 x 10: %.2f MiB above its inputs" % (extra / 2 ** 20))
    assert extra < 32 * 2 ** 20
    assert torch.isfinite(voted).all() and torch.allclose(voted.sum(-1), torch.ones(2, 8192, device="cuda"), atol=1e-5)


def test_driver_on_the_device(tmp_path, capsys):
    """The OGC-DR synthetic configuration (4 frames x 4096 points, 8 slots; random weights where there is no checkpoint) on a
    root of its own."""
    from ogc_amd import vote
    with open(os.path.join(ROOT, "config", "ogcdr_unsup_synthetic.yaml")) as f:
        cfg = yaml.safe_load(f)
    root = str(tmp_path / "data")
    os.makedirs(root)
    cfg["data"] = {"root": root, "decentralize": True}
    cfg["save_path"] = str(tmp_path / "no_checkpoint")
    path = str(tmp_path / "cfg.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    res = vote.main([path, "--split", "val", "--synthetic", "2", "--use_gt_flow", "--save", "--test_batch_size", "8",
                     "--num_workers", "0"])
    assert res["save_dir"] == os.path.join(root, "segm_preds", "Vote_T3")
    for scene in ("00000000", "00000001"):
        for k in range(4):
            lab = np.load(os.path.join(root, "segm_preds", "Vote_T3", scene, "segm_%02d.npy" % k))
            assert lab.shape == (4096,) and lab.dtype == np.int64 and 0 <= lab.min() and lab.max() < 8
    keys = {"AP", "PQ", "F1", "Pre", "Rec", "per_scan_iou_avg", "per_scan_iou_std", "per_scan_ri_avg", "per_scan_ri_std"}
    for kind in ("voted", "raw"):
        assert set(res[kind]) == keys
        assert all(math.isfinite(v) for v in res[kind].values()), res[kind]
    out = capsys.readouterr().out
    assert "Evaluation on ogcdr-val:" in out and "AveragePrecision@50:" in out and "Without voting:" in out

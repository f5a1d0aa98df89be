"""Multi-frame co-segmentation by voting (reference: vote.py:17-131) and its evaluation driver (:134-352).

The masks a network predicts for the T frames of a sequence are made consistent over time: every frame collects the
masks of the frames inside its time window, carried over by soft point correspondences (softmax of the negative
distance between the flow-warped frame and the other frame, chained over intermediate frames), aligned in slot order
by a Hungarian match, and averaged.

`pairwise_correspondence`, `collect_correspondences`, `match_mask_by_cost` and `mask_voting` keep the reference's
signatures and results.  What differs underneath:
  * `mask_voting` never forms the chained (N, N) correspondence products (O(N^3) each, vote.py:52-58): only their action
    on the (N, K) masks is needed, and  normalise(A @ B) @ X = (A @ (B @ X)) / clamp(A @ (B @ 1))  gets it with
    matrix-times-thin-matrix products — the normalisers ride along as an extra column.
  * the slot alignment runs on the device (ogc_lsap_maximize, scipy's tie-breaking) instead of a host round trip per
    frame pair, and its cross-entropy cost is two (K, N) x (N, K) products instead of an (N, K, K) tensor.
  * on CUDA float32 inputs `mask_voting` and `vote_batch` never form an (N, N) correspondence either: every adjacent frame pair
    is applied once per call, to all the columns that cross it and to all scenes of the batch, by ogc_soft_carry
    (csrc/soft_carry.hip; `_vote_scenes`), and all slot alignments of the call are one assignment launch.
Run as a module it is the reference's quantitative mode on this package's data-set readers,

    python -m ogc_amd.vote CONFIG --split S [--round R] [--test_batch_size 64] [--time_window_size 3] [--use_gt_flow] [--save]
                                  [--mapping FILE] [--synthetic N] [--num_workers 4] [--device cuda]

for sapien, ogcdr, kittisf and kittidet: view selections, frames per scene, ignore threshold, checkpoint and flow source
(`predflow_path` of the config, `_R<round-1>` appended from round 2 on; none with --use_gt_flow) are the reference's, the
metrics of the voted and of the raw masks come from the device evaluation kernel as in test_seg, and --save writes the voted
labels under <root>/segm_preds/Vote_T<window>.  `--synthetic N` runs on N scenes written into a temporary root.  Left out:
`--visualize` (needs open3d).  Without --split it evaluates with and without voting on in-memory synthetic sequences
(`python -m ogc_amd.vote <config> --round R`), printing the reference's metrics (AP, PQ, F1, Pre, Rec, mIoU, RI).
"""
import argparse
import os

import numpy as np
import torch

from .losses.seg_loss_unsup import _assign_columns


def pairwise_correspondence(pc1, pc2, flow, temperature=0.01):
    """pc1, pc2, flow (B, N, 3) -> soft correspondence (B, N1, N2), rows sum to one.  Reference: vote.py:17-28."""
    return (-torch.cdist(pc1 + flow, pc2) / temperature).softmax(-1)


def _adjacent(pc, flows):
    """{(t, t+1), (t+1, t)} -> (N, N) correspondence of every adjacent frame pair (vote.py:47-49)."""
    adj = {}
    for t in range(pc.size(0) - 1):
        adj[(t, t + 1)] = pairwise_correspondence(pc[t:t + 1], pc[t + 1:t + 2], flows[t:t + 1, 0])[0]
        adj[(t + 1, t)] = pairwise_correspondence(pc[t + 1:t + 2], pc[t:t + 1], flows[t:t + 1, 1])[0]
    return adj


def collect_correspondences(pc, flows):
    """pc (T, N, 3), flows (T-1, 2, N, 3) [forward flow of frame t, backward flow of frame t+1] -> dict
    '%d_%d' % (a, b) -> (1, N, N) for all frame pairs, as the reference builds it (vote.py:31-60): identity, adjacent
    pairs from the flows, longer spans by chaining and re-normalising the rows."""
    n_frame, n_point, _ = pc.size()
    corrs = {}
    eye = torch.eye(n_point, device=pc.device).unsqueeze(0)
    for t in range(n_frame):
        corrs['%d_%d' % (t, t)] = eye
    for (a, b), m in _adjacent(pc, flows).items():
        corrs['%d_%d' % (a, b)] = m.unsqueeze(0)
    for interval in range(2, n_frame):
        for t in range(0, n_frame - interval):
            corr = torch.bmm(corrs['%d_%d' % (t, t + interval - 1)], corrs['%d_%d' % (t + interval - 1, t + interval)])
            corrs['%d_%d' % (t, t + interval)] = corr / corr.sum(-1, keepdim=True).clamp(1e-10)
            corr = torch.bmm(corrs['%d_%d' % (t + interval, t + interval - 1)], corrs['%d_%d' % (t + interval - 1, t)])
            corrs['%d_%d' % (t + interval, t)] = corr / corr.sum(-1, keepdim=True).clamp(1e-10)
    return corrs


def _carry(adj, t, v, x):
    """corrs['t_v'] @ x without the (N, N) chain:  x (N, c) lives on frame v, the result on frame t.
    Forward spans are nested from the left, corr(t, v) = norm(corr(t, v-1) @ adj(v-1, v)); backward spans from the
    right, corr(t, v) = norm(adj(t, t-1) @ corr(t-1, v))   (vote.py:53-58)."""
    if abs(t - v) == 1:
        return adj[(t, v)] @ x
    ones = torch.ones(x.size(0), 1, dtype=x.dtype, device=x.device)
    c = x.size(1)
    if v > t:
        z = _carry(adj, t, v - 1, adj[(v - 1, v)] @ torch.cat([x, ones], 1))
    else:
        z = adj[(t, t - 1)] @ _carry(adj, t - 1, v, torch.cat([x, ones], 1))
    return z[:, :c] / z[:, c:].clamp(1e-10)


def match_mask_by_cost(mask1, mask2, measure='ce'):
    """mask1, mask2 (N, K) -> mask2 with its slots re-ordered to match mask1: Hungarian on the mean binary cross
    entropy (input mask1, target mask2) or on the soft IoU.  Reference: vote.py:63-92."""
    n_object = mask1.shape[-1]
    if measure == 'ce':
        # mean_n BCE(mask1[n, i], mask2[n, j]) with torch's clamp of the logarithms at -100
        log_p = torch.log(mask1).clamp_min(-100.0)
        log_q = torch.log1p(-mask1).clamp_min(-100.0)
        cost = -(log_p.t() @ mask2 + log_q.t() @ (1.0 - mask2)) / mask1.shape[0]
        col_ind = _assign_columns(-cost)
    else:
        intersection = mask1.t() @ mask2
        union = mask1.sum(0).unsqueeze(1) + mask2.sum(0).unsqueeze(0)
        col_ind = _assign_columns(intersection / union.clamp(1e-10))
    perm = torch.eye(n_object, dtype=torch.float32, device=mask2.device)[col_ind]
    return torch.einsum('ij,nj->ni', perm, mask2)


def _native_carry(temperature=0.01):
    """carry(p1 (S, N1, 3), p2 (S, N2, 3), x (S, N2, c)) -> softmax_rows(-cdist(p1, p2) / temperature) @ x through the native's
    soft_carry_wrapper (ogc_soft_carry: nothing of size N1 x N2 is stored), or None when the native has none (the CPU oracle)."""
    from .pointnet2 import pointnet2 as _api
    fused = getattr(_api._native, "soft_carry_wrapper", None)
    if fused is None:
        return None

    def carry(p1, p2, x):
        p1, p2, x = p1.contiguous(), p2.contiguous(), x.contiguous()
        out = torch.empty(x.size(0), p1.size(1), x.size(2), dtype=torch.float32, device=x.device)
        fused(x.size(0), p1.size(1), p2.size(1), x.size(2), temperature, p1, p2, x, out)
        return out
    return carry


def _fusable(*tensors):
    return all(t.is_cuda and t.dtype == torch.float32 and not t.requires_grad for t in tensors)


def _vote_scenes(pc, mask, flows, time_window_size, carry):
    """mask_voting of S scenes at once: pc (S, T, N, 3), mask (S, T, N, K), flows (S, T-1, 2, N, 3) -> (S, T, N, K), with every
    adjacent-pair correspondence applied ONCE, through `carry` (see _native_carry), to all the columns that cross it:
      forward spans (v > t):  corr(t, v) is nested from the left (vote.py:53-55), so its normalisers all sit on frame t's rows and
        the recursion is linear:  W_s = adj(s, s+1) @ [W_{s+1}, 1],  W_v = mask[v]  — the ones are left out of the last product
        of a span's longest reach, where nothing would read them.  corr(t, v) @ mask[v] is read off W_t by _carry's nested
        z[:, :c] / z[:, c:].clamp(1e-10).  The W of every v inside the window ride through adj(s, s+1) side by side.
      backward spans (v < t):  corr(s, v) = norm(adj(s, s-1) @ corr(s-1, v)) normalises frame by frame, so what is carried is
        [corr(s, v) @ mask[v], corr(s, v) @ 1], divided by its own last column after every step, again for all v at once.
    2 (T - 1) launches of the correspondence kernel and one of the assignment kernel, whatever S."""
    S, T, N, K = mask.shape
    w = int(time_window_size)
    if T == 1 or w < 1:
        return mask / mask.sum(-1, keepdim=True).clamp(1e-10)
    ones = mask.new_ones(S, N, 1)
    carried = {}                                    # (t, v) -> corr(t, v) @ mask[v], (S, N, K)
    live = {}                                       # forward: v -> W_{s+1} of span target v
    for s in range(T - 2, -1, -1):
        live[s + 1] = mask[:, s + 1]
        vs = list(range(s + 1, min(T - 1, s + w) + 1))
        cols = [live[v] if s == max(0, v - w) else torch.cat([live[v], ones], -1) for v in vs]
        out = carry(pc[:, s] + flows[:, s, 0], pc[:, s + 1], torch.cat(cols, -1))
        live = dict(zip(vs, out.split([c.size(-1) for c in cols], -1)))
        for v in vs:
            z = live[v][..., :K + (v - s) - 1]
            while z.size(-1) > K:
                z = z[..., :-1] / z[..., -1:].clamp(1e-10)
            carried[(s, v)] = z
    live = {}                                       # backward: v -> [corr(s-1, v) @ mask[v], corr(s-1, v) @ 1]
    for s in range(1, T):
        vs = list(range(max(0, s - w), s))
        goes_on = s + 1 <= T - 1 and w >= 2         # frame s+1 votes with frame s-1 through this product
        cols = [live[v] if v < s - 1 else (torch.cat([mask[:, v], ones], -1) if goes_on else mask[:, v]) for v in vs]
        out = carry(pc[:, s] + flows[:, s - 1, 1], pc[:, s - 1], torch.cat(cols, -1))
        live = {}
        for v, z in zip(vs, out.split([c.size(-1) for c in cols], -1)):
            if v < s - 1:
                z = z / z[..., K:].clamp(1e-10)
            carried[(s, v)], live[v] = z[..., :K], z
    # slot alignment of every (t, v) pair of every scene: one batched cost, one assignment launch
    pairs = sorted(carried)
    t_of = torch.tensor([t for t, _ in pairs], device=mask.device)
    other = torch.stack([carried[p] for p in pairs], 1)                                    # (S, P, N, K)
    log_p = torch.log(mask).clamp_min(-100.0)[:, t_of].transpose(-1, -2)                   # (S, P, K, N)
    log_q = torch.log1p(-mask).clamp_min(-100.0)[:, t_of].transpose(-1, -2)
    cost = -(log_p @ other + log_q @ (1.0 - other)) / N
    perm = torch.eye(K, dtype=torch.float32, device=mask.device)[_assign_columns(-cost)]   # (S, P, K, K)
    aligned = torch.einsum('spij,spnj->spni', perm, other)
    where = {p: i for i, p in enumerate(pairs)}
    voted = []
    for t in range(T):
        vs = range(max(0, t - w), min(T, t + w + 1))
        total = None
        for v in vs:                                # summed one by one: the same bits whatever S
            m = mask[:, t] if v == t else aligned[:, where[(t, v)]]
            total = m if total is None else total + m
        vote = total / len(vs)
        voted.append(vote / vote.sum(-1, keepdim=True).clamp(1e-10))
    return torch.stack(voted, 1)


def mask_voting(pc, mask, flows, time_window_size=3):
    """pc (T, N, 3), mask (T, N, K), flows (T-1, 2, N, 3) -> voted masks (T, N, K).  Reference: vote.py:95-131.
    CUDA float32 inputs go through the fused correspondence kernel (_vote_scenes); everything else through the dense
    (N, N) correspondences below."""
    n_frame = pc.size(0)
    carry = _native_carry() if _fusable(pc, mask, flows) else None
    if carry is not None:
        return _vote_scenes(pc[None], mask[None], flows[None], time_window_size, carry)[0]
    adj = _adjacent(pc, flows)
    voted = []
    for t in range(n_frame):
        votes = []
        for v in range(max(0, t - time_window_size), min(n_frame, t + time_window_size + 1)):
            if v == t:
                votes.append(mask[t])
            else:
                votes.append(match_mask_by_cost(mask[t], _carry(adj, t, v, mask[v])))
        vote = torch.stack(votes, 0).mean(0)
        voted.append(vote / vote.sum(-1, keepdim=True).clamp(1e-10))
    return torch.stack(voted, 0)


def vote_batch(pc, mask, flows, n_frame, time_window_size=3):
    """The evaluation loop's inner step (vote.py:302-310): the batch holds whole scenes of `n_frame` consecutive
    frames; `flows` is the loader's (B, 2, N, 3) [forward, backward] tensor of which the last entry of every scene is
    redundant.  CUDA float32 inputs: all scenes ride in the batch dimension of the fused kernel (_vote_scenes)."""
    n_scene = pc.size(0) // n_frame
    carry = _native_carry() if _fusable(pc, mask, flows) and n_scene > 0 else None
    if carry is not None:
        shape = (n_scene, n_frame)
        used = n_scene * n_frame
        voted = _vote_scenes(pc[:used].reshape(shape + pc.shape[1:]), mask[:used].reshape(shape + mask.shape[1:]),
                             flows[:used].reshape(shape + flows.shape[1:])[:, :n_frame - 1], time_window_size, carry)
        return voted.reshape((used,) + mask.shape[1:])
    out = []
    for sid in range(pc.size(0) // n_frame):
        lo, hi = n_frame * sid, n_frame * (sid + 1)
        out.append(mask_voting(pc[lo:hi], mask[lo:hi], flows[lo:hi - 1].contiguous(), time_window_size))
    return torch.cat(out, 0)


def evaluate_voting(segnet, sequences, n_frame, time_window_size=3, ignore_npoint_thresh=0, device="cuda"):
    """Metrics of the raw and the voted masks over an iterable of (pc (T,N,3), segm (T,N), flows (T-1,2,N,3))
    sequences.  Returns {'raw': {...}, 'voted': {...}} with AP, PQ, F1, Pre, Rec, mIoU, RI (vote.py:284-352)."""
    from .metrics.seg_metric import ClusteringMetrics, accumulate_eval_results, calculate_AP, calculate_PQ_F1
    clustering = ClusteringMetrics()
    acc = {k: {'iou': [], 'matched': [], 'conf': [], 'n_gt': 0, 'miou': [], 'ri': []} for k in ('raw', 'voted')}
    segnet.eval()
    for pc, segm, flows in sequences:
        pc, segm, flows = pc.to(device), segm.to(device), flows.to(device)
        with torch.no_grad():
            mask = segnet(pc, pc).detach()
            both = {'raw': mask, 'voted': mask_voting(pc, mask, flows, time_window_size)}
        for key, m in both.items():
            a = acc[key]
            iou, matched, conf, n_gt = accumulate_eval_results(segm, m, ignore_npoint_thresh)
            a['iou'].append(iou); a['matched'].append(matched); a['conf'].append(conf); a['n_gt'] += n_gt
            scan = clustering(m, segm.long(), ignore_npoint_thresh)
            a['miou'].append(np.mean(scan['iou'])); a['ri'].append(np.mean(scan['ri']))
    out = {}
    for key, a in acc.items():
        iou, matched, conf = (np.concatenate(a[k]) for k in ('iou', 'matched', 'conf'))
        pq, f1, pre, rec = calculate_PQ_F1(iou, matched, a['n_gt'])
        out[key] = {'AP': calculate_AP(matched, conf, a['n_gt']), 'PQ': pq, 'F1': f1, 'Pre': pre, 'Rec': rec,
                    'mIoU': float(np.mean(a['miou'])), 'RI': float(np.mean(a['ri']))}
    return out


class _SegMeter:
    """What the reference's loop accumulates for one kind of mask (vote.py:294-335, :341-353).  On the device: seg_eval_batch /
    accumulate_seg_eval as in test_seg.evaluate (one small device->host copy per batch, no soft masks on the host); on the CPU
    the reference-shaped functions of metrics/seg_metric.py."""

    def __init__(self, n_frame, ignore_npoint_thresh):
        from .utils.pytorch_util import AverageMeter
        self.n_frame, self.thresh = n_frame, ignore_npoint_thresh
        self.meter = AverageMeter()
        self.iou, self.matched, self.conf, self.n_gt = [], [], [], 0

    def add(self, segm, mask):
        """segm (B, N), mask (B, N, K) -> hard labels (B, N)."""
        if mask.is_cuda:
            from .metrics.seg_eval import accumulate_seg_eval, seg_eval_batch
            result = seg_eval_batch(segm, mask, self.thresh)
            iou, matched, conf, n_gt, miou, ri = accumulate_seg_eval(segm, mask, self.thresh, result=result)
            hard = result.hard
            if bool((result.status != 0).any()):    # labels beyond the kernel's table: its arg-max of that sample is zeroed
                hard = torch.where(result.status[:, None] != 0, mask.argmax(dim=2).to(torch.int32), hard)
        else:
            from .metrics.seg_metric import ClusteringMetrics, accumulate_eval_results
            iou, matched, conf, n_gt = accumulate_eval_results(segm, mask, self.thresh)
            scan = ClusteringMetrics()(mask, segm.long(), self.thresh)
            miou, ri = np.asarray(scan['iou']), np.asarray(scan['ri'])
            hard = mask.argmax(dim=2)
        self.iou.append(iou); self.matched.append(matched); self.conf.append(conf); self.n_gt += n_gt
        for sid in range(segm.shape[0] // self.n_frame):
            scan = slice(self.n_frame * sid, self.n_frame * (sid + 1))
            self.meter.append_loss({'per_scan_iou_avg': np.mean(miou[scan]), 'per_scan_iou_std': np.std(miou[scan]),
                                    'per_scan_ri_avg': np.mean(ri[scan]), 'per_scan_ri_std': np.std(ri[scan])})
        return hard

    def result(self):
        from .metrics.seg_metric import calculate_AP, calculate_PQ_F1
        iou, matched, conf = np.concatenate(self.iou), np.concatenate(self.matched), np.concatenate(self.conf)
        pq, f1, pre, rec = calculate_PQ_F1(iou, matched, self.n_gt)
        out = {'AP': float(calculate_AP(matched, conf, self.n_gt)), 'PQ': float(pq), 'F1': float(f1), 'Pre': float(pre),
               'Rec': float(rec)}
        out.update(self.meter.get_mean_loss_dict())
        return out


def evaluate_dataset(segnet, loader, n_frame, ignore_npoint_thresh, time_window_size=3, saver=None, device='cuda'):
    """The reference's quantitative loop (vote.py:284-353).  loader yields (pcs, segms, flows, valids) with the n_frame samples
    of a scene adjacent in one batch; saver(hard (B, N) labels of the voted masks, batch index) stores the predictions.
    -> {'raw': {...}, 'voted': {...}}, each with AP, PQ, F1, Pre, Rec and per_scan_{iou,ri}_{avg,std}."""
    meters = {key: _SegMeter(n_frame, ignore_npoint_thresh) for key in ('raw', 'voted')}
    n_batches = 0
    for i, batch in enumerate(loader):
        pcs, segms, flows = batch[0], batch[1], batch[2]
        pc = pcs[:, 0].contiguous().to(device)
        segm = segms[:, 0].contiguous().to(device)
        if segm.shape[0] % n_frame != 0:
            raise ValueError("a batch of %d samples does not hold whole scenes of %d frames" % (segm.shape[0], n_frame))
        with torch.no_grad():
            mask = segnet(pc, pc).detach().float()
            voted = vote_batch(pc, mask, flows.to(device).float(), n_frame, time_window_size)
        meters['raw'].add(segm, mask)
        hard = meters['voted'].add(segm, voted)
        if saver is not None:
            saver(hard, i)
        n_batches += 1
    if n_batches == 0:
        raise ValueError("the data set is empty")
    return {key: m.result() for key, m in meters.items()}


def _write_synthetic_root(cfg, split, n_scenes, data_root, predflow):
    """A temporary root in the layout `dataset`'s reader takes (utils/synthetic.py) -> path of the split file or None."""
    from .utils import synthetic
    name, data = cfg['dataset'], cfg.get('data') or {}
    n_points, n_objects = data.get('n_points', cfg['segnet']['n_point']), data.get('n_objects', 3)
    if name == 'ogcdr':
        synthetic.write_ogcdr_root(data_root, n_scenes, n_points, n_objects=n_objects, split=split)
    elif name == 'sapien':
        sub = os.path.join(data_root, 'mbs-sapien' if split == 'test' else 'mbs-shapepart')
        os.makedirs(sub, exist_ok=True)
        synthetic.write_sapien_root(sub, n_scenes, n_points, n_parts=n_objects, split=split)
    elif name == 'kittisf':
        full = os.path.join(data_root, 'full')
        synthetic.write_kitti_processed_root(full, n_scenes, 2 * n_points, split=split)
        return synthetic.write_kitti_downsampled_root(full, data_root, n_points, predflow=predflow, split=split)[0]
    else:
        return synthetic.write_labelled_root(data_root, 'kittidet', n_scenes, n_points, n_objects, split=split)[0]
    return None


def build_vote_set(cfg, split, data_root, mapping=None, predflow_path=None):
    """test_seg.build_test_set with the flow source of voting (vote.py:198-232): with `predflow_path` the flows of the
    multi-frame sets come from <root>/flow_preds/<predflow_path> instead of the ground truth.
    -> (data set, n_frame, ignore_npoint_thresh, data root as the data set sees it)."""
    from . import datasets, test_seg
    name = cfg['dataset']
    if predflow_path is None or name not in ('sapien', 'ogcdr', 'kittisf'):
        return test_seg.build_test_set(cfg, split, data_root, mapping)
    data = cfg.get('data') or {}
    decentralize = bool(data.get('decentralize', False))
    if name == 'kittisf':
        if mapping is None:
            mapping = data.get('val_mapping' if split == 'val' else 'train_mapping') or os.path.join(data_root, split + '.txt')
        return (datasets.KITTISceneFlowDataset(data_root=data_root, mapping_path=mapping, downsampled=True,
                                               view_sels=test_seg.KITTISF_VIEW_SELS, predflow_path=predflow_path,
                                               decentralize=decentralize),
                len(test_seg.KITTISF_VIEW_SELS), test_seg.OUTDOOR_IGNORE_NPOINT_THRESH, data_root)
    if name == 'sapien':
        data_root = os.path.join(data_root, 'mbs-sapien' if split == 'test' else 'mbs-shapepart')
    cls = datasets.SapienDataset if name == 'sapien' else datasets.OGCDynamicRoomDataset
    return (cls(data_root=data_root, split=split, view_sels=test_seg.INDOOR_VIEW_SELS, predflow_path=predflow_path,
                decentralize=decentralize), len(test_seg.INDOOR_VIEW_SELS), 0, data_root)


def _main_dataset(args, cfg):
    """The reference's quantitative mode (vote.py:152-232, :284-353) on this package's readers."""
    import json
    import shutil
    import tempfile
    from . import test_seg
    name = cfg['dataset']
    if name not in ('sapien', 'ogcdr', 'kittisf', 'kittidet'):
        raise KeyError('Unrecognized dataset %r' % name)
    device = torch.device(args.device)
    data = cfg.get('data') or {}
    if args.use_gt_flow or name == 'kittidet':      # (single frames: there is no flow to read)
        predflow = None
    elif not cfg.get('predflow_path'):
        raise ValueError("the config names no predflow_path: name the predicted flows there, or vote with --use_gt_flow")
    else:
        predflow = cfg['predflow_path'] + ('_R%d' % (args.round - 1) if args.round > 1 else '')

    torch.manual_seed(cfg.get('random_seed', 10))
    segnet = test_seg.build_segnet(cfg).to(device)
    path = test_seg.weight_path(cfg, args.round)
    if os.path.isfile(path):
        segnet.load_state_dict(torch.load(path, map_location='cpu')['model_state'])
        print('Loaded weights from %s' % path, flush=True)
    elif args.synthetic:
        print('No checkpoint at %s: random weights' % path, flush=True)
    else:
        raise FileNotFoundError('no checkpoint at %s' % path)
    segnet.eval()

    tmp, mapping = None, args.mapping
    if args.synthetic:
        tmp = tempfile.mkdtemp(prefix='ogc_vote_') if not data.get('root') else None
        data_root = tmp if tmp is not None else data['root']
        mapping = _write_synthetic_root(cfg, args.split, args.synthetic, data_root, predflow)
    else:
        data_root = data['root']
    test_set, n_frame, ignore_npoint_thresh, data_root = build_vote_set(cfg, args.split, data_root, mapping, predflow_path=predflow)
    batch_size = args.test_batch_size
    if batch_size % n_frame != 0:
        raise ValueError('Frames of one scene should be in the same batch, otherwise very inconvenient for evaluation! '
                         '(test_batch_size %d, %d frames)' % (batch_size, n_frame))
    saver, save_dir = None, os.path.join(data_root, 'segm_preds', 'Vote_T%d' % args.time_window_size)
    if args.save:
        os.makedirs(save_dir, exist_ok=True)
        print('Save segmentation predictions into %s ...' % save_dir, flush=True)

        def saver(hard, i):
            test_set._save_predsegm(hard, save_root=save_dir, batch_size=batch_size, n_frame=n_frame, offset=i)
    loader = torch.utils.data.DataLoader(test_set, batch_size=batch_size, shuffle=False, pin_memory=device.type == 'cuda',
                                         num_workers=args.num_workers)
    res = evaluate_dataset(segnet, loader, n_frame, ignore_npoint_thresh, args.time_window_size, saver=saver, device=device)
    voted, raw = res['voted'], res['raw']
    print('Evaluation on %s-%s:' % (name, args.split), flush=True)
    print('AveragePrecision@50: %s' % voted['AP'], flush=True)
    print('PanopticQuality@50: %s F1-score@50: %s Prec@50: %s Recall@50: %s' % (voted['PQ'], voted['F1'], voted['Pre'],
                                                                                  voted['Rec']), flush=True)
    print(json.dumps({k: v for k, v in voted.items() if k.startswith('per_scan')}), flush=True)
    print('Without voting: AveragePrecision@50: %s PanopticQuality@50: %s F1-score@50: %s Prec@50: %s Recall@50: %s mIoU: %s RI: %s'
          % (raw['AP'], raw['PQ'], raw['F1'], raw['Pre'], raw['Rec'], raw['per_scan_iou_avg'], raw['per_scan_ri_avg']), flush=True)
    if args.save:
        res['save_dir'] = save_dir
        print('Saved to %s' % save_dir, flush=True)
    if tmp is not None and not args.save:           # saved predictions stay where the line above says
        shutil.rmtree(tmp, ignore_errors=True)
    return res


def main(argv=None):
    import yaml
    from .utils.synthetic import make_sequence
    ap = argparse.ArgumentParser(description="evaluate a trained segmentation network with multi-frame voting")
    ap.add_argument('config', type=str)
    ap.add_argument('--split', type=str, default=None, help='data set split: evaluate on the data set of the config (without it: '
                                                            'on in-memory synthetic sequences)')
    ap.add_argument('--round', type=int, default=0)
    ap.add_argument('--time_window_size', type=int, default=3)
    ap.add_argument('--test_batch_size', type=int, default=64)
    ap.add_argument('--use_gt_flow', action='store_true', help='vote with the ground-truth flows of the data set')
    ap.add_argument('--save', action='store_true', help='write the voted labels under <root>/segm_preds/Vote_T<window>')
    ap.add_argument('--mapping', default=None, help='kittisf, kittidet: the split file (default data.<split>_mapping, then '
                                                    '<data.root>/<split>.txt)')
    ap.add_argument('--synthetic', type=int, default=0, help='with --split: run on this many synthetic scenes in a temporary root')
    ap.add_argument('--num_workers', type=int, default=4)
    ap.add_argument('--n_frame', type=int, default=4)
    ap.add_argument('--n_sequence', type=int, default=4)
    ap.add_argument('--device', type=str, default='cuda')
    args = ap.parse_args(argv)
    with open(args.config) as f:
        cfg = yaml.safe_load(f)
    if args.split is not None:
        return _main_dataset(args, cfg)
    from .train_seg import build_segnet
    segnet = build_segnet(cfg).to(args.device)
    weight_path = os.path.join(cfg['save_path'] + '_R%d' % args.round, 'best.pth.tar')   # where train_seg writes
    segnet.load_state_dict(torch.load(weight_path, map_location=args.device)['model_state'])
    print('Loaded weights from', weight_path)
    outdoor = cfg['dataset'] in ('kittisf', 'kittidet', 'waymo')
    seqs = (make_sequence(args.n_frame, cfg['segnet']['n_point'], cfg['segnet']['n_slot'], seed=10_000 + i,
                          outdoor=outdoor) for i in range(args.n_sequence))
    res = evaluate_voting(segnet, seqs, args.n_frame, args.time_window_size,
                          ignore_npoint_thresh=50 if outdoor else 0, device=args.device)
    for key in ('raw', 'voted'):
        print('%-5s ' % key + '  '.join('%s %.4f' % kv for kv in res[key].items()))
    return res


if __name__ == '__main__':
    main()

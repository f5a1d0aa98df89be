"""Inputs and oracles shared by the supervised-loss tests and by tests/golden/make_sup_golden.py.

Inputs are built so that the Hungarian assignment is DECIDED: every point belongs to one of a few GT objects, the model's mask
puts ~0.9 on the slot a fixed permutation gives that object, and the remaining GT columns are empty.  Empty columns are
identical, so which of them an unmatched slot receives is a tie without consequence: tests compare the permuted labels, the loss
and the gradient, never the permutation."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import detgen  # noqa: E402


def make_inputs(B, n, k, seed, fractional=False, valid="none", n_object=None):
    """mask, gt_mask (B, n, k) float32, valid (B, n) float32 or None.  valid: "none", "partial" (every fourth point out, and a few
    fractional weights) or "zero0" (sample 0 entirely invalid, the others partial)."""
    n_object = max(1, min(k, 5) if n_object is None else n_object)
    segm = (detgen.uniform((B, n), seed, 0.0, 1.0) * n_object).astype(np.int64).clip(0, n_object - 1)
    order = np.argsort(detgen.uniform((B, k), seed + 1), axis=1)              # GT column j is predicted in slot order[b, j]
    gt = np.eye(k, dtype=np.float32)[segm]
    if fractional:
        gt = gt * detgen.uniform((B, 1, k), seed + 2, 0.6, 1.0)
    logits = 5.0 * np.eye(k, dtype=np.float64)[np.take_along_axis(order, segm, 1)] + detgen.uniform((B, n, k), seed + 3)
    e = np.exp(logits - logits.max(-1, keepdims=True))
    mask = (e / e.sum(-1, keepdims=True)).astype(np.float32)
    v = None
    if valid != "none":
        v = np.ones((B, n), np.float32)
        v[:, 3::4] = 0.0
        v[:, 1::7] = 0.5
        if valid == "zero0":
            v[0] = 0.0
    return torch.from_numpy(mask), torch.from_numpy(gt.astype(np.float32)), None if v is None else torch.from_numpy(v)


def S():
    from ogc_amd.losses import seg_loss_sup
    return seg_loss_sup


def make_losses(focal):
    """focal: None or (alpha, gamma) -> (ce_loss, dice_loss) of ogc_amd.losses.seg_loss_sup."""
    from ogc_amd.losses import seg_loss_sup as S
    return (S.CrossEntropyLoss() if focal is None else S.FocalLoss(*focal)), S.DiceLoss()


def tensor_path(mask, gt, valid, focal, weights, dtype, cols=None):
    """Everything the kernels compute, by the package's tensor path on CPU tensors of `dtype`: cost_ce, cost_dice (B, k, k), cols
    (B, k) (given, or the minimiser of the reference's cost), perm_gt, sums (B, k, 4), terms (2,), loss, grad (B, n, k)."""
    from ogc_amd.losses import seg_loss_sup as S
    ce_loss, dice_loss = make_losses(focal)
    w_ce, w_dice = weights
    m = mask.detach().to(dtype).clone().requires_grad_(True)
    g = gt.to(dtype)
    v = None if valid is None else valid.to(dtype)
    cost_ce, cost_dice = S.match_cost_tables(ce_loss, dice_loss, m, g, v)
    if cols is None:
        cols = S._columns_by_cost(w_ce * cost_ce + w_dice * cost_dice.mean())
    perm_gt = S.permute_labels(g, cols)
    vv = torch.ones_like(m[..., 0]) if v is None else v
    with torch.no_grad():
        sums = torch.stack([(ce_loss.elementwise(m, perm_gt) * vv[..., None]).sum(1), ((m * perm_gt) * vv[..., None]).sum(1),
                            (m * vv[..., None]).sum(1), (perm_gt * vv[..., None]).sum(1)], -1)
    l_ce, l_dice = ce_loss(m, perm_gt, v), dice_loss(m, perm_gt, v)
    loss = w_ce * l_ce + w_dice * l_dice
    grad, = torch.autograd.grad(loss, m)
    return dict(cost_ce=cost_ce.detach(), cost_dice=cost_dice.detach(), cols=cols, perm_gt=perm_gt, sums=sums,
                terms=torch.stack([l_ce, l_dice]).detach(), loss=loss.detach(), grad=grad)


def within(got, truth, yard, scale=None):
    """The issue's bound: |got - truth| <= 2 * max|yard - truth| + 4 float32 ulps of the value (of `scale` when given: the
    largest entry, for gradients).  Returns (ok, ratio) with ratio = max|got - truth| / max|yard - truth| (inf when the
    float32 path is exact)."""
    got, truth, yard = (np.asarray(x, np.float64) for x in (got, truth, yard))
    ref = np.abs(truth) if scale is None else np.full(truth.shape, float(scale))
    floor = 4.0 * np.spacing(ref.astype(np.float32)).astype(np.float64)
    d_yard = float(np.max(np.abs(yard - truth))) if truth.size else 0.0
    err = np.abs(got - truth)
    ok = bool(np.all(err <= 2.0 * d_yard + floor))
    d_got = float(err.max()) if truth.size else 0.0
    return ok, (d_got / d_yard if d_yard > 0 else (0.0 if d_got == 0 else float("inf")))


# ---- the supervised trainer's replay (tests/golden/make_sup_golden.py records the reference's run, test_train_sup_driver.py
# replays it): segnet_kitti on six 512-point scenes, 2 epochs, the schedules moving every two iterations.  A small learning rate,
# as for the other replays (golden/driver_cases.py): Adam turns the rounding noise of analytically zero gradients into steps of
# size lr.
N_SUP, K_SUP, OBJECTS_SUP = 512, 8, 5
SUP_CFG = {
    "dataset": "kittisf", "random_seed": 10, "ignore_npoint_thresh": 60,
    "epochs": 2, "batch_size": 2, "lr": 1.0e-5, "lr_decay": 0.5, "lr_clip": 2.0e-6, "bn_momentum": 0.9, "bn_decay": 0.5,
    "weight_decay": 1.0e-4, "decay_step": 4,
    "segnet": {"n_slot": K_SUP, "n_point": N_SUP, "use_xyz": True, "n_transformer_layer": 1, "transformer_embed_dim": 32,
               "transformer_input_pos_enc": False},
    "loss": {"use_focal": True, "focal_loss_params": {"alpha": 0.25, "gamma": 2}, "weights": [2.0, 0.1]},
}


class SupScenes(torch.utils.data.Dataset):
    """Six (train) or two (val) scenes of golden/driver_cases.SegScenes with the sample contract of a reader built with
    onehot_label=True: segms (2, N, K_SUP) f32 one-hot, valids 0 at the points of objects under the threshold.  `poisoned` is
    True while the batch that holds the SECOND draw of scene 5 (the last iteration of epoch 2) is the latest one drawn: the
    replay's gradient hook (nan_gradient_hook) turns that step's gradients into NaN, and both trainers must leave the weights
    and the optimiser state alone (train_seg_sup.py:74-76)."""

    def __init__(self, train=True, seed=0, ulp=0, dtype=np.float32):
        import driver_cases as dc
        self.inner = dc.SegScenes(train, N_SUP, OBJECTS_SUP, seed=seed, ulp=ulp)
        self.inner.poison = False
        self.train, self.dtype, self.poisoned = train, dtype, False

    def __len__(self):
        return len(self.inner)

    def __getitem__(self, i):
        from ogc_amd.utils.data_util import batch_segm_to_mask
        pcs, segms, flows, _ = self.inner[i]
        masks, valids = batch_segm_to_mask(segms.astype(np.int64), K_SUP, SUP_CFG["ignore_npoint_thresh"])
        if self.train and i >= 4:
            self.poisoned = self.inner.calls[5] == 2
        return pcs.astype(self.dtype), masks.astype(self.dtype), flows.astype(self.dtype), valids.astype(self.dtype)


def nan_gradient_hook(net, train_set):
    """While train_set.poisoned, the gradient of the net's first parameter comes out as NaN."""
    first = next(net.parameters())
    first.register_hook(lambda g: g * float("nan") if train_set.poisoned else g)


# ---- the readers with onehot_label=True (tests/golden/sup_readers.npz)
READER_CASES = (   # (tag, data set, reference module, class, extra keyword arguments)
    ("kittisf_t0", "kittisf", "datasets.dataset_kittisf", "KITTISceneFlowDataset", dict(max_n_object=9)),
    ("kittisf_t15", "kittisf", "datasets.dataset_kittisf", "KITTISceneFlowDataset", dict(max_n_object=9, ignore_npoint_thresh=15, decentralize=True)),
    ("kittidet_t15", "kittidet", "datasets.dataset_kittidet", "KITTIDetectionDataset", dict(max_n_object=9, ignore_npoint_thresh=15)),
    ("ogcdr", "ogcdr", "datasets.dataset_ogcdr", "OGCDynamicRoomDataset", dict(max_n_object=6)),
)
N_READER = 96


def _reader_labels(seed, n_frame):
    """(n_frame, N_READER) int32 object ids with gaps (0, 3, 4, 7, 9, 12) and sizes that fall with the id, so that a threshold
    of 15 points drops some objects; integer hashing only."""
    ids = np.array([0, 3, 4, 7, 9, 12], np.int32)
    return ids[(detgen.uniform((n_frame, N_READER), seed, 0.0, 1.0) ** 2 * 6).astype(np.int64).clip(0, 5)]


def write_reader_roots(root, dataset):
    """Three training and two validation scenes under <root>/train and <root>/val in the layout `dataset`'s reader takes
    (kittisf, kittidet, ogcdr), from integer-hash data (detgen): the same bytes on every machine.  OGC-DR poses are a quarter
    turn about y and a shift, exact in binary.  Returns {split: (data root, split file or None)}."""
    out = {}
    for split, n_scene, base in (("train", 3, 8100), ("val", 2, 8200)):
        sub, names = os.path.join(root, split), []
        for i in range(n_scene):
            seed, name = base + 10 * i, "%06d" % i
            names.append(name)
            if dataset == "kittisf":
                d = os.path.join(sub, "data", name)
                os.makedirs(d, exist_ok=True)
                segm = _reader_labels(seed, 2)
                for v in (0, 1):
                    np.save(os.path.join(d, "pc%d.npy" % (v + 1)), detgen.cloud(1, N_READER, seed + 1 + v)[0])
                    np.save(os.path.join(d, "segm%d.npy" % (v + 1)), segm[v])
                    np.save(os.path.join(d, "flow%d.npy" % (v + 1)), detgen.uniform((N_READER, 3), seed + 3 + v, -0.5, 0.5))
            elif dataset == "kittidet":
                d = os.path.join(sub, "downsampled", name)
                os.makedirs(d, exist_ok=True)
                np.save(os.path.join(d, "pc.npy"), detgen.cloud(1, N_READER, seed + 1)[0])
                np.save(os.path.join(d, "segm.npy"), _reader_labels(seed, 1)[0])
            else:
                d = os.path.join(sub, "data", name)
                os.makedirs(d, exist_ok=True)
                segm = (_reader_labels(seed, 4) % 4).astype(np.int32)        # 0 background, objects 1..3
                turn = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])
                for t in range(4):
                    pose = np.tile(np.eye(4), (3, 1, 1))
                    for k in range(3):
                        pose[k, :3, :3] = np.linalg.matrix_power(turn, (t + k) % 4)
                        pose[k, :3, 3] = 0.125 * np.array([t, k, t + k], np.float64)
                    np.save(os.path.join(d, "pc_%02d.npy" % t), detgen.uniform((N_READER, 3), seed + 1 + t, -0.5, 0.5))
                    np.save(os.path.join(d, "segm_%02d.npy" % t), segm[t])
                    np.save(os.path.join(d, "pose_%02d.npy" % t), pose)
        mapping = None
        if dataset == "ogcdr":
            with open(os.path.join(sub, "data", split + ".lst"), "w") as f:
                f.write("\n".join(names) + "\n")
        else:
            mapping = os.path.join(sub, split + ".txt")
            with open(mapping, "w") as f:
                f.write("\n".join(names) + "\n")
        out[split] = (sub, mapping)
    return out


def reader_kwargs(dataset, root, mapping, split, extra):
    """Constructor arguments shared by the reference's classes and this package's ."""
    kw = dict(data_root=root, onehot_label=True, **extra)
    if dataset == "kittisf":
        kw.update(mapping_path=mapping, downsampled=True, view_sels=[[0, 1], [1, 0]])
    elif dataset == "kittidet":
        kw.update(mapping_path=mapping)
    else:
        kw.update(split=split, view_sels=[[0, 1], [1, 2], [2, 3], [3, 2]])
    return kw

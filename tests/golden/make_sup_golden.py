"""Generates the fixtures of the supervised segmentation path by running the reference's own code (imported from
/root/reference, which exists only in the build container) on the CPU:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_sup_golden.py

  sup_loss.npz   losses/seg_loss_sup.py: SupervisedMaskLoss in float32 — loss, loss_dict, the gradient of the masks and the
                 PERMUTED LABELS — for BCE and focal, with and without `valid`, weights [2.0, 0.1] and [2.0, 0], on one input
                 (tests/sup_cases.py: make_inputs, stored).  The float64 truth of each case: the reference's einsum mixes its
                 float32 `perm` with double labels and raises, so the permutation is taken from the float32 run and the
                 reference's ce_loss / dice_loss forward are evaluated on double tensors with the labels permuted by it.
                 The assignment is DECIDED: for every sample and case the float64 cost of the best assignment beats that of
                 every assignment yielding different permuted labels by MARGIN (asserted here, stored in the metadata).
                 utils/data_util.py: batch_segm_to_mask and batch_segm_to_mask_withconf on label arrays with small objects,
                 with and without a threshold, including the labels as the in-place relabelling leaves them.
  train_seg_sup_trace.npz   train_seg_sup.Trainer.train (train_seg_sup.py:19-202) over 2 epochs of the six-scene, 512-point
                 in-memory set of tests/sup_cases.py (SupScenes) with segnet_kitti, detgen weights, its LambdaLR(lr_curve) and
                 BNMomentumScheduler(bn_curve): per iteration the loss_dict, the learning rate, the norm momentum and a summary
                 of the weights after the step (one NaN-gradient step included); per epoch the validation loss, its loss_dict,
                 PQ / F1 / Pre / Rec and the best-checkpoint decision.  As gen_train_seg_waymo of make_driver_golden.py, the
                 data seed is the first whose run does not move (< 1e-4 on every loss term) under one-ulp changes of the
                 coordinates.  `python tests/golden/make_sup_golden.py trace64` writes the float64 twin (train_seg_sup_trace_f64.npz)
                 for the stored seed, in a process of its own; there the reference's float32 permutation matrix is cast to the
                 labels' dtype (its einsum raises on mixed dtypes).
  sup_readers.npz   samples of the reference's KITTISceneFlowDataset, KITTIDetectionDataset and OGCDynamicRoomDataset built
                 with onehot_label=True on small roots of integer-hash data (tests/sup_cases.py: write_reader_roots; the test
                 writes the same roots again): every array of the first and the last sample of both splits, with and without a
                 threshold, augmentation off.
                 (SapienDataset is not pinned against the reference's class: it imports pyquaternion, which this image lacks.)
Only data is written."""
import itertools
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import detgen  # noqa: E402
import sup_cases as sc  # noqa: E402
from make_golden import install_shims, save  # noqa: E402

MARGIN = 1e-2   # float32 rounding moves a cost of this size (<= a few units) by ~1e-6
B, N, K = 3, 150, 7
FOCAL = (0.25, 2)


def label_margin(cost, gt):
    """Per sample: (cost of the best assignment whose permuted labels differ from the optimum's) - (optimal cost)."""
    perms = np.array(list(itertools.permutations(range(cost.shape[-1]))))
    rows = np.arange(cost.shape[-1])
    out = []
    for b in range(cost.shape[0]):
        # columns that are equal as label vectors (the empty ones) get one name
        _, name = np.unique(gt[b].T, axis=0, return_inverse=True)
        totals = cost[b][rows, perms].sum(1)
        best = int(totals.argmin())
        other = (name.reshape(-1)[perms] != name.reshape(-1)[perms[best]]).any(1)
        out.append(float(totals[other].min() - totals[best]))
    return out


def gen_loss(arrays, meta):
    from losses.seg_loss_sup import CrossEntropyLoss, DiceLoss, FocalLoss, SupervisedMaskLoss
    mask, gt, valid = sc.make_inputs(B, N, K, 41, fractional=True, valid="partial", n_object=5)
    arrays.update(mask=mask.numpy(), gt_mask=gt.numpy(), valid=valid.numpy())
    meta["cases"], meta["margin"] = [], MARGIN
    for focal in (None, FOCAL):
        for use_valid in (False, True):
            for weights in ([2.0, 0.1], [2.0, 0]):
                tag = "%s_%s_w%d" % ("focal" if focal else "bce", "valid" if use_valid else "all", weights[1] > 0)
                ce_loss = FocalLoss(*focal) if focal else CrossEntropyLoss()
                crit = SupervisedMaskLoss(ce_loss, DiceLoss(), weights)
                v = valid if use_valid else None
                m = mask.clone().requires_grad_(True)
                # the permuted labels: the reference keeps them in a local; record them through its ce_loss
                seen = {}
                inner = ce_loss.forward
                ce_loss.forward = lambda pred, target, valid=None, _f=inner: (seen.__setitem__("perm_gt", target.clone()),
                                                                              _f(pred, target, valid))[1]
                loss, loss_dict = crit(m, gt.clone(), v)
                ce_loss.forward = inner
                loss.backward()
                perm_gt = seen["perm_gt"]
                # float64 truth with the float32 run's permuted labels
                m64 = mask.double().requires_grad_(True)
                v64 = None if v is None else v.double()
                l_ce, l_dice = ce_loss(m64, perm_gt.double(), v64), DiceLoss()(m64, perm_gt.double(), v64)
                loss64 = weights[0] * l_ce + weights[1] * l_dice
                loss64.backward()
                # decidedness, on the float64 cost the reference's formula gives
                rep_m = mask.double().unsqueeze(3).repeat(1, 1, 1, K)
                rep_g = gt.double().unsqueeze(2).repeat(1, 1, K, 1)
                cost = weights[0] * ce_loss.match_cost(rep_m, rep_g, v64) + weights[1] * DiceLoss().match_cost(rep_m, rep_g, v64)
                margins = label_margin(cost.numpy(), gt.numpy())
                assert min(margins) > MARGIN, (tag, margins)
                names = ("cross_entropy", "dice", "sum")
                arrays.update({tag + "/loss": np.float64(loss.item()), tag + "/loss_dict": np.array([loss_dict[k] for k in names]),
                               tag + "/grad": m.grad.numpy(), tag + "/perm_gt": perm_gt.numpy(),
                               tag + "/loss64": np.float64(loss64.item()),
                               tag + "/loss_dict64": np.array([l_ce.item(), l_dice.item(), loss64.item()]),
                               tag + "/grad64": m64.grad.numpy()})
                meta["cases"].append(dict(tag=tag, focal=focal, valid=use_valid, weights=weights, margins=margins))
                print("%-18s loss %.7f (float64 %.7f)  smallest margin %.3f" % (tag, loss.item(), loss64.item(), min(margins)))


def label_arrays():
    """(B, N) labels with a few small objects and non-consecutive ids, and per-sample confidences indexed by object id."""
    segm = (detgen.uniform((3, 120), 51, 0.0, 1.0) ** 2 * 6).astype(np.int64)     # sizes fall with the id
    segm[1] = segm[1] * 2 + 1                                                      # odd ids 1, 3, ..., 11
    segm[2, :5] = 9                                                                # a five-point object
    confs = [detgen.uniform((int(s.max()) + 1,), 52 + i, 0.3, 1.0) for i, s in enumerate(segm)]
    return segm, confs


def gen_masks(arrays, meta):
    from utils.data_util import batch_segm_to_mask, batch_segm_to_mask_withconf
    segm, confs = label_arrays()
    arrays["segm"] = segm
    for i, c in enumerate(confs):
        arrays["conf%d" % i] = c
    meta["mask_cases"] = []
    for thresh in (0, 8, 20):
        for withconf in (False, True):
            tag = "masks_t%d%s" % (thresh, "_conf" if withconf else "")
            work = segm.copy()
            if withconf:
                masks, valids = batch_segm_to_mask_withconf(work, confs, 12, thresh)
            else:
                masks, valids = batch_segm_to_mask(work, 12, thresh)
            arrays.update({tag + "/masks": masks, tag + "/valids": valids, tag + "/segm_after": work})
            meta["mask_cases"].append(dict(tag=tag, thresh=thresh, withconf=withconf, max_n_object=12))
            print("%-18s masks %s %s, %d points relabelled" % (tag, masks.shape, masks.dtype, int((work != segm).sum())))


def gen_readers():
    import importlib.util
    import tempfile

    arrays = {}
    for tag, dataset, module, cls_name, extra in sc.READER_CASES:
        spec = importlib.util.spec_from_file_location("ref_" + module.replace(".", "_"),
                                                      os.path.join("/root/reference", *module.split(".")) + ".py")
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        with tempfile.TemporaryDirectory() as tmp:
            roots = sc.write_reader_roots(tmp, dataset)
            for split in ("train", "val"):
                ds = getattr(mod, cls_name)(**sc.reader_kwargs(dataset, *roots[split], split, extra))
                arrays["%s/%s/len" % (tag, split)] = np.array([len(ds)])
                for sid in (0, len(ds) - 1):
                    for name, value in zip(("pcs", "segms", "flows", "valids"), ds[sid]):
                        arrays["%s/%s/%d/%s" % (tag, split, sid, name)] = value
        print("%-14s %d samples recorded, segms %s" % (tag, 4, arrays["%s/train/0/segms" % tag].shape))
    save("sup_readers", **arrays)


def trace(f64, seed, ulp, write):
    import shutil
    import tempfile
    import types

    import train_seg_sup as ref
    from losses import seg_loss_sup as ref_loss
    from metrics.seg_metric import calculate_PQ_F1
    from models.segnet_kitti import MaskFormer3D
    from utils.pytorch_util import BNMomentumScheduler
    from make_driver_golden import weight_summary
    cfg = sc.SUP_CFG
    ref.args = types.SimpleNamespace(**cfg)
    if f64 and not getattr(ref_loss, "_cast", False):
        inner_match = ref_loss.match_mask_by_cost
        ref_loss.match_mask_by_cost = lambda cost: inner_match(cost).to(cost.dtype)
        ref_loss._cast = True
    net = detgen.fill_module(MaskFormer3D(**cfg["segnet"]), 35)
    if f64:
        net = net.double()
    optimizer = torch.optim.Adam(net.parameters(), lr=cfg["lr"], weight_decay=cfg["weight_decay"])
    lr_scheduler = torch.optim.lr_scheduler.LambdaLR(optimizer, lr_lambda=ref.lr_curve)
    bnm_scheduler = BNMomentumScheduler(net, bn_lambda=ref.bn_curve)
    L = cfg["loss"]
    ce_loss = ref_loss.FocalLoss(**L["focal_loss_params"]) if L["use_focal"] else ref_loss.CrossEntropyLoss()
    criterion = ref_loss.SupervisedMaskLoss(ce_loss, ref_loss.DiceLoss(), weights=L["weights"])
    tmp = tempfile.mkdtemp()
    trainer = ref.Trainer(segnet=net, criterion=criterion, optimizer=optimizer, ignore_npoint_thresh=cfg["ignore_npoint_thresh"],
                          exp_base=os.path.join(tmp, "sup"), lr_scheduler=lr_scheduler, bnm_scheduler=bnm_scheduler)
    dtype = np.float64 if f64 else np.float32
    train_set, val_set = sc.SupScenes(True, seed, ulp, dtype), sc.SupScenes(False, seed, ulp, dtype)
    sc.nan_gradient_hook(net, train_set)
    train_loader = torch.utils.data.DataLoader(train_set, batch_size=cfg["batch_size"], shuffle=False)
    val_loader = torch.utils.data.DataLoader(val_set, batch_size=cfg["batch_size"], shuffle=False)
    its, epochs = [], []
    inner, inner_eval = trainer._train_it, trainer.eval_epoch

    def recording_train_it(it, batch, aug_transform=False):
        out = inner(it, batch, aug_transform=aug_transform)
        norms, heads = weight_summary(net)
        mom = next(m.momentum for m in net.modules() if isinstance(m, torch.nn.GroupNorm))
        its.append(dict(loss=dict(out[0]), lr=optimizer.param_groups[0]["lr"], momentum=mom, norms=norms, heads=heads))
        return out

    def recording_eval(loader):
        val_loss, val_avg, ap = inner_eval(loader)
        pq = calculate_PQ_F1(np.concatenate(ap["Pred_IoU"]), np.concatenate(ap["Pred_Matched"]), np.sum(ap["N_GT_Inst"]))
        epochs.append(dict(val_loss=val_loss, val_avg=dict(val_avg), pq=pq))
        return val_loss, val_avg, ap

    trainer._train_it, trainer.eval_epoch = recording_train_it, recording_eval
    best = trainer.train(cfg["epochs"], train_loader, val_loader)
    names = sorted(its[0]["loss"])
    val_loss = np.array([e["val_loss"] for e in epochs])
    out = dict(loss_names=np.array(names), loss=np.array([[r["loss"][k] for k in names] for r in its], np.float64),
               lr=np.array([r["lr"] for r in its]), momentum=np.array([r["momentum"] for r in its]),
               norms=np.stack([r["norms"] for r in its]), heads=np.stack([r["heads"] for r in its]), val_loss=val_loss,
               val_names=np.array(sorted(epochs[0]["val_avg"])),
               val_avg=np.array([[e["val_avg"][k] for k in sorted(e["val_avg"])] for e in epochs]),
               val_pq=np.array([e["pq"] for e in epochs], np.float64), best=np.array([best]),
               is_best=np.array([v < np.min(np.append(val_loss[:i], 1e10)) for i, v in enumerate(val_loss)]),
               data_seed=np.array([seed]))
    ck = torch.load(os.path.join(tmp, "sup", "best.pth.tar"))
    out["ckpt_keys"], out["ckpt_top"] = np.array(sorted(ck["model_state"].keys())), np.array(sorted(ck.keys()))
    assert sorted(os.listdir(os.path.join(tmp, "sup"))) == ["best.pth.tar", "current.pth.tar", "log"]
    shutil.rmtree(tmp)
    if write:
        save("train_seg_sup_trace" + ("_f64" if f64 else ""), **out)
    return out


def gen_trace(f64):
    if f64:
        return trace(True, int(np.load(os.path.join(HERE, "train_seg_sup_trace.npz"))["data_seed"][0]), 0, True)
    for seed in range(5000, 5400, 20):
        base = trace(False, seed, 0, False)
        assert np.isfinite(base["loss"]).all() and len(base["lr"]) == 6
        dev = 0.0
        for ulp in (1, 2):
            other = trace(False, seed, ulp, False)
            for key in ("loss", "val_avg"):
                dev = max(dev, float(np.max(np.abs(other[key] - base[key]) / np.abs(base[key]).clip(1e-3))))
        print("seed %d: largest change of a loss under one-ulp perturbations %.2e" % (seed, dev), flush=True)
        if dev < 1e-4:
            return trace(False, seed, 0, True)
    raise RuntimeError("no stable seed")


if __name__ == "__main__":
    which = sys.argv[1:] or ["loss", "readers", "trace"]
    writer = type("_Writer", (), {"__init__": lambda self, *a, **k: None, "add_scalar": lambda self, *a, **k: None,
                                  "flush": lambda self: None})
    if "trace64" in which:
        # as make_driver_golden.py: make_truth_f64.py's shims (indices decided in fp32, floats in fp64), a process of its own
        from make_truth_f64 import install_shims_f64
        install_shims_f64()
        torch.set_default_dtype(torch.float64)
        sys.modules["tensorboardX"].SummaryWriter = writer
        gen_trace(True)
        sys.exit(0)
    install_shims()
    sys.modules["tensorboardX"].SummaryWriter = writer
    if "loss" in which:
        arrays, meta = {}, {}
        gen_loss(arrays, meta)
        gen_masks(arrays, meta)
        save("sup_loss", meta=json.dumps(meta), **arrays)
    if "readers" in which:
        gen_readers()
    if "trace" in which:
        gen_trace(False)

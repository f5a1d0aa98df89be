"""The supervised path on the CPU against tests/golden/sup_loss.npz, recorded from the reference's own code
(tests/golden/make_sup_golden.py): the tensor path of ogc_amd/losses/seg_loss_sup.py against the reference's
SupervisedMaskLoss, and utils/data_util.py's batch_segm_to_mask / batch_segm_to_mask_withconf against the reference's.

Bounds.  The permuted labels are EQUAL (the fixture's inputs have a decided assignment: its generator asserts the margin).  The
tensor path evaluates the reference's element-wise float32 expressions and differs from it only in the order of float32 sums
over at most B * N * K = 3150 terms: a loss term is within 1e-6 relative of the reference's float32 value (pairwise float32
summation of n non-negative terms is good to about log2(n) * 2^-24 = 7e-7), the gradient — element-wise, no sum but the Dice
coefficients — within 1e-6 of its largest entry.  In float64 the same code is within 1e-12 of the recorded float64 truth."""
import json
import os

import numpy as np
import pytest
import torch

import sup_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("cross_entropy", "dice", "sum")


@pytest.fixture(scope="module")
def golden():
    data = np.load(os.path.join(HERE, "golden", "sup_loss.npz"))
    return data, json.loads(str(data["meta"]))


def _criterion(case):
    from ogc_amd.losses.seg_loss_sup import SupervisedMaskLoss
    return SupervisedMaskLoss(*sc.make_losses(case["focal"]), case["weights"])


def test_tensor_path_reproduces_the_reference_in_float32(golden):
    data, meta = golden
    assert len(meta["cases"]) == 8 and min(min(c["margins"]) for c in meta["cases"]) > meta["margin"]
    for case in meta["cases"]:
        tag, crit = case["tag"], _criterion(case)
        mask = torch.from_numpy(data["mask"]).requires_grad_(True)
        gt, valid = torch.from_numpy(data["gt_mask"]), (torch.from_numpy(data["valid"]) if case["valid"] else None)
        assert not crit.kernels_apply(mask, gt, valid)
        assert np.array_equal(crit.matched_labels(mask, gt, valid).numpy(), data[tag + "/perm_gt"]), tag
        loss, loss_dict = crit(mask, gt, valid)
        loss.backward()
        assert sorted(loss_dict) == sorted(NAMES) and all(isinstance(loss_dict[k], float) for k in NAMES)
        got = np.array([loss_dict[k] for k in NAMES])
        assert np.allclose(got, data[tag + "/loss_dict"], rtol=1e-6, atol=0), (tag, got, data[tag + "/loss_dict"])
        assert abs(loss.item() - float(data[tag + "/loss"])) <= 1e-6 * abs(float(data[tag + "/loss"]))
        ref = data[tag + "/grad"]
        assert np.abs(mask.grad.numpy() - ref).max() <= 1e-6 * np.abs(ref).max(), tag
        assert not gt.requires_grad


def test_tensor_path_reproduces_the_float64_truth(golden):
    data, meta = golden
    for case in meta["cases"]:
        tag, crit = case["tag"], _criterion(case)
        mask = torch.from_numpy(data["mask"]).double().requires_grad_(True)
        gt = torch.from_numpy(data["gt_mask"]).double()
        valid = torch.from_numpy(data["valid"]).double() if case["valid"] else None
        assert np.array_equal(crit.matched_labels(mask, gt, valid).numpy(), data[tag + "/perm_gt"].astype(np.float64)), tag
        loss, loss_dict = crit(mask, gt, valid)
        loss.backward()
        got = np.array([loss_dict[k] for k in NAMES])
        assert np.allclose(got, data[tag + "/loss_dict64"], rtol=1e-12, atol=0), (tag, got)
        ref = data[tag + "/grad64"]
        assert np.abs(mask.grad.numpy() - ref).max() <= 1e-12 * np.abs(ref).max(), tag


def test_pairwise_tables_are_the_reference_formula_on_the_repeats(golden):
    """match_cost_tables (one GT column at a time) against match_cost on the (B, N, K, K) repeats the reference builds; the
    Dice part of the matching cost is ONE scalar (the reference's mean without an axis)."""
    from ogc_amd.losses import seg_loss_sup as S
    data, _ = golden
    mask, gt, valid = (torch.from_numpy(data[k]).double() for k in ("mask", "gt_mask", "valid"))
    K = mask.shape[-1]
    rep_m, rep_g = mask.unsqueeze(3).repeat(1, 1, 1, K), gt.unsqueeze(2).repeat(1, 1, K, 1)
    for focal in (None, (0.25, 2), (-1, 3)):
        ce_loss, dice_loss = sc.make_losses(focal)
        for v in (None, valid):
            cost_ce, cost_dice = S.match_cost_tables(ce_loss, dice_loss, mask, gt, v)
            assert torch.allclose(cost_ce, ce_loss.match_cost(rep_m, rep_g, v), rtol=1e-13, atol=0)
            scalar = dice_loss.match_cost(rep_m, rep_g, v)
            assert scalar.shape == torch.Size([]) and torch.allclose(cost_dice.mean(), scalar, rtol=1e-13, atol=0)
            assert torch.allclose(cost_dice, dice_loss.per_object(rep_m, rep_g, v), rtol=1e-13, atol=0)


def test_match_mask_by_cost_is_scipys_minimiser_and_nan_costs_give_nan():
    from scipy.optimize import linear_sum_assignment
    from ogc_amd.losses import seg_loss_sup as S
    cost = torch.from_numpy(sc.detgen.uniform((4, 6, 6), 77))
    perm = S.match_mask_by_cost(cost)
    assert perm.shape == (4, 6, 6) and perm.dtype == torch.float32
    for b in range(4):
        cols = linear_sum_assignment(cost[b].numpy(), maximize=False)[1]
        assert np.array_equal(perm[b].numpy(), np.eye(6, dtype=np.float32)[cols])
    cost[2, 3, 1] = float("nan")
    perm = S.match_mask_by_cost(cost)
    assert torch.isnan(perm[2]).all() and not torch.isnan(perm[[0, 1, 3]]).any()


def test_sync_false_returns_a_pending_dictionary_on_the_cpu(golden):
    from ogc_amd.losses import seg_loss_sup as S
    data, meta = golden
    case = meta["cases"][0]
    crit = _criterion(case)
    loss, pending = crit(torch.from_numpy(data["mask"]), torch.from_numpy(data["gt_mask"]), None, sync=False)
    assert isinstance(pending, S.PendingLossDict)
    assert pending.resolve() == crit(torch.from_numpy(data["mask"]), torch.from_numpy(data["gt_mask"]), None)[1]


def test_batch_segm_to_mask_reproduces_the_reference(golden):
    from ogc_amd.utils.data_util import batch_segm_to_mask, batch_segm_to_mask_withconf
    data, meta = golden
    confs = [data["conf%d" % i] for i in range(3)]
    assert len(meta["mask_cases"]) == 6
    for case in meta["mask_cases"]:
        tag, work = case["tag"], data["segm"].copy()
        if case["withconf"]:
            masks, valids = batch_segm_to_mask_withconf(work, confs, case["max_n_object"], case["thresh"])
        else:
            masks, valids = batch_segm_to_mask(work, case["max_n_object"], case["thresh"])
        for got, key in ((masks, "masks"), (valids, "valids"), (work, "segm_after")):
            want = data[tag + "/" + key]
            assert got.dtype == want.dtype and np.array_equal(got, want), (tag, key)
    # more objects than columns: the reference's IndexError
    with pytest.raises(IndexError):
        batch_segm_to_mask(data["segm"].copy(), 3)


def test_readers_with_onehot_labels_reproduce_the_reference(tmp_path):
    """KITTISceneFlowDataset, KITTIDetectionDataset and OGCDynamicRoomDataset with onehot_label=True against samples of the
    reference's classes on the same roots (tests/golden/sup_readers.npz; integer-hash data, the same bytes everywhere): the
    one-hot labels and the valids bit for bit; clouds and flows, which pass through a mean and a matrix product on the host,
    within 1e-6."""
    from ogc_amd import datasets
    data = np.load(os.path.join(HERE, "golden", "sup_readers.npz"))
    for tag, dataset, _, cls_name, extra in sc.READER_CASES:
        roots = sc.write_reader_roots(str(tmp_path / tag), dataset)
        for split in ("train", "val"):
            ds = getattr(datasets, cls_name)(**sc.reader_kwargs(dataset, *roots[split], split, extra))
            assert len(ds) == int(data["%s/%s/len" % (tag, split)][0])
            for sid in (0, len(ds) - 1):
                for name, got in zip(("pcs", "segms", "flows", "valids"), ds[sid]):
                    want = data["%s/%s/%d/%s" % (tag, split, sid, name)]
                    assert got.dtype == want.dtype and got.shape == want.shape, (tag, split, sid, name)
                    if name in ("segms", "valids"):
                        assert np.array_equal(got, want), (tag, split, sid, name)
                    else:
                        assert np.allclose(got, want, rtol=1e-6, atol=1e-6), (tag, split, sid, name)
    assert any((data[k] == 0).any() for k in data.files if k.endswith("valids"))   # the threshold does drop objects somewhere


def test_onehot_label_off_leaves_the_samples_as_they_were(tmp_path):
    """onehot_label=False (the default): labels stay (t, N) int32 and valids ones; with it on, the arg-max of the masks over the
    valid points gives those labels back, for all four readers (the SAPIEN reader is not pinned against the reference's class)."""
    from ogc_amd import datasets
    from ogc_amd.utils.synthetic import write_supervised_roots
    for dataset, cls_name, extra in (("sapien", "SapienDataset", {}), ("ogcdr", "OGCDynamicRoomDataset", {}),
                                     ("kittisf", "KITTISceneFlowDataset", dict(ignore_npoint_thresh=15)),
                                     ("kittidet", "KITTIDetectionDataset", dict(ignore_npoint_thresh=15))):
        roots = write_supervised_roots(str(tmp_path / dataset), dataset, n_train=3, n_val=2, n_points=96, n_objects=4)
        kw = sc.reader_kwargs(dataset, *roots["train"], "train", dict(max_n_object=9, **extra))
        hot = getattr(datasets, cls_name)(**kw)
        kw.pop("onehot_label"), kw.pop("max_n_object"), kw.pop("ignore_npoint_thresh", None)
        plain = getattr(datasets, cls_name)(**kw)
        for sid in range(len(plain)):
            (pcs, segms, flows, valids), (hpcs, hsegms, hflows, hvalids) = plain[sid], hot[sid]
            assert segms.dtype == np.int32 and segms.ndim == 2 and (valids == 1).all()
            assert hsegms.dtype == np.float32 and hsegms.shape == segms.shape + (9,) and hvalids.dtype == np.float32
            assert np.array_equal(pcs, hpcs) and np.array_equal(flows, hflows)
            keep = hvalids > 0
            assert np.array_equal(hsegms.sum(2), hvalids) and (dataset in ("sapien", "ogcdr")) <= bool(keep.all())
            for t in range(2):   # ranks are kept among the valid points: dropped objects only vacate label 0's neighbours
                ranks = np.unique(np.where(keep[t], segms[t], 0), return_inverse=True)[1]
                assert np.array_equal(hsegms[t].argmax(1)[keep[t]], ranks[keep[t]])

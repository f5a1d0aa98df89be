"""Self-training end to end on the device: `export_pseudo_labels` writes the predicted segmentations of a model, as
`test_seg --save` does, and the confidence of every object, KITTIDetectionDataset(load_prediction=, load_confidence=True) reads
them back as confidence-scaled targets, and `train_seg_sup` on config/kittidet_selftrain_synthetic.yaml trains on them.

One root for all tests (module scope): a kittidet training set of 4 frames and a validation set of 2, 512 points and 4 objects
each (write_supervised_roots; the validation frames are then moved into the training root under ids of their own, because the
trainer takes one data.root for both splits), and a randomly initialised segnet_kitti of the config's size saved where test_seg.weight_path
looks for round 0.  ogc_slot_confidence itself is checked against float64 truth in tests/test_seg_conf_gpu.py."""
import os
import shutil

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_TRAIN, N_VAL, N_POINT, N_OBJECT = 4, 2, 512, 4
COMMON = ["--num_workers", "0"]


def _dump(cfg, path):
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    return path


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """-> dict(cfg of the trainer, its path, export_path = the config of the model whose predictions are saved, roots, ids,
    a = the metrics of `test_seg --save`, segm_a = the bytes it wrote, b = the metrics of export_pseudo_labels, save_dir)."""
    from ogc_amd import export_pseudo_labels, test_seg
    from ogc_amd.utils.synthetic import write_supervised_roots
    tmp = str(tmp_path_factory.mktemp("selftrain"))
    with open(os.path.join(ROOT, "config", "kittidet_selftrain_synthetic.yaml")) as f:
        cfg = yaml.safe_load(f)
    assert cfg["segnet"]["n_point"] == N_POINT and cfg["data"]["load_prediction"] == "OGC_R0" and cfg["data"]["load_confidence"] is True
    roots = write_supervised_roots(os.path.join(tmp, "data"), "kittidet", N_TRAIN, N_VAL, N_POINT, N_OBJECT)
    # both splits under the one root the trainer takes: the writers number their scenes from 0, so the validation ids get a prefix
    with open(roots["val"][1]) as f:
        val_ids = f.read().split()
    assert len(val_ids) == N_VAL
    for i in val_ids:
        shutil.move(os.path.join(roots["val"][0], "downsampled", i), os.path.join(roots["train"][0], "downsampled", "val_" + i))
    val_mapping = os.path.join(roots["train"][0], "val.txt")
    with open(val_mapping, "w") as f:
        f.write("\n".join("val_" + i for i in val_ids) + "\n")
    cfg["data"].update(root=roots["train"][0], train_mapping=roots["train"][1], val_mapping=val_mapping)
    cfg["save_path"] = os.path.join(tmp, "ckpt", "selftrain")
    path = _dump(cfg, os.path.join(tmp, "selftrain.yaml"))
    export = dict(cfg, save_path=os.path.join(tmp, "ckpt", "r0"))          # the round-0 model: same network, its own directory
    export_path = _dump(export, os.path.join(tmp, "r0.yaml"))
    torch.manual_seed(77)
    net = test_seg.build_segnet(export)
    os.makedirs(export["save_path"])
    torch.save({"model_state": net.state_dict()}, test_seg.weight_path(export, 0))
    with open(roots["train"][1]) as f:
        ids = f.read().split()
    assert len(ids) == N_TRAIN

    argv = [export_path, "--split", "train", "--mapping", roots["train"][1], "--test_batch_size", str(N_TRAIN)] + COMMON
    a = test_seg.main(argv + ["--save"])
    save_dir = a["save_dir"]
    assert save_dir == os.path.join(roots["train"][0], "segm_preds", "OGC_R0")
    assert all(os.listdir(os.path.join(save_dir, i)) == ["segm.npy"] for i in ids)       # test_seg writes no conf.npy
    segm_a = [open(os.path.join(save_dir, i, "segm.npy"), "rb").read() for i in ids]
    b = export_pseudo_labels.main(argv)
    return dict(cfg=cfg, path=path, export=export, export_path=export_path, roots=roots, ids=ids, a=a, b=b, segm_a=segm_a,
                save_dir=save_dir, tmp=tmp)


def test_export_writes_a_confidence_per_saved_label_and_changes_nothing_else(world):
    from ogc_amd import datasets, test_seg
    from ogc_amd.metrics.seg_conf import pseudo_label_confidences
    w = world
    assert sorted(w["a"]) == sorted(w["b"])
    for key in w["a"]:                                                    # the metrics are test_seg's
        assert w["a"][key] == w["b"][key] or (w["a"][key] != w["a"][key] and w["b"][key] != w["b"][key]), key
    # the masks the same network gives for the same frames, in the driver's batch
    net = test_seg.build_segnet(w["export"]).cuda()
    net.load_state_dict(torch.load(test_seg.weight_path(w["export"], 0), map_location="cpu")["model_state"])
    net.eval()
    ds = datasets.KITTIDetectionDataset(data_root=w["roots"]["train"][0], mapping_path=w["roots"]["train"][1],
                                        decentralize=bool(w["export"]["data"]["decentralize"]))
    pc = torch.from_numpy(np.stack([ds[i][0][0] for i in range(N_TRAIN)], 0)).cuda()
    with torch.no_grad():
        mask = net(pc, pc).detach().float()
    want = pseudo_label_confidences(mask)
    hard = mask.argmax(dim=2).cpu().numpy()
    for i, idx in enumerate(w["ids"]):
        d = os.path.join(w["save_dir"], idx)
        assert sorted(os.listdir(d)) == ["conf.npy", "segm.npy"]
        assert open(os.path.join(d, "segm.npy"), "rb").read() == w["segm_a"][i]          # written exactly as before
        segm, conf = np.load(os.path.join(d, "segm.npy")), np.load(os.path.join(d, "conf.npy"))
        assert segm.dtype == np.int64 and segm.shape == (N_POINT,) and np.array_equal(segm, hard[i])
        assert conf.dtype == np.float32 and conf.shape == (len(np.unique(segm)),)
        assert np.isfinite(conf).all() and (conf > 0).all() and (conf <= 1).all()
        print(idx, "labels", np.unique(segm).tolist(), "conf", conf.tolist())
        assert conf.tobytes() == want[i].tobytes()


def test_export_is_refused_for_sets_without_one_label_file_per_id(capsys):
    from ogc_amd import export_pseudo_labels
    with pytest.raises(SystemExit):
        export_pseudo_labels.main([os.path.join(ROOT, "config", "kittisf_unsup_synthetic.yaml")] + COMMON)
    assert "kittidet, semantickitti" in capsys.readouterr().err


def test_export_refuses_labels_that_are_not_the_arg_max_of_the_kept_masks(monkeypatch, tmp_path):
    from ogc_amd import export_pseudo_labels, test_seg
    mask = torch.softmax(torch.randn(2, 33, 5, generator=torch.Generator().manual_seed(3)), dim=2).cuda()
    wrong = mask.argmax(dim=2).to(torch.int32)
    wrong[1, 7] = (wrong[1, 7] + 1) % 5

    def evaluate(segnet, loader, n_frame, ignore_npoint_thresh, saver=None, device="cuda"):
        segnet(None, None)
        saver(wrong, 0)

    monkeypatch.setattr(test_seg, "evaluate", evaluate)
    with pytest.raises(RuntimeError, match="not the arg-max"):
        export_pseudo_labels.export(lambda a, b: mask, None, None, 0, str(tmp_path), 2)
    assert os.listdir(str(tmp_path)) == []


def test_export_on_semantickitti(tmp_path):
    """The other set the driver covers: ids carry a sequence prefix, there is no split file."""
    from ogc_amd import export_pseudo_labels, test_seg
    from ogc_amd.utils.synthetic import write_labelled_root
    with open(os.path.join(ROOT, "config", "semantickitti_unsup_synthetic.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg["data"]["root"] = str(tmp_path / "root")
    cfg["save_path"] = str(tmp_path / "ckpt")
    cfg["segnet"]["n_point"] = N_POINT
    path = _dump(cfg, str(tmp_path / "semantickitti.yaml"))
    write_labelled_root(cfg["data"]["root"], "semantickitti", 3, N_POINT, N_OBJECT)
    os.makedirs(cfg["save_path"])
    torch.save({"model_state": test_seg.build_segnet(cfg).state_dict()}, test_seg.weight_path(cfg, 0))
    metrics = export_pseudo_labels.main([path, "--split", "val", "--test_batch_size", "1"] + COMMON)
    ids = sorted(os.listdir(metrics["save_dir"]))
    written = sorted(os.listdir(os.path.join(cfg["data"]["root"], "downsampled")))
    # the reader takes the sequences 0 .. 10; the synthetic root holds one frame of a later sequence as well
    assert len(ids) >= 2 and ids == [i for i in written if int(i[:2]) in test_seg.SEMANTICKITTI_SEQUENCES]
    for idx in ids:
        segm = np.load(os.path.join(metrics["save_dir"], idx, "segm.npy"))
        conf = np.load(os.path.join(metrics["save_dir"], idx, "conf.npy"))
        assert conf.dtype == np.float32 and conf.shape == (len(np.unique(segm)),) and (conf > 0).all() and (conf <= 1).all()


def test_reader_delivers_targets_scaled_by_the_saved_confidences(world):
    from ogc_amd import datasets
    w = world
    k = w["cfg"]["segnet"]["n_slot"]
    ds = datasets.KITTIDetectionDataset(data_root=w["roots"]["train"][0], mapping_path=w["roots"]["train"][1], decentralize=True,
                                        onehot_label=True, max_n_object=k, load_prediction="OGC_R0", load_confidence=True)
    for i, idx in enumerate(w["ids"]):
        conf = np.load(os.path.join(w["save_dir"], idx, "conf.npy"))
        segm = np.load(os.path.join(w["save_dir"], idx, "segm.npy"))
        _, segms, _, valids = ds[i]
        assert segms.shape == (2, N_POINT, k) and segms.dtype == np.float32 and (valids == 1).all()
        labels = np.unique(segm)
        for j in range(k):
            column = segms[0][:, j]
            if j < len(conf):
                assert np.array_equal(column != 0, segm == labels[j]) and (column[column != 0] == conf[j]).all()
            else:
                assert not column.any()


def _train(world, monkeypatch, load_confidence, name):
    from ogc_amd import train_seg_sup
    cfg = dict(world["cfg"], save_path=os.path.join(world["tmp"], "ckpt", name))
    cfg["data"] = dict(cfg["data"], load_confidence=load_confidence)
    path = _dump(cfg, os.path.join(world["tmp"], name + ".yaml"))
    losses = []
    base = getattr(train_seg_sup.Trainer, "recorded_base", train_seg_sup.Trainer)   # the driver's own class, also the second time

    class Recording(base):
        recorded_base = base

        def __init__(self, *args, **kw):
            kw["on_iteration"] = lambda it, loss_dict, stepped: losses.append((it, loss_dict["sum"], stepped))
            super().__init__(*args, **kw)

    monkeypatch.setattr(train_seg_sup, "Trainer", Recording)
    best = train_seg_sup.main([path, "--max-iters", "3"] + COMMON)
    return cfg, losses, best


def test_training_on_the_saved_predictions_and_the_confidences_reach_the_loss(world, monkeypatch):
    cfg, losses, best = _train(world, monkeypatch, True, "with_conf")
    print("losses with confidences", losses, "best validation loss", best)
    assert [it for it, _, _ in losses] == [0, 1, 2] and all(np.isfinite(v) for _, v, _ in losses) and all(s for _, _, s in losses)
    assert np.isfinite(best) and "current.pth.tar" in os.listdir(cfg["save_path"])
    _, ones, _ = _train(world, monkeypatch, False, "without_conf")
    print("losses with confidences of one", ones)
    assert len(ones) == 3 and np.isfinite(ones[0][1]) and ones[0][1] != losses[0][1]

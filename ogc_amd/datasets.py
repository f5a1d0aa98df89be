"""Readers / writers of the two on-disk layouts the drivers exchange data in — scenes as the reference's preparation scripts
leave them, predicted flows as its refinement script leaves them — with the interface of the reference's data sets (same class
names, constructor arguments and sample contract), so that `train_seg`, `oa_icp_round` and the reference's own tools can work on
one directory tree:

  KITTISceneFlowDataset      <root>/data/<id>/{pc,segm,flow}{1,2}.npy, a split file listing the ids
                             (datasets/dataset_kittisf.py:9-137); predicted flows <root>/flow_preds/<name>/<id>/flow{1,2}.npy
  OGCDynamicRoomDataset      <root>/data/<id>/{pc,segm,pose}_%02d.npy, <root>/data/<split>.lst
                             (datasets/dataset_ogcdr.py:30-157); predicted flows <root>/flow_preds/<name>/<id>.npy (P, N, 3) with
                             <root>/flow_preds/<name>.json {"view_sel": [...]} naming the P ordered frame pairs
  SapienDataset              <root>/data/%06d.npz {pc (V, N, 3), segm (V, N), trans: {"cam": (V, 4, 4), part id: (V, 4, 4)}},
                             <root>/meta.json {split: [ids]} (datasets/dataset_sapien.py:22-170); predicted flows in the
                             OGC-DR layout under %06d.npy.  NOT pinned against the reference's class: it imports pyquaternion
                             (utils/sapien_util.py), which this image lacks — tests/test_sapien_reader.py checks the flows against
                             the rigid motions applied directly
  WaymoOpenDataset           <root>/data/<sequence>/{pc,segm,semantic_segm}_%04d.npy and the backward flows flow_%04d_%04d.npy
                             (t, t - 1), a split file listing the sequences (datasets/dataset_waymo.py:19-181); predicted flows
                             <root>/flow_preds/<name>/<sequence>/flow_%04d_%04d.npy.  A sample id is (sequence, t, t - 1); with
                             downsampled=False the four items are lists of two frames with their own numbers of points

  WaymoSingleFrameDataset    the same files without the flows, one frame per sample: a sample id is (sequence, t)
                             (datasets/dataset_waymo_singleframe.py:54-206), and a sample is (pcs, segms, valids) — no flows.
                             For the supervised Waymo baseline and the Waymo evaluation (train_seg_waymo_sup.py,
                             test_seg_waymo.py); predicted segmentations <save_root>/<sequence>/segm_%04d.npy

  KITTIDetectionDataset      <root>/downsampled/<id>/{pc,segm}.npy, a split file listing the ids (datasets/dataset_kittidet.py)
  SemanticKITTIDataset       the same files; the ids are the sorted directory names whose first two characters are a sequence
                             number in `sequence_list` (datasets/dataset_semantickitti.py).  Both are single-frame sets for
                             evaluation (test_seg.py): the frame is duplicated to two views, the flows are zero.
                             KITTIDetectionDataset(load_prediction=NAME, load_confidence=True) takes its labels from
                             <root>/segm_preds/NAME/<id>/segm.npy and scales every object's one-hot column by conf.npy beside it

Predicted segmentations (`_save_predsegm`, written by test_seg.py under <root>/segm_preds/<name>): int64 labels per frame as
<id>/segm{1,2}.npy (KITTI-SF), <id>/segm_%02d.npy (OGC-DR; SAPIEN with <id> = %06d), <id>/segm.npy (KITTI-Det, SemanticKITTI;
with `conf=`, export_pseudo_labels.py, also <id>/conf.npy: one float32 confidence per distinct label, in ascending label order).

A sample is (pcs (t, N, 3) f32, segms (t, N) i32, flows (t, N, 3) f32, valids (t, N) f32), t = 2 frames, or 4 with
`aug_transform` (two random similarity transforms of the pair, utils/data_util.py:140-195).  With `onehot_label=True` — what the
supervised trainer (train_seg_sup.py) asks of KITTISceneFlowDataset, KITTIDetectionDataset, OGCDynamicRoomDataset and
SapienDataset — segms is instead (t, N, max_n_object) f32, one-hot over the ranks of the compressed labels, and valids is 0 at
the points of objects smaller than `ignore_npoint_thresh` (the two KITTI sets; utils/data_util.py: batch_segm_to_mask).
tests/golden/flow_store.npz and sup_readers.npz pin files and samples against the reference's classes.
"""
import os

import numpy as np
from torch.utils.data import Dataset

from .utils import flow_store
from .utils.data_util import augment_transform, batch_segm_to_mask, batch_segm_to_mask_withconf, compress_label_id


def _one_hot(segms, max_n_object, ignore_npoint_thresh):
    """The one-hot variant of a sample's labels (dataset_kittisf.py:106-109): (t, N, max_n_object) f32 masks and valids."""
    assert max_n_object > 0, 'max_n_object must be above 0!'
    return batch_segm_to_mask(segms, max_n_object, ignore_npoint_thresh)


def _finish(pcs, segms, flows, decentralize, aug_transform, aug_transform_args, valids=None, onehot=None):
    """Common tail of the readers: centring, label compression, augmentation, dtypes (dataset_kittisf.py:95-122).  `valids`:
    per-point validity of the two frames where the reader filters its labels (Waymo), all ones otherwise.  `onehot`:
    (max_n_object, ignore_npoint_thresh) of a reader built with onehot_label=True, else None."""
    pcs, segms, flows = np.stack(pcs, 0), np.stack(segms, 0), np.stack(flows, 0)
    if decentralize:
        pcs = pcs - pcs.mean(1).mean(0)
    segms = compress_label_id(np.reshape(segms, -1)).reshape(2, -1)
    if onehot is not None:
        segms, valids = _one_hot(segms, *onehot)
        if aug_transform:
            pcs, flows = augment_transform(pcs, flows, aug_transform_args)
            segms, valids = np.concatenate((segms, segms), 0), np.concatenate((valids, valids), 0)
        return pcs.astype(np.float32), segms.astype(np.float32), flows.astype(np.float32), valids.astype(np.float32)
    valids = np.ones_like(segms, dtype=np.float32) if valids is None else np.stack(valids, 0)
    if aug_transform:
        pcs, flows = augment_transform(pcs, flows, aug_transform_args)
        segms = np.concatenate((segms, segms), 0)
        valids = np.concatenate((valids, valids), 0)
    return pcs.astype(np.float32), segms.astype(np.int32), flows.astype(np.float32), valids.astype(np.float32)


def _hard_labels(mask_or_hard):
    """(B, N, K) soft masks -> their arg-max over K; (B, N) hard labels as they are; a tensor or an array -> numpy int64, what
    numpy's argmax gives the reference (`mask[sid].argmax(1)`, dataset_kittisf.py:144-146)."""
    x = mask_or_hard
    if hasattr(x, "detach"):
        x = x.detach()
        x = (x.argmax(dim=2) if x.dim() == 3 else x).cpu().numpy()
    else:
        x = np.asarray(x)
        x = x.argmax(2) if x.ndim == 3 else x
    if x.ndim != 2:
        raise ValueError("expected (B, N, K) masks or (B, N) labels, got shape %s" % (tuple(x.shape),))
    return x.astype(np.int64)


def _save_frame_labels(mask_or_hard, save_root, batch_size, n_frame, offset, scene_dir, file_name):
    """Sample `offset * batch_size + i` of a loader over (scene, frame) pairs -> <save_root>/<scene_dir(idx)>/<file_name(k)>."""
    hard = _hard_labels(mask_or_hard)
    for i in range(hard.shape[0]):
        idx, k = divmod(offset * batch_size + i, n_frame)
        d = os.path.join(save_root, scene_dir(idx))
        os.makedirs(d, exist_ok=True)
        np.save(os.path.join(d, file_name(k)), hard[i])


class KITTISceneFlowDataset(Dataset):
    def __init__(self, data_root, mapping_path, downsampled=False, view_sels=[[0, 1]], predflow_path=None, decentralize=False,
                 aug_transform=False, aug_transform_args=None, onehot_label=False, max_n_object=15, ignore_npoint_thresh=0):
        self.onehot_label, self.max_n_object, self.ignore_npoint_thresh = onehot_label, max_n_object, ignore_npoint_thresh
        self.data_root = os.path.join(data_root, "data" if downsampled else "processed")
        with open(mapping_path, "r") as f:
            self.data_ids = f.read().strip().split("\n")
        self.view_sels = [list(v) for v in view_sels]
        self.predflow_path = os.path.join(data_root, "flow_preds", predflow_path) if predflow_path is not None else None
        self.downsampled, self.decentralize = downsampled, decentralize
        self.aug_transform, self.aug_transform_args = aug_transform, aug_transform_args

    def __len__(self):
        return len(self.data_ids) * len(self.view_sels)

    def _load_data(self, idx, view_sel):
        d = os.path.join(self.data_root, self.data_ids[idx])
        a, b = view_sel
        pc1, pc2 = np.load(os.path.join(d, "pc%d.npy" % (a + 1))), np.load(os.path.join(d, "pc%d.npy" % (b + 1)))
        if self.downsampled:
            segms = [np.load(os.path.join(d, "segm%d.npy" % (v + 1))) for v in (a, b)]
            flows = [np.load(os.path.join(d, "flow%d.npy" % (v + 1))) for v in (a, b)]
        else:  # the full-resolution scans: one labelling, points in correspondence (dataset_kittisf.py:73-76)
            segm = np.load(os.path.join(d, "segm.npy"))
            segms, flows = [segm, segm], [pc2 - pc1, pc1 - pc2]
        return [pc1, pc2], segms, flows

    def _load_predflow(self, idx, view_sel):
        stored = flow_store.load_pair(self.predflow_path, self.data_ids[idx], view_sel)
        if stored is None:
            raise FileNotFoundError("no predicted flows for scene %s under %s" % (self.data_ids[idx], self.predflow_path))
        return stored

    def __getitem__(self, sid):
        idx, view_sel = sid // len(self.view_sels), self.view_sels[sid % len(self.view_sels)]
        pcs, segms, flows = self._load_data(idx, view_sel)
        if self.predflow_path is not None:
            flows = self._load_predflow(idx, view_sel)
        return _finish(pcs, segms, flows, self.decentralize, self.aug_transform, self.aug_transform_args,
                       onehot=(self.max_n_object, self.ignore_npoint_thresh) if self.onehot_label else None)

    def _save_predflow(self, flow_pred, save_root, batch_size, n_frame=1, offset=0):
        """flow_pred (B, N, 3): sample `offset * batch_size + i` of a loader over (scene, frame) pairs -> <save_root>/<id>/flow<k>.npy
        (dataset_kittisf.py:125-137)."""
        flow_pred = flow_pred.detach().cpu().numpy() if hasattr(flow_pred, "detach") else np.asarray(flow_pred)
        for i in range(flow_pred.shape[0]):
            idx, k = divmod(offset * batch_size + i, n_frame)
            d = os.path.join(save_root, self.data_ids[idx])
            os.makedirs(d, exist_ok=True)
            np.save(os.path.join(d, "flow%d.npy" % (k + 1)), flow_pred[i])

    def _save_predsegm(self, mask_or_hard, save_root, batch_size, n_frame=1, offset=0):
        """(B, N, K) masks or (B, N) hard labels -> <save_root>/<id>/segm<k + 1>.npy, int64 (dataset_kittisf.py:140-152)."""
        _save_frame_labels(mask_or_hard, save_root, batch_size, n_frame, offset, lambda idx: self.data_ids[idx],
                           lambda k: "segm%d.npy" % (k + 1))


class WaymoOpenDataset(Dataset):
    """Reference: datasets/dataset_waymo.py:19-181.  Waymo carries backward scene flow only, so the samples of a sequence of T
    frames are the pairs (t, t - 1), t = 1 .. T - 1, and both entries of `flows` are that one flow.  `select_frame` names a json
    file with the sample ids to use instead; `ignore_class_ids` / `ignore_npoint_thresh` send the points of those semantic
    classes / of objects smaller than that to label 0 and mark them invalid."""

    def __init__(self, data_root, mapping_path, downsampled=False, select_frame=None, sampled_interval=1, predflow_path=None,
                 decentralize=False, aug_transform=False, aug_transform_args=None, ignore_class_ids=(), ignore_npoint_thresh=0):
        import json
        self.data_root = os.path.join(data_root, "data")
        with open(mapping_path, "r") as f:
            self.sequence_list = [line.strip() for line in f if line.strip()]
        self.downsampled = downsampled
        if select_frame is not None:
            with open(select_frame, "r") as f:
                self.data_ids = [(str(seq), int(a), int(b)) for seq, a, b in json.load(f)]
        else:
            self.data_ids = self._make_dataset(sampled_interval)
        self.predflow_path = os.path.join(data_root, "flow_preds", predflow_path) if predflow_path is not None else None
        self.decentralize = decentralize
        self.aug_transform, self.aug_transform_args = aug_transform, aug_transform_args
        self.ignore_class_ids, self.ignore_npoint_thresh = list(ignore_class_ids), ignore_npoint_thresh

    def _make_dataset(self, sampled_interval):
        """Listed sequences that are not on disk are passed over (`n_skipped` counts them)."""
        import glob
        data_ids, self.n_skipped = [], 0
        for entry in self.sequence_list:
            name = os.path.splitext(entry)[0]          # the split files list the .tfrecord names
            d = os.path.join(self.data_root, name)
            if not os.path.isdir(d):
                self.n_skipped += 1
                continue
            n_frame = len(glob.glob(os.path.join(d, "pc_*")))
            data_ids += [(name, t, t - 1) for t in range(1, n_frame)]
        return data_ids[::sampled_interval] if sampled_interval > 1 else data_ids

    def __len__(self):
        return len(self.data_ids)

    def _load_data(self, name, view1, view2):
        d = os.path.join(self.data_root, name)
        return tuple([np.load(os.path.join(d, "%s_%04d.npy" % (what, v))) for v in (view1, view2)]
                     for what in ("pc", "segm", "semantic_segm"))

    def _load_flow(self, name, view1, view2):
        flow = np.load(os.path.join(self.data_root, name, "flow_%04d_%04d.npy" % (view1, view2)))
        return [flow, flow]

    def _load_predflow(self, name, view1, view2):
        path = os.path.join(self.predflow_path, name, "flow_%04d_%04d.npy" % (view1, view2))
        if not os.path.isfile(path):
            raise FileNotFoundError("no predicted flow %s" % path)
        flow = np.load(path)
        return [flow, flow]

    def filter_segm(self, segms, semantic_segms):
        """-> (labels with the ignored points at 0, validity 0 / 1 int32), per frame (dataset_waymo.py:110-128)."""
        filtered, valids = [], []
        for segm, semantic in zip(segms, semantic_segms):
            ids, sizes = np.unique(segm, return_counts=True)
            ignore = np.logical_or(np.isin(semantic, self.ignore_class_ids),
                                   np.isin(segm, ids[sizes < self.ignore_npoint_thresh]))
            filtered.append(np.where(ignore, 0, segm).astype(segm.dtype))
            valids.append(1 - ignore.astype(np.int32))
        return filtered, valids

    def __getitem__(self, sid):
        name, view1, view2 = self.data_ids[sid]
        pcs, segms, semantic_segms = self._load_data(name, view1, view2)
        flows = (self._load_predflow if self.predflow_path is not None else self._load_flow)(name, view1, view2)
        segms, valids = self.filter_segm(segms, semantic_segms)
        if not self.downsampled:      # the full scans: two frames with their own numbers of points, as loaded
            return pcs, segms, flows, valids
        return _finish(pcs, segms, flows, self.decentralize, self.aug_transform, self.aug_transform_args, valids)

    def _save_predflow(self, flow_pred, save_root, batch_size, n_frame=1, offset=0):
        """flow_pred (B, N, 3): sample `(offset * batch_size + i) // n_frame` -> <save_root>/<sequence>/flow_%04d_%04d.npy
        (dataset_waymo.py:169-181)."""
        flow_pred = flow_pred.detach().cpu().numpy() if hasattr(flow_pred, "detach") else np.asarray(flow_pred)
        for i in range(flow_pred.shape[0]):
            name, view1, view2 = self.data_ids[(offset * batch_size + i) // n_frame]
            d = os.path.join(save_root, name)
            os.makedirs(d, exist_ok=True)
            np.save(os.path.join(d, "flow_%04d_%04d.npy" % (view1, view2)), flow_pred[i])


class WaymoSingleFrameDataset(WaymoOpenDataset):
    """Reference: datasets/dataset_waymo_singleframe.py:54-206 (its class is also called WaymoOpenDataset).  One frame per
    sample, id (sequence, t); a sample is (pcs (1, N, 3) f32, segms (1, N) i32, valids (1, N) i32) with the ignored points —
    semantic classes `ignore_class_ids`, objects below `ignore_npoint_thresh` — at label 0 and valid 0.  With `onehot_label`
    segms is (1, N, max_n_object) f32, one-hot over the ranks of the filtered labels times valid, and valids is f32.  With
    `aug_transform` the frame is doubled for the augmentation and views 0 and 2 — the two transforms of the one frame — come
    back as pcs (2, N, 3), while segms and valids are repeated to two entries: the reference's shapes, kept.  With
    downsampled=False the three items are one-element lists as loaded."""

    def __init__(self, data_root, mapping_path, downsampled=False, select_frame=None, sampled_interval=1, decentralize=False,
                 aug_transform=False, aug_transform_args=None, onehot_label=False, max_n_object=20, ignore_class_ids=(),
                 ignore_npoint_thresh=0):
        import json
        self.data_root = os.path.join(data_root, "data")
        with open(mapping_path, "r") as f:
            self.sequence_list = [line.strip() for line in f if line.strip()]
        self.downsampled = downsampled
        if select_frame is not None:
            with open(select_frame, "r") as f:
                self.data_ids = [(str(seq), int(t)) for seq, t in json.load(f)]
        else:
            self.data_ids = self._make_dataset(sampled_interval)
        self.decentralize = decentralize
        self.aug_transform, self.aug_transform_args = aug_transform, aug_transform_args
        self.onehot_label, self.max_n_object = onehot_label, max_n_object
        self.ignore_class_ids, self.ignore_npoint_thresh = list(ignore_class_ids), ignore_npoint_thresh

    def _make_dataset(self, sampled_interval):
        """Every frame of every listed sequence that is on disk (`n_skipped` counts the others)."""
        import glob
        data_ids, self.n_skipped = [], 0
        for entry in self.sequence_list:
            name = os.path.splitext(entry)[0]
            d = os.path.join(self.data_root, name)
            if not os.path.exists(d):
                self.n_skipped += 1
                continue
            data_ids += [(name, t) for t in range(len(glob.glob(os.path.join(d, "pc_*"))))]
        return data_ids[::sampled_interval] if sampled_interval > 1 else data_ids

    def _load_data(self, name, view):
        d = os.path.join(self.data_root, name)
        return tuple([np.load(os.path.join(d, "%s_%04d.npy" % (what, view)))] for what in ("pc", "segm", "semantic_segm"))

    def __getitem__(self, sid):
        name, view = self.data_ids[sid]
        pcs, segms, semantic_segms = self._load_data(name, view)
        segms, valids = self.filter_segm(segms, semantic_segms)
        if not self.downsampled:
            return pcs, segms, valids
        pcs, segms, valids = np.stack(pcs, 0), np.stack(segms, 0), np.stack(valids, 0)
        if self.decentralize:
            pcs = pcs - pcs.mean(1).mean(0)
        segms = np.stack([compress_label_id(segm) for segm in segms], 0)
        if self.onehot_label:
            assert self.max_n_object > 0, 'max_n_object must be above 0!'
            segms = np.eye(self.max_n_object, dtype=np.float32)[segms] * np.expand_dims(valids, 2)
        if self.aug_transform:       # the frame as both frames of a pair with zero flows; views 0 and 2 are its two transforms
            pcs = np.concatenate((pcs, pcs), 0)
            pcs, _ = augment_transform(pcs, np.zeros_like(pcs), self.aug_transform_args)
            pcs = pcs[[0, 2]]
            segms, valids = np.concatenate((segms, segms), 0), np.concatenate((valids, valids), 0)
        if self.onehot_label:
            return pcs.astype(np.float32), segms.astype(np.float32), valids.astype(np.float32)
        return pcs.astype(np.float32), segms.astype(np.int32), valids.astype(np.int32)

    def _load_flow(self, name, view1, view2):
        raise NotImplementedError("the single-frame reader has no flows")

    _load_predflow = _save_predflow = _load_flow

    def _save_predsegm(self, mask_or_hard, save_root, batch_size, n_frame=1, offset=0):
        """(B, N, K) masks or (B, N) hard labels -> <save_root>/<sequence>/segm_%04d.npy, int64; sample `offset * batch_size + i`
        (dataset_waymo_singleframe.py:194-206, which does not divide by n_frame)."""
        hard = _hard_labels(mask_or_hard)
        for i in range(hard.shape[0]):
            name, view = self.data_ids[offset * batch_size + i]
            os.makedirs(os.path.join(save_root, name), exist_ok=True)
            np.save(os.path.join(save_root, name, "segm_%04d.npy" % view), hard[i])


def compute_flow(pc1, segm1, pose1, pose2):
    """Per-point flow of frame 1 from the objects' pose change; object ids start at 1, id 0 (background) stays put
    (dataset_ogcdr.py:10-27)."""
    flow = np.zeros_like(pc1)
    for k in range(pose1.shape[0]):
        rel = pose2[k] @ np.linalg.inv(pose1[k])
        sel = segm1 == (k + 1)
        flow[sel] = pc1[sel] @ rel[:3, :3].T + rel[:3, 3] - pc1[sel]
    return flow


class OGCDynamicRoomDataset(Dataset):
    def __init__(self, data_root, split="train", view_sels=[[0, 1]], predflow_path=None, decentralize=False, aug_transform=False,
                 aug_transform_args=None, onehot_label=False, max_n_object=8):
        self.onehot_label, self.max_n_object = onehot_label, max_n_object
        self.data_root = os.path.join(data_root, "data")
        self.split = split
        with open(os.path.join(self.data_root, split + ".lst"), "r") as f:
            self.data_ids = f.read().strip().split("\n")
        self.view_sels = [list(v) for v in view_sels]
        self.predflow_path, self.pf_view_sels = None, None
        if predflow_path is not None:
            self.predflow_path = os.path.join(data_root, "flow_preds", predflow_path)
            self.pf_view_sels = flow_store.read_meta(self.predflow_path)
            if self.pf_view_sels is None:
                raise FileNotFoundError(self.predflow_path + ".json")
            if any(sel not in self.pf_view_sels for sel in self.view_sels):
                raise ValueError("Flow predictions cannot cover specified view selections!")
        self.decentralize = decentralize
        self.aug_transform, self.aug_transform_args = aug_transform, aug_transform_args

    def __len__(self):
        return len(self.data_ids) * len(self.view_sels)

    def _load_data(self, idx, view_sel):
        d = os.path.join(self.data_root, self.data_ids[idx])
        return tuple([np.load(os.path.join(d, "%s_%02d.npy" % (what, v))) for v in view_sel] for what in ("pc", "segm", "pose"))

    def __getitem__(self, sid):
        idx, view_sel = sid // len(self.view_sels), self.view_sels[sid % len(self.view_sels)]
        pcs, segms, poses = self._load_data(idx, view_sel)
        if self.predflow_path is not None:
            flows = flow_store.load_pair(self.predflow_path, self.data_ids[idx], view_sel, self.pf_view_sels)
        else:
            flows = [compute_flow(pcs[0], segms[0], poses[0], poses[1]), compute_flow(pcs[1], segms[1], poses[1], poses[0])]
        return _finish(pcs, segms, flows, self.decentralize, self.aug_transform, self.aug_transform_args,
                       onehot=(self.max_n_object, 0) if self.onehot_label else None)

    def _save_predflow(self, flow_pred, save_root, batch_size, n_frame=1, offset=0):
        """flow_pred (B, N, 3), the n_frame ordered pairs of a scene adjacent -> <save_root>/<id>.npy (n_frame, N, 3)
        (dataset_ogcdr.py:147-157)."""
        flow_pred = flow_pred.detach().cpu().numpy() if hasattr(flow_pred, "detach") else np.asarray(flow_pred)
        for i in range(flow_pred.shape[0] // n_frame):
            idx = offset * batch_size // n_frame + i
            np.save(os.path.join(save_root, self.data_ids[idx] + ".npy"), flow_pred[i * n_frame:(i + 1) * n_frame])

    def _save_predsegm(self, mask_or_hard, save_root, batch_size, n_frame=1, offset=0):
        """(B, N, K) masks or (B, N) hard labels -> <save_root>/<id>/segm_%02d.npy, int64 (dataset_ogcdr.py:160-172)."""
        _save_frame_labels(mask_or_hard, save_root, batch_size, n_frame, offset, lambda idx: self.data_ids[idx],
                           lambda k: "segm_%02d.npy" % k)


def _rigid_inverse(m):
    """Inverse of a 4x4 rigid transform as (R^T, -R^T t) — what the reference's Isometry.inv() computes on (quaternion, t)
    (utils/sapien_util.py:49-51), not a general matrix inverse."""
    out = np.eye(4, dtype=np.float64)
    out[:3, :3] = m[:3, :3].T
    out[:3, 3] = -(m[:3, :3].T @ m[:3, 3])
    return out


def compute_part_flow(base_pc, base_segms, base_cam, base_motions, dest_cam, dest_motions):
    """Flow of a SAPIEN frame from its parts' motions: part k (label k + 1) moves by
    dest_cam^-1 . dest_motion_k . base_motion_k^-1 . base_cam (all 4x4, camera-to-world and part-to-world);
    points of no part keep whatever np.empty_like holds in the reference — here 0 (datasets/dataset_sapien.py:12-20)."""
    final_pc = base_pc.astype(np.float64).copy()
    for k in range(len(base_motions)):
        sel = np.where(base_segms == (k + 1))[0]
        rel = _rigid_inverse(dest_cam) @ dest_motions[k] @ _rigid_inverse(base_motions[k]) @ base_cam
        final_pc[sel] = base_pc[sel] @ rel[:3, :3].T + rel[:3, 3]
    return (final_pc - base_pc).astype(base_pc.dtype)


class SapienDataset(Dataset):
    """Reference: datasets/dataset_sapien.py:22-170."""

    def __init__(self, data_root, split="train", view_sels=[[0, 1]], predflow_path=None, decentralize=False, aug_transform=False,
                 aug_transform_args=None, onehot_label=False, max_n_object=8):
        import json
        self.onehot_label, self.max_n_object = onehot_label, max_n_object
        self.data_root = os.path.join(data_root, "data")
        with open(os.path.join(data_root, "meta.json")) as f:
            self.meta = json.load(f)
        self.split, self.data_ids = split, self.meta[split]
        self.view_sels = [list(v) for v in view_sels]
        self.predflow_path, self.pf_view_sels = None, None
        if predflow_path is not None:
            self.predflow_path = os.path.join(data_root, "flow_preds", predflow_path)
            self.pf_view_sels = flow_store.read_meta(self.predflow_path)
            if self.pf_view_sels is None:
                raise FileNotFoundError(self.predflow_path + ".json")
            if any(sel not in self.pf_view_sels for sel in self.view_sels):
                raise ValueError("Flow predictions cannot cover specified view selections!")
        self.decentralize = decentralize
        self.aug_transform, self.aug_transform_args = aug_transform, aug_transform_args

    def __len__(self):
        return len(self.data_ids) * len(self.view_sels)

    def _name(self, idx):
        return "%06d" % self.data_ids[idx]

    def _load_data(self, idx):
        data = np.load(os.path.join(self.data_root, self._name(idx) + ".npz"), allow_pickle=True)
        return data["pc"].astype(np.float32), data["segm"], data["trans"].item()

    def __getitem__(self, sid):
        idx, view_sel = sid // len(self.view_sels), self.view_sels[sid % len(self.view_sels)]
        pcs, segms, trans = self._load_data(idx)
        n_parts = len(trans) - 1
        a, b = view_sel
        pcs, segms = pcs[view_sel], segms[view_sel]
        if self.predflow_path is not None:
            flows = flow_store.load_pair(self.predflow_path, self._name(idx), view_sel, self.pf_view_sels)
            if flows is None:
                raise FileNotFoundError(os.path.join(self.predflow_path, self._name(idx) + ".npy"))
        else:
            def motions(v):
                return [np.asarray(trans[t][v], dtype=np.float64) for t in range(1, n_parts + 1)]
            cam = lambda v: np.asarray(trans["cam"][v], dtype=np.float64)
            flows = [compute_part_flow(pcs[0], segms[0], cam(a), motions(a), cam(b), motions(b)),
                     compute_part_flow(pcs[1], segms[1], cam(b), motions(b), cam(a), motions(a))]
        return _finish(list(pcs), list(segms), flows, self.decentralize, self.aug_transform, self.aug_transform_args,
                       onehot=(self.max_n_object, 0) if self.onehot_label else None)

    def _save_predflow(self, flow_pred, save_root, batch_size, n_frame=1, offset=0):
        """flow_pred (B, N, 3), the n_frame ordered pairs of a scene adjacent -> <save_root>/%06d.npy (n_frame, N, 3)
        (dataset_sapien.py:140-151)."""
        flow_pred = flow_pred.detach().cpu().numpy() if hasattr(flow_pred, "detach") else np.asarray(flow_pred)
        for i in range(flow_pred.shape[0] // n_frame):
            idx = offset * batch_size // n_frame + i
            np.save(os.path.join(save_root, self._name(idx) + ".npy"), flow_pred[i * n_frame:(i + 1) * n_frame])

    def _save_predsegm(self, mask_or_hard, save_root, batch_size, n_frame=1, offset=0):
        """(B, N, K) masks or (B, N) hard labels -> <save_root>/%06d/segm_%02d.npy, int64 (dataset_sapien.py:158-170)."""
        _save_frame_labels(mask_or_hard, save_root, batch_size, n_frame, offset, self._name, lambda k: "segm_%02d.npy" % k)


class _SingleFrameDataset(Dataset):
    """The sample contract of the two single-frame sets (dataset_kittidet.py:73-114, dataset_semantickitti.py:53-85): centring
    on the frame's own mean, labels compressed per frame, the frame duplicated to two views, zero flows, valids of ones.
    `onehot_label` (KITTI-Det): one-hot masks and the valids of batch_segm_to_mask instead (dataset_kittidet.py:95-112).
    `predsegm_path` (KITTI-Det): the labels come from <predsegm_path>/<id>/segm.npy instead of the ground truth, and under
    `onehot_label` every object's column is scaled by its confidence (dataset_kittidet.py:63-70, :77-79, :92-101)."""
    onehot_label, max_n_object, ignore_npoint_thresh = False, 18, 0
    predsegm_path, load_confidence = None, False

    def __len__(self):
        return len(self.data_ids)

    def _load_data(self, idx):
        d = os.path.join(self.data_root, self.data_ids[idx])
        return np.load(os.path.join(d, "pc.npy")), np.load(os.path.join(d, "segm.npy"))

    def _load_predsegm(self, idx):
        """-> (labels, confidences) of a saved prediction; ones(max_n_object) without `load_confidence`."""
        d = os.path.join(self.predsegm_path, self.data_ids[idx])
        segm = np.load(os.path.join(d, "segm.npy"))
        if self.load_confidence:
            conf = np.load(os.path.join(d, "conf.npy")).astype(np.float32)
        else:
            conf = np.ones((self.max_n_object), dtype=np.float32)
        return segm, conf

    def __getitem__(self, sid):
        pc, segm = self._load_data(sid)
        if self.predsegm_path is not None:
            segm, conf = self._load_predsegm(sid)
        if self.decentralize:
            pc = pc - pc.mean(0)
        segm = compress_label_id(segm)
        pcs, segms = np.stack([pc, pc], 0), np.stack([segm, segm], 0)
        flows = np.zeros_like(pcs)
        if self.onehot_label and self.predsegm_path is not None:
            assert self.max_n_object > 0, 'max_n_object must be above 0!'
            segms, valids = batch_segm_to_mask_withconf(segms, [conf, conf], self.max_n_object, self.ignore_npoint_thresh)
        elif self.onehot_label:
            segms, valids = _one_hot(segms, self.max_n_object, self.ignore_npoint_thresh)
        else:
            valids = np.ones_like(segms, dtype=np.float32)
        if self.aug_transform:
            pcs, flows = augment_transform(pcs, flows, self.aug_transform_args)
            segms = np.concatenate((segms, segms), 0)
            valids = np.concatenate((valids, valids), 0)
        return (pcs.astype(np.float32), segms.astype(np.float32 if self.onehot_label else np.int32), flows.astype(np.float32),
                valids.astype(np.float32))

    def _save_predsegm(self, mask_or_hard, save_root, batch_size, n_frame=1, offset=0, conf=None):
        """(B, N, K) masks or (B, N) hard labels -> <save_root>/<id>/segm.npy, int64; sample `offset * batch_size + i`, whatever
        n_frame (dataset_kittidet.py:117-129).  `conf`: one array of confidences per sample (metrics/seg_conf.py), written as
        float32 to <save_root>/<id>/conf.npy beside it — the file `load_confidence` reads; the reference has no writer of it."""
        _save_frame_labels(mask_or_hard, save_root, batch_size, 1, offset, lambda idx: self.data_ids[idx],
                           lambda k: "segm.npy")
        for i, c in enumerate(conf if conf is not None else ()):
            np.save(os.path.join(save_root, self.data_ids[offset * batch_size + i], "conf.npy"), np.asarray(c, dtype=np.float32))


class KITTIDetectionDataset(_SingleFrameDataset):
    """Reference: datasets/dataset_kittidet.py:9-129.  `load_prediction`: train on the segmentations another model saved under
    <data_root>/segm_preds/<load_prediction> (test_seg.py --save) instead of the ground truth; `load_confidence`: scale every
    object's target column by the confidence in conf.npy beside them (export_pseudo_labels.py), ones otherwise."""

    def __init__(self, data_root, mapping_path, decentralize=False, aug_transform=False, aug_transform_args=None,
                 onehot_label=False, max_n_object=18, ignore_npoint_thresh=0, load_prediction=None, load_confidence=False):
        self.onehot_label, self.max_n_object, self.ignore_npoint_thresh = onehot_label, max_n_object, ignore_npoint_thresh
        self.predsegm_path = None if load_prediction is None else os.path.join(data_root, "segm_preds", load_prediction)
        self.load_confidence = load_confidence
        self.data_root = os.path.join(data_root, "downsampled")
        with open(mapping_path, "r") as f:
            self.data_ids = f.read().strip().split("\n")
        self.decentralize = decentralize
        self.aug_transform, self.aug_transform_args = aug_transform, aug_transform_args


class SemanticKITTIDataset(_SingleFrameDataset):
    """Reference: datasets/dataset_semantickitti.py:9-100.  `sequence_list` None takes every frame (the reference leaves
    `data_ids` undefined there)."""

    def __init__(self, data_root, sequence_list=None, decentralize=False, aug_transform=False, aug_transform_args=None):
        self.data_root = os.path.join(data_root, "downsampled")
        data_ids = sorted(os.listdir(self.data_root))
        if sequence_list is not None:
            data_ids = [idx for idx in data_ids if int(idx[:2]) in sequence_list]
        self.data_ids = data_ids
        self.decentralize = decentralize
        self.aug_transform, self.aug_transform_args = aug_transform, aug_transform_args

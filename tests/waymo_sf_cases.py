"""Shared by tests/golden/make_waymo_singleframe_golden.py (the reference's single-frame Waymo reader) and
tests/test_waymo_singleframe.py (ogc_amd.datasets.WaymoSingleFrameDataset): the seeded synthetic root and the reader cases."""
import numpy as np

SEED = 77
N_POINTS, N_FRAMES, THRESH = 384, 3, 30
AUG_ARGS = {"scale_low": 0.95, "scale_high": 1.05, "degree_range": [0, 180, 0], "shift_range": [1, 0.1, 1]}
SAVE_BATCH, SAVE_SLOTS = 2, 5

CASES = (   # (tag, split, keyword arguments on top of reader_kwargs' defaults)
    ("plain", "train", {}),
    ("onehot", "train", {"onehot_label": True}),
    ("aug", "train", {"aug_transform": True, "aug_transform_args": AUG_ARGS}),
    ("onehot_aug", "train", {"onehot_label": True, "aug_transform": True, "aug_transform_args": AUG_ARGS, "decentralize": False}),
    ("full", "val", {"downsampled": False}),
    ("select", "train", {"select_frame": True}),
    ("interval", "train", {"sampled_interval": 2}),
    ("no_filter", "val", {"ignore_class_ids": [], "ignore_npoint_thresh": 0}),
)


def write_root(root):
    from ogc_amd.utils.synthetic import write_waymo_singleframe_roots
    return write_waymo_singleframe_roots(root, 2, 1, N_FRAMES, N_POINTS, seed=8100, small_object=12)


def reader_kwargs(root, made, split, extra):
    kwargs = dict(data_root=root, mapping_path=made[split]["mapping"], downsampled=True, decentralize=True, max_n_object=12,
                  ignore_class_ids=[2, 3], ignore_npoint_thresh=THRESH)
    kwargs.update(extra)
    if kwargs.get("select_frame") is True:
        kwargs["select_frame"] = made[split]["select_frame"]
    return kwargs


def save_masks():
    """(6, N_POINTS, SAVE_SLOTS) soft masks for the six samples of the `plain` case."""
    return np.random.RandomState(SEED).rand(2 * N_FRAMES, N_POINTS, SAVE_SLOTS).astype(np.float32)

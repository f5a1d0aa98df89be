"""Shared by tests/golden/make_waymo_sup_golden.py (the reference's train_seg_waymo_sup.Trainer) and
tests/test_waymo_sup_driver.py (ogc_amd.train_seg_waymo_sup.Trainer): the replay's data set — the scenes, configuration and
NaN-gradient step of the supervised replay (tests/sup_cases.py) with the sample contract of the single-frame Waymo reader."""
import numpy as np
import torch

import sup_cases as sc

CFG = dict(sc.SUP_CFG, dataset="waymo")


class WaymoSupScenes(torch.utils.data.Dataset):
    """sup_cases.SupScenes as (pcs, segms one-hot, valids): no flows.  `poisoned` is that set's flag (nan_gradient_hook)."""

    def __init__(self, train=True, seed=0, ulp=0, dtype=np.float32):
        self.inner = sc.SupScenes(train, seed, ulp, dtype)

    @property
    def poisoned(self):
        return self.inner.poisoned

    def __len__(self):
        return len(self.inner)

    def __getitem__(self, i):
        pcs, masks, _, valids = self.inner[i]
        return pcs, masks, valids

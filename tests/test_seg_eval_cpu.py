"""CPU-side checks of ogc_seg_eval and ogc_amd.metrics.seg_eval: the entry point is exported and bound, refuses bad sizes and
null pointers before anything is launched (so these calls need no GPU), and the Python layer has no CPU path."""
import ctypes
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def test_seg_eval_has_no_cpu_path():
    from ogc_amd.metrics.seg_eval import accumulate_seg_eval, seg_eval_batch
    segm, mask = torch.zeros(2, 8, dtype=torch.int64), torch.full((2, 8, 4), 0.25)
    for fn in (seg_eval_batch, accumulate_seg_eval):
        with pytest.raises(RuntimeError) as err:
            fn(segm, mask)
        assert "no CPU path" in str(err.value)
    with pytest.raises(TypeError):
        seg_eval_batch(segm, mask.double())
    with pytest.raises(TypeError):
        seg_eval_batch(segm.float(), mask)
    with pytest.raises(TypeError):
        seg_eval_batch(segm.numpy(), mask)
    with pytest.raises(TypeError):
        seg_eval_batch(segm, np.zeros((2, 8, 4), np.float32))


def test_entry_point_is_exported_bound_and_refuses_before_launching():
    from ogc_amd import _lib, pointnet2_cuda
    from ogc_amd.csrc import build as b
    lib = ctypes.CDLL(b.build())
    assert hasattr(lib, "ogc_seg_eval") and "ogc_seg_eval" in _lib.SIGNATURES and callable(pointnet2_cuda.seg_eval_wrapper)
    header = open(os.path.join(os.path.dirname(HERE), "include", "ogc_ops.h")).read()
    assert "#define OGC_SEG_EVAL_MAX_LABELS 64" in header and "#define OGC_VERSION 208" in header
    fn = lib.ogc_seg_eval
    fn.argtypes, fn.restype = _lib.SIGNATURES["ogc_seg_eval"], ctypes.c_int
    lib.ogc_last_error.restype = ctypes.c_char_p
    null = [None] * 10

    def call(B, n, k, thresh):
        return fn(B, n, k, None, None, thresh, *null, None), lib.ogc_last_error().decode()
    assert call(0, 16, 4, 0)[0] == 0                    # B == 0 is a no-op whatever else is passed
    for args, word in (((2, 0, 4, 0), "at least one point"), ((2, 16, 0, 0), "k = 0"), ((2, 16, 65, 0), "k = 65"),
                       ((-1, 16, 4, 0), "negative batch"), ((2, 16, 4, -1), "ignore_npoint_thresh"),
                       ((2, 16, 4, 0), "null pointer")):
        rc, message = call(*args)
        assert rc == -1 and word in message, (args, message)

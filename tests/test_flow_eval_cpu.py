"""CPU-side checks of ogc_flow_eval and ogc_amd.metrics.flow_eval: the entry point is exported and bound, refuses bad arguments
and null pointers before anything is launched (so these calls need no GPU), and the Python layer has no CPU path."""
import ctypes
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def test_flow_eval_has_no_cpu_path():
    from ogc_amd.metrics.flow_eval import eval_flow_device, flow_eval_batch
    gt, pred = torch.zeros(2, 8, 3), torch.full((2, 8, 3), 0.25)
    for fn in (flow_eval_batch, eval_flow_device):
        with pytest.raises(RuntimeError) as err:
            fn(gt, pred)
        assert "no CPU path" in str(err.value)
    with pytest.raises(TypeError):
        flow_eval_batch(gt.double(), pred)
    with pytest.raises(TypeError):
        flow_eval_batch(gt, pred.double())
    with pytest.raises(TypeError):
        flow_eval_batch(gt.numpy(), pred)
    with pytest.raises(TypeError):
        flow_eval_batch(gt, np.zeros((2, 8, 3), np.float32))


def test_entry_point_is_exported_bound_and_refuses_before_launching():
    from ogc_amd import _lib, pointnet2_cuda
    from ogc_amd.csrc import build as b
    assert "flow_eval.hip" in b.SOURCES
    lib = ctypes.CDLL(b.build())
    assert hasattr(lib, "ogc_flow_eval") and "ogc_flow_eval" in _lib.SIGNATURES and callable(pointnet2_cuda.flow_eval_wrapper)
    header = open(os.path.join(os.path.dirname(HERE), "include", "ogc_ops.h")).read()
    assert "int ogc_flow_eval(" in header and "#define OGC_VERSION 208" in header and _lib.HEADER_VERSION == 208
    fn = lib.ogc_flow_eval
    fn.argtypes, fn.restype = _lib.SIGNATURES["ogc_flow_eval"], ctypes.c_int
    lib.ogc_last_error.restype = ctypes.c_char_p

    def call(B, N, thresh, eps):
        return fn(B, N, None, None, thresh, eps, None, None, None), lib.ogc_last_error().decode()
    assert call(0, 16, 0.05, 1e-10)[0] == 0             # B == 0 is a no-op whatever else is passed
    assert call(0, -3, float("nan"), -1.0)[0] == 0
    nan, inf = float("nan"), float("inf")
    for args, word in (((-1, 16, 0.05, 1e-10), "negative batch"), ((2, 0, 0.05, 1e-10), "at least one point"),
                       ((2, -5, 0.05, 1e-10), "at least one point"), ((2, 16, 0.0, 1e-10), "epe_norm_thresh"),
                       ((2, 16, -0.05, 1e-10), "epe_norm_thresh"), ((2, 16, nan, 1e-10), "epe_norm_thresh"),
                       ((2, 16, inf, 1e-10), "epe_norm_thresh"), ((2, 16, 0.05, -1e-10), "eps ="), ((2, 16, 0.05, nan), "eps ="),
                       ((2, 16, 0.05, inf), "eps ="), ((2, 16, 0.05, 1e-10), "null pointer"), ((2, 16, 0.05, 0.0), "null pointer")):
        rc, message = call(*args)
        assert rc == -1 and word in message and message.startswith("ogc_flow_eval"), (args, message)

"""Classical point-to-point ICP on the device (reference: utils/icp_util.py:73-124, sklearn + numpy on the CPU).

`icp_batch` is the operator: B pairs, one launch of ogc_rigid_icp (csrc/rigid_icp.hip) on the current stream, every iteration
inside it, nothing read back — it can be captured in a torch.cuda.graph.  `icp` carries the reference's name, argument order
and return triple for callers written against it.  `rigid_flow` turns a fitted transform into the flow it induces, as the
flow-prediction driver does (test_flow_kittisf.py:104-107).  There is no CPU path.
"""
import numpy as np
import torch

from .. import pointnet2_cuda as _native


def icp_batch(src, dst, init_pose=None, max_iterations=20, tolerance=0.001):
    """src, dst (B, n, 3) fp32 CUDA tensors, init_pose (B, 4, 4) fp64 or None ->
    T (B, 4, 4) fp64, distances (B, n) fp64 (nearest-neighbour distances of the last search), iters (B,) int32 (the
    reference's returned `i`), all on the device."""
    for name, t in (("src", src), ("dst", dst)):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor" % name)
        if t.dtype != torch.float32:
            raise TypeError("%s must be float32, got %s" % (name, t.dtype))
        if t.device.type != "cuda":
            raise RuntimeError("%s must be a CUDA tensor (HIP device); ogc_amd has no CPU path" % name)
    if src.dim() != 3 or src.shape[2] != 3 or src.shape != dst.shape:
        raise ValueError("src and dst must both be (B, n, 3), got %s and %s" % (tuple(src.shape), tuple(dst.shape)))
    B, n = src.shape[0], src.shape[1]
    if init_pose is not None:
        if tuple(init_pose.shape) != (B, 4, 4):
            raise ValueError("init_pose must be (B, 4, 4), got %s" % (tuple(init_pose.shape),))
        init_pose = init_pose.to(device=src.device, dtype=torch.float64).contiguous()
    T = torch.empty(B, 4, 4, dtype=torch.float64, device=src.device)
    distances = torch.empty(B, n, dtype=torch.float64, device=src.device)
    iters = torch.empty(B, dtype=torch.int32, device=src.device)
    _native.rigid_icp_wrapper(B, n, src.contiguous(), dst.contiguous(), init_pose, max_iterations, tolerance, T, distances, iters)
    return T, distances, iters


def _on_device(x, name):
    if isinstance(x, torch.Tensor):
        if x.dtype != torch.float32:
            raise TypeError("%s must be float32, got %s" % (name, x.dtype))
        if x.device.type != "cuda":
            raise RuntimeError("%s must be a CUDA tensor (HIP device); ogc_amd has no CPU path" % name)
        return x
    x = np.asarray(x)
    if x.dtype != np.float32:
        raise TypeError("%s must be float32, got %s" % (name, x.dtype))
    if not torch.cuda.is_available():
        raise RuntimeError("icp needs a HIP device; ogc_amd has no CPU path")
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def icp(A, B, init_pose=None, max_iterations=20, tolerance=0.001):
    """The reference's `icp`: A, B (n, 3) fp32 numpy arrays or CUDA tensors, init_pose (4, 4) or None ->
    (T (4, 4) float64 ndarray, distances (n,) float64 ndarray, i int)."""
    src, dst = _on_device(A, "A"), _on_device(B, "B")
    if src.dim() != 2 or src.shape != dst.shape:
        raise ValueError("A and B must both be (n, 3), got %s and %s" % (tuple(src.shape), tuple(dst.shape)))
    if init_pose is not None:
        init_pose = torch.as_tensor(np.asarray(init_pose.cpu() if isinstance(init_pose, torch.Tensor) else init_pose,
                                               dtype=np.float64)).reshape(1, 4, 4)
    T, distances, iters = icp_batch(src[None], dst[None], init_pose, max_iterations, tolerance)
    return T[0].cpu().numpy(), distances[0].cpu().numpy(), int(iters[0])


def _moved(pc, T):
    T = torch.as_tensor(T, dtype=torch.float64, device=pc.device)
    p = pc.to(torch.float64)
    return torch.einsum("...ij,...nj->...ni", T[..., :3, :3], p) + T[..., None, :3, 3], p


def rigid_apply(pc, T):
    """R pc + t evaluated in float64 and returned as fp32 (test_flow_kittisf.py:111-112).  Shapes as rigid_flow."""
    return _moved(pc, T)[0].to(torch.float32)


def rigid_flow(pc, T):
    """The flow a rigid transform induces, R pc + t - pc, evaluated in float64 and returned as fp32.
    pc (..., N, 3) with T (..., 4, 4) or one (4, 4) for all; tensors on one device (T may be a numpy array)."""
    moved, p = _moved(pc, T)
    return (moved - p).to(torch.float32)

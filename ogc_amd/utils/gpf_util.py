"""Ground-plane fitting on the device (reference: utils/gpf_util.py:20-70, numpy + scikit-spatial on the CPU).

`ground_plane_fit_batch` is the operator: B clouds, one launch of ogc_ground_plane_fit (csrc/ground_plane.hip) on the current
stream — the seed from the lowest points, every plane fit, every retry with a raised seed threshold inside it, nothing read
back — so it can be captured in a torch.cuda.graph.  `plane_mask` labels any set of points against a fitted plane, and
`ground_plane_fitting` carries the reference's name, argument order and result for callers written against it: FPS sample,
fit, label all points.  There is no CPU path.
"""
import numpy as np
import torch

from .. import pointnet2_cuda as _native
from ..pointnet2.pointnet2 import furthest_point_sample


def ground_plane_fit_batch(pc, n_iter=5, n_lpr=200, thresh_seed=0.4, thresh_dist=0.4, vertical_axis=1):
    """pc (B, n, 3) fp32 CUDA tensor -> plane (B, 6) fp64 (centre, unit normal with a vertical component >= 0; zeros where the
    fit gave up), is_ground (B, n) bool, attempts (B,) int32 (the fits started: 1 when the first seed gave a plane), all on
    the device."""
    if not isinstance(pc, torch.Tensor):
        raise TypeError("pc must be a torch.Tensor")
    if pc.dtype != torch.float32:
        raise TypeError("pc must be float32, got %s" % pc.dtype)
    if pc.device.type != "cuda":
        raise RuntimeError("pc must be a CUDA tensor (HIP device); ogc_amd has no CPU path")
    if pc.dim() != 3 or pc.shape[2] != 3:
        raise ValueError("pc must be (B, n, 3), got %s" % (tuple(pc.shape),))
    B, n = pc.shape[0], pc.shape[1]
    plane = torch.empty(B, 6, dtype=torch.float64, device=pc.device)
    is_ground = torch.empty(B, n, dtype=torch.int32, device=pc.device)
    attempts = torch.empty(B, dtype=torch.int32, device=pc.device)
    _native.ground_plane_fit_wrapper(B, n, pc.contiguous(), n_iter, n_lpr, thresh_seed, thresh_dist, vertical_axis, plane,
                                     is_ground, attempts)
    return plane, is_ground.bool(), attempts


def plane_mask(points, plane, thresh_dist):
    """|(points - c) . n| < thresh_dist in float64 (gpf_util.py:68-69): points (..., N, 3), plane (..., 6) or one (6,) for all,
    on one device -> (..., N) bool.  A plane of zeros (a fit that gave up) yields all False."""
    plane = plane.to(torch.float64)
    dist = torch.einsum("...nj,...j->...n", points.to(torch.float64) - plane[..., None, :3], plane[..., 3:]).abs()
    return torch.logical_and(dist < thresh_dist, (plane[..., 3:] != 0).any(-1)[..., None])


def ground_plane_fitting(points, n_sample_point=8192, n_iter=5, n_lpr=200, thresh_seed=0.4, thresh_dist=0.4, vertical_axis=1):
    """The reference's `ground_plane_fitting`: points (N, 3) fp32 -> is_ground (N,) int32; a numpy array in gives a numpy array
    out, a CUDA tensor in a CUDA tensor out.  The plane is fitted to min(n_sample_point, N) FPS samples (to all points when
    n_sample_point <= 0) and every point is labelled against it."""
    as_numpy = not isinstance(points, torch.Tensor)
    if as_numpy:
        points = np.asarray(points)
        if points.dtype != np.float32:
            raise TypeError("points must be float32, got %s" % points.dtype)
        if not torch.cuda.is_available():
            raise RuntimeError("ground_plane_fitting needs a HIP device; ogc_amd has no CPU path")
        pts = torch.from_numpy(np.ascontiguousarray(points)).cuda()
    else:
        if points.dtype != torch.float32:
            raise TypeError("points must be float32, got %s" % points.dtype)
        if points.device.type != "cuda":
            raise RuntimeError("points must be a CUDA tensor (HIP device); ogc_amd has no CPU path")
        pts = points
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError("points must be (N, 3), got %s" % (tuple(pts.shape),))
    pc = pts[None].contiguous()
    if n_sample_point > 0:
        idx = furthest_point_sample(pc, min(n_sample_point, pts.shape[0]))
        pc = pts[idx[0].long()][None].contiguous()
    plane, _, _ = ground_plane_fit_batch(pc, n_iter, n_lpr, thresh_seed, thresh_dist, vertical_axis)
    is_ground = plane_mask(pts, plane[0], thresh_dist).to(torch.int32)
    return is_ground.cpu().numpy() if as_numpy else is_ground

"""Radius outlier removal on the GPU -- the reference's use_radius_outlier_removal (dataset/dataset.py:29-35, Open3D's
remove_radius_outlier(nb_points=3, radius=1)) on librpcc_filter.so, for a batch of point lists on the device.  DESIGN.md
section 17 has the specification; nothing falls back to the CPU."""
from collections import namedtuple

import numpy as np
import torch

from . import _filter_lib as F
from ._lib import RpccError, ptr, stream

RadiusMask = namedtuple("RadiusMask", "keep count kept stats masked")


def workspace_bytes(total, B):
    return F.lib().rpcc_filter_workspace_bytes(int(total), int(B))


def radius_outlier_mask(xyz, offsets, nb_points=3, radius=1.0, brute_force=False, stats=False, masked=False, ws=None):
    """xyz f32 [total,3] -- or the stored rows f32 [total,4] (x, y, z, intensity), read with a 16-byte stride --, offsets i64 [B+1]
    (device tensors) -> RadiusMask(keep bool [total], count int32 [total]: the neighbour count clipped at nb_points + 1, kept int64 [B]:
    kept points per frame, stats: int64 [B,2] pair tests and tiles visited per frame or None, masked: a copy of xyz with x, y, z of every
    removed point NaN or None).  A point is kept when more than nb_points points of its frame, itself included, lie within radius of it
    (strictly, in fp64).  brute_force: every point of the frame tested in fp64, no pruning (the tests' reference).  ws: the caller's work
    buffer of workspace_bytes(total, B) bytes (uint8; allocated here when None).  Queued on the current stream; nothing synchronises."""
    if xyz.dim() != 2 or xyz.shape[1] not in (3, 4):
        raise ValueError("xyz must be [N,3] or [N,4], got %s" % (tuple(xyz.shape),))
    if offsets.dim() != 1 or offsets.numel() < 2 or offsets.dtype != torch.int64:
        raise ValueError("offsets must be int64 [B+1] with B >= 1")
    if xyz.dtype != torch.float32:
        if xyz.shape[1] != 3:
            raise ValueError("stored rows [N,4] must be float32")
        xyz = xyz.to(torch.float32)     # wider inputs are narrowed first, as the projection does
    xyz = xyz.contiguous()
    total, B, dev = int(xyz.shape[0]), offsets.numel() - 1, offsets.device
    if ws is None:
        ws = torch.empty(max(workspace_bytes(total, B), 1), dtype=torch.uint8, device=dev)
    keep = torch.empty((total,), dtype=torch.uint8, device=dev)
    count = torch.empty((total,), dtype=torch.int32, device=dev)
    kept = torch.empty((B,), dtype=torch.int64, device=dev)
    st = torch.empty((B, F.NSTATS), dtype=torch.int64, device=dev) if stats else None
    out = torch.empty_like(xyz) if masked else None
    p = lambda t: ptr(t) if t is not None and t.numel() else None
    F.check(F.lib().rpcc_filter_radius(p(xyz), 4 * int(xyz.shape[1]), ptr(offsets), total, B, float(radius), int(nb_points),
                                       F.BRUTEFORCE if brute_force else 0, p(keep), p(count), ptr(kept), p(out), ptr(st), ptr(ws), stream()))
    return RadiusMask(keep.view(torch.bool), count, kept, st, out)


def remove_radius_outlier(points, nb_points=3, radius=1.0, device=None):
    """points: a host or device [N,>=3] array of any float dtype -> (filtered [n,3], index int64 [n]), as Open3D's
    remove_radius_outlier returns (cloud, index): the kept rows in input order, in the input's dtype, and their positions.  A numpy
    array comes back as numpy arrays, a tensor as tensors on its device.  Raises RpccError without a visible GPU."""
    host = not isinstance(points, torch.Tensor)
    if not torch.cuda.is_available():
        raise RpccError("remove_radius_outlier runs on librpcc_filter.so and needs a GPU; the HIP path has no CPU fallback")
    src = torch.from_numpy(np.ascontiguousarray(np.asarray(points)[:, :3])) if host else points[:, :3]
    dev = torch.device(device) if device is not None else (src.device if src.is_cuda else torch.device("cuda:0"))
    with torch.cuda.device(dev):
        xyz = src.to(dev).to(torch.float32).contiguous()
        offsets = torch.tensor([0, xyz.shape[0]], dtype=torch.int64, device=dev)
        keep = radius_outlier_mask(xyz, offsets, nb_points, radius).keep
        index = torch.nonzero(keep).flatten()      # boolean indexing is stable: input order
        index = index.to(src.device)
    filtered = src[index]
    return (filtered.numpy(), index.numpy()) if host else (filtered, index)

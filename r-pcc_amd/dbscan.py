"""DBSCAN segmentation on the GPU -- the reference's segment_method 'DBSCAN' (utils/segment_utils.py:149-169, Open3D's
cluster_dbscan) on librpcc_seg.so, for a batch of range images on the device.  DESIGN.md section 10 has the
specification; nothing falls back to the CPU."""
import torch

from . import _seg_lib as S
from ._lib import RpccError, ptr, stream


def dbscan_segment(ri, tm, ground, eps, min_points=10, brute_force=False, stats=False, ws=None, check=True):
    """ri f32 [B,H,W], tm f32 [H,W,3], ground f64 [B,4] (device tensors) -> (seg int32 [B,H,W], max_label int32 [B]) in the
    reference's final labels: ground 0, ri == 0 pixels 1, noise 2, cluster k -> k + 3.  stats=True adds an int64 [B,2]
    tensor: pair tests and tiles visited per frame.  brute_force: every candidate tested in fp64, no pruning (the tests'
    reference).  ws: the caller's work buffer of rpcc_seg_workspace_bytes(B, H, W) bytes (uint8; allocated here when None).
    Raises RpccError if a frame's union-find hit its iteration cap (this synchronises the stream).  check=False: max_label is not
    read back -- nothing synchronises, and a capped frame is the caller's to find (max_label == _seg_lib.CAPPED;
    ops.compress_batch_labels gives it the status LABELS_E_CAPPED)."""
    if ri.dim() != 3:
        raise ValueError("ri must be [B,H,W], got %s" % (tuple(ri.shape),))
    B, H, W = ri.shape
    if tuple(tm.shape) != (H, W, 3) or tuple(ground.shape) != (B, 4):
        raise ValueError("tm must be [%d,%d,3] and ground [%d,4]" % (H, W, B))
    if ri.dtype != torch.float32 or tm.dtype != torch.float32 or ground.dtype != torch.float64:
        raise ValueError("ri and tm are float32, ground float64")
    dev = ri.device
    if ws is None:
        ws = torch.empty(max(S.lib().rpcc_seg_workspace_bytes(B, H, W), 1), dtype=torch.uint8, device=dev)
    seg = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    mx = torch.empty((B,), dtype=torch.int32, device=dev)
    st = torch.empty((B, S.NSTATS), dtype=torch.int64, device=dev) if stats else None
    S.check(S.lib().rpcc_seg_dbscan(ptr(ri), ptr(tm), ptr(ground), B, H, W, float(eps), int(min_points),
                                    S.BRUTEFORCE if brute_force else 0, ptr(seg), ptr(mx), ptr(st), ptr(ws), stream()))
    if check and bool((mx == S.CAPPED).any()):
        raise RpccError("librpcc_seg: a union-find loop hit its iteration cap (frames %s)"
                        % (torch.nonzero(mx == S.CAPPED).flatten().tolist(),))
    return (seg, mx, st) if stats else (seg, mx)

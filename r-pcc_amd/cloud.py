"""The rows of the .bin file of a frame whose cloud is "image points, then a variable number of extra points" (the hidden_points
trailer), made on the device: rows.py's rule over both segments -- a point is kept iff (x + y) + z, in fp32 and in that order, is != 0;
the kept pixels in raster order, then the kept extra points in their order, become float32 rows (x, y, z, w), bits unchanged; w is the
intensity of a pixel row (+0.0 without one) and +0.0 for an extra row.  pack() is the device call (librpcc_cloud.so, no CPU fallback);
the host counterpart is rows.pack_host over the concatenated points with tools.decompress.point_intensity.  DESIGN.md section 26."""


def pack(pc, intensity=None, ri_rec=None, extra=None, extra_count=None, rows=None, table=None, nonzero=None, base=None):
    """rows.pack's arguments and results, plus extra: f32 [B,capacity,3] device tensor or None, extra_count: i32 [B] device tensor read on
    the device -- frame b contributes extra[b][:min(max(extra_count[b], 0), capacity)].  rows defaults to B*(P+capacity) rows, which always
    suffice.  With extra=None the results are rows.pack's, bit for bit.  Raises RpccError without a GPU."""
    import torch
    from . import _cloud_lib as R
    from ._lib import RpccError, ptr, stream
    if not isinstance(pc, torch.Tensor) or not pc.is_cuda:
        raise RpccError("cloud.pack runs on librpcc_cloud.so and needs a GPU tensor; the HIP path has no CPU fallback (host arrays: rows.pack_host)")
    if pc.dtype != torch.float32 or pc.dim() < 3 or pc.shape[-1] != 3:
        raise ValueError("pc must be float32 [B,P,3] or [B,H,W,3], got %s %s" % (pc.dtype, tuple(pc.shape)))
    B, dev = pc.shape[0], pc.device
    P = pc.numel() // (3 * B) if B else 0
    for name, t in (("intensity", intensity), ("ri_rec", ri_rec)):
        if t is not None and (t.dtype != torch.float32 or t.device != dev or t.shape[0] != B or t.numel() != B * P):
            raise ValueError("%s must be float32 [%d,%d] on %s" % (name, B, P, dev))
    cap = 0
    if extra is not None:
        if extra.dtype != torch.float32 or extra.dim() != 3 or extra.shape[0] != B or extra.shape[2] != 3 or extra.device != dev or not extra.is_contiguous():
            raise ValueError("extra must be a contiguous float32 [%d,capacity,3] on %s" % (B, dev))
        if extra_count is None or extra_count.dtype != torch.int32 or extra_count.numel() != B or extra_count.device != dev:
            raise ValueError("extra_count must be int32 [%d] on %s" % (B, dev))
        cap = extra.shape[1]
    if rows is None:
        rows = torch.empty((B * (P + cap), 4), dtype=torch.float32, device=dev)
    elif rows.dtype != torch.float32 or rows.dim() != 2 or rows.shape[1] != 4 or rows.device != dev:
        raise ValueError("rows must be float32 [capacity,4] on %s" % (dev,))
    if table is None:
        table = torch.empty((R.table_words(B),), dtype=torch.int64, device=dev)
    elif table.dtype != torch.int64 or table.numel() != R.table_words(B) or table.device != dev:
        raise ValueError("table must be int64 [%d] on %s" % (R.table_words(B), dev))
    if ri_rec is None:
        nonzero = None
    elif nonzero is None:
        nonzero = torch.empty((B,), dtype=torch.int32, device=dev)
    elif nonzero.dtype != torch.int32 or nonzero.numel() != B or nonzero.device != dev:
        raise ValueError("nonzero must be int32 [%d] on %s" % (B, dev))
    if base is not None and (base.dtype != torch.int64 or base.numel() != 1 or base.device != dev):
        raise ValueError("base must be a one-element int64 tensor on %s" % (dev,))
    with torch.cuda.device(dev):
        R.check(R.lib().rpcc_cloud_pack(ptr(pc), ptr(intensity), ptr(ri_rec), B, P, ptr(rows) if rows.numel() else None, rows.shape[0],
                                        ptr(table), ptr(nonzero), ptr(base), ptr(extra) if cap else None, cap,
                                        ptr(extra_count) if cap else None, stream()))
    return table, rows, nonzero

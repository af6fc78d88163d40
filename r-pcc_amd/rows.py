"""The rows of the .bin files a decoded batch is saved as -- the reference's save rule (dataset/dataset.py:72-107, restated in
DatasetTemplate.save_point_cloud_to_file) -- made on the device: a pixel is kept iff (x + y) + z, in fp32 and in that order, is != 0 (NaN
is kept; (1.5, -1.5, 0) is dropped, as the reference does); the kept pixels in raster order become float32 rows (x, y, z, w), bits
unchanged, w the intensity or +0.0.  pack() is the device call (librpcc_rows.so, no CPU fallback); pack_host() is the same rule in numpy
for the frames that go through the per-frame fallback.  DESIGN.md section 22 has the specification."""
import numpy as np


def pack_host(pc, intensity=None):
    """pc f32 [P,3] (or [H,W,3]), intensity f32 [P] or None -> float32 [n,4] rows, the bytes save_point_cloud_to_file writes to a .bin."""
    pc = np.ascontiguousarray(pc, dtype=np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):     # (an overflow to inf, inf - inf: both kept, neither worth a warning)
        keep = (pc[:, 0] + pc[:, 1]) + pc[:, 2] != 0
    rows = np.zeros((int(keep.sum()), 4), np.float32)
    rows.view(np.uint32)[:, :3] = pc.view(np.uint32)[keep]
    if intensity is not None:
        rows.view(np.uint32)[:, 3] = np.ascontiguousarray(intensity, dtype=np.float32).reshape(-1).view(np.uint32)[keep]
    return rows


def pack(pc, intensity=None, ri_rec=None, rows=None, table=None, nonzero=None, base=None):
    """pc: f32 [B,P,3] (or [B,H,W,3]) device tensor; intensity, ri_rec: f32 [B,P] ([B,H,W]) or None.  -> (table, rows, nonzero), queued on
    the current stream, nothing synchronises:
      table i64 [2B+2]: table[:B+1] the offsets -- frame b is rows[table[b]:table[b+1]] --, table[B+1] the status (_rows_lib.OK / E_CAPACITY:
        more rows than `rows` holds, and then nothing of it was written);
      rows f32 [capacity,4]: the caller's, or B*P rows, which always suffice;
      nonzero i32 [B]: the pixels with ri_rec != 0 (None without ri_rec).
    base: a one-element i64 device tensor holding the row the first frame starts at (an earlier call's table[B:B+1]); None: 0.
    Raises RpccError without a GPU."""
    import torch
    from . import _rows_lib as R
    from ._lib import RpccError, ptr, stream
    if not isinstance(pc, torch.Tensor) or not pc.is_cuda:
        raise RpccError("rows.pack runs on librpcc_rows.so and needs a GPU tensor; the HIP path has no CPU fallback (host arrays: rows.pack_host)")
    if pc.dtype != torch.float32 or pc.dim() < 3 or pc.shape[-1] != 3:
        raise ValueError("pc must be float32 [B,P,3] or [B,H,W,3], got %s %s" % (pc.dtype, tuple(pc.shape)))
    B, dev = pc.shape[0], pc.device
    P = pc.numel() // (3 * B) if B else 0
    for name, t in (("intensity", intensity), ("ri_rec", ri_rec)):
        if t is not None and (t.dtype != torch.float32 or t.device != dev or t.shape[0] != B or t.numel() != B * P):
            raise ValueError("%s must be float32 [%d,%d] on %s" % (name, B, P, dev))
    if rows is None:
        rows = torch.empty((B * P, 4), dtype=torch.float32, device=dev)
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
        R.check(R.lib().rpcc_rows_pack(ptr(pc), ptr(intensity), ptr(ri_rec), B, P, ptr(rows) if rows.numel() else None, rows.shape[0],
                                       ptr(table), ptr(nonzero), ptr(base), stream()))
    return table, rows, nonzero

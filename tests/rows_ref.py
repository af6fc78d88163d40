"""The specification of the .bin row packer (librpcc_rows.so, r-pcc_amd/rows.py), stated once: the reference's save rule
(dataset/dataset.py:72-107, restated in DatasetTemplate.save_point_cloud_to_file) for a .bin file.

Inputs for frame b: pc f32 [P,3] in raster order, optionally w f32 [P].
  * pixel p is kept iff s = (x + y) + z is != 0, s computed in fp32, one rounded addition after the other in exactly that order.  NaN is
    kept (it compares unequal); inf - inf is NaN and kept.  numpy's float32 np.sum(..., -1) over three columns is this sequence (checked
    against 200 000 seeded rows plus special values; x + (y + z) differs).  The rule drops real points such as (1.5, -1.5, 0): that is the
    reference's behaviour.
  * the kept pixels in ascending pixel order become rows (x, y, z, w) of four float32, bits unchanged; w is +0.0 without an intensity.
A batch writes its frames back to back: frame b is rows[offsets[b]:offsets[b+1]], offsets[0] = 0; nonzero[b] counts ri_rec != 0."""
import numpy as np


def kept(pc):
    """pc f32 [P,3] -> bool [P], one scalar float32 addition at a time."""
    pc = np.asarray(pc)
    assert pc.dtype == np.float32 and pc.ndim == 2 and pc.shape[1] == 3
    out = np.zeros(pc.shape[0], bool)
    with np.errstate(all="ignore"):
        for p in range(pc.shape[0]):
            s = np.float32(np.float32(pc[p, 0] + pc[p, 1]) + pc[p, 2])
            out[p] = not (s == np.float32(0))
    return out


def kept_fast(pc):
    """The same rule, vectorised (elementwise float32 additions in the same order); test_rows_ref.py holds it to kept()."""
    pc = np.asarray(pc)
    assert pc.dtype == np.float32 and pc.ndim == 2 and pc.shape[1] == 3
    with np.errstate(all="ignore"):
        return np.add(np.add(pc[:, 0], pc[:, 1], dtype=np.float32), pc[:, 2], dtype=np.float32) != 0


def pack(pc, w=None, keep=None):
    """One frame -> float32 [n,4] rows, moved as bit patterns."""
    pc = np.ascontiguousarray(pc)
    keep = kept_fast(pc) if keep is None else keep
    rows = np.zeros((int(keep.sum()), 4), np.uint32)      # +0.0
    rows[:, :3] = pc.view(np.uint32)[keep]
    if w is not None:
        w = np.ascontiguousarray(w)
        assert w.dtype == np.float32 and w.shape == (pc.shape[0],)
        rows[:, 3] = w.view(np.uint32)[keep]
    return rows.view(np.float32)


def pack_batch(pc, w=None, ri_rec=None):
    """pc f32 [B,P,3], w / ri_rec f32 [B,P] or None -> (offsets i64 [B+1], rows f32 [total,4], nonzero i32 [B] or None)."""
    B = pc.shape[0]
    parts = [pack(pc[b], None if w is None else w[b]) for b in range(B)]
    offsets = np.zeros(B + 1, np.int64)
    offsets[1:] = np.cumsum([p.shape[0] for p in parts])
    rows = np.concatenate(parts) if B else np.zeros((0, 4), np.float32)
    nonzero = None if ri_rec is None else np.array([(ri_rec[b] != 0).sum() for b in range(B)], np.int32)
    return offsets, rows, nonzero

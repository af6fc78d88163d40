"""NCLT velodyne_sync records -- the reference's NcltDataset.load_original_utf8_data / convert
(dataset/datasets/nclt_dataset.py:36-63) and the float32 cast of its preprocess_original_utf8_to_bin_file (:31-33) -- as a third point
format beside packed xyz and stored float rows.  A record is 8 bytes, little endian, no header: uint16 x_s, y_s, z_s, uint8 intensity,
uint8 laser; its row is (float32(v_s * 0.005 + -100.0) for x, y, z in fp64, un-fused; the intensity byte as a float).  unpack() is the
device call (librpcc_records.so, no CPU fallback); unpack_host() is the same rule in vectorised numpy for the per-frame front end's
file reader, which is host numpy for every format.  DESIGN.md section 21 has the specification."""
import os

import numpy as np

RECORD_BYTES = 8
SCALING, OFFSET = 0.005, -100.0     # nclt_dataset.py:58-59
POINT_FORMATS = (None, "nclt")      # what the front ends take as point_format / --input_format nclt


def check_point_format(point_format):
    if point_format not in POINT_FORMATS:
        raise ValueError("point_format %r: None (float points) or 'nclt' (8-byte velodyne_sync records)" % (point_format,))
    return point_format


def read_records(path):
    """A velodyne_sync/*.bin file -> uint8 [N,8].  ValueError for a file that holds no whole number of records."""
    nbytes = os.path.getsize(path)
    if nbytes % RECORD_BYTES:
        raise ValueError("%s: %d bytes is no whole number of %d-byte NCLT records" % (path, nbytes, RECORD_BYTES))
    return np.fromfile(path, dtype=np.uint8).reshape(-1, RECORD_BYTES)


def as_records(records):
    """uint8 [N,8] (or flat, a multiple of 8 long) -> contiguous uint8 [N,8]."""
    r = np.asarray(records)
    if r.dtype != np.uint8 or r.size % RECORD_BYTES or (r.ndim == 2 and r.shape[1] != RECORD_BYTES) or r.ndim > 2:
        raise ValueError("records must be uint8 [N,%d] (or flat), got %s %s" % (RECORD_BYTES, r.dtype, r.shape))
    return np.ascontiguousarray(r).reshape(-1, RECORD_BYTES)


def unpack_host(records):
    """uint8 [N,8] records -> float32 [N,4] rows (x, y, z, intensity) by the rule of csrc_records/records_rule.h: numpy's float64 product
    and sum are two rounded operations, astype(float32) the third rounding."""
    r = as_records(records)
    v = r[:, :6].copy().view("<u2").astype(np.float64)          # [N,3]
    rows = np.empty((r.shape[0], 4), np.float32)
    rows[:, :3] = (v * SCALING + OFFSET).astype(np.float32)
    rows[:, 3] = r[:, 6]
    return rows


def unpack(records_dev, out=None):
    """records_dev: a uint8 device tensor, [N,8] or flat -> float32 [N,4] rows on its device, queued on the current stream; nothing
    synchronises.  out: the caller's float32 [N,4] tensor (contiguous, not the records' memory).  Raises RpccError without a GPU."""
    import torch
    from . import _records_lib as R
    from ._lib import RpccError, ptr, stream
    if not isinstance(records_dev, torch.Tensor) or not records_dev.is_cuda:
        raise RpccError("records.unpack runs on librpcc_records.so and needs a GPU tensor; the HIP path has no CPU fallback "
                        "(host arrays: records.unpack_host)")
    if records_dev.dtype != torch.uint8 or records_dev.numel() % RECORD_BYTES or records_dev.dim() > 2 or \
            (records_dev.dim() == 2 and records_dev.shape[1] != RECORD_BYTES):
        raise ValueError("records must be uint8 [N,%d] (or flat), got %s %s" % (RECORD_BYTES, records_dev.dtype, tuple(records_dev.shape)))
    total = records_dev.numel() // RECORD_BYTES
    if out is None:
        out = torch.empty((total, 4), dtype=torch.float32, device=records_dev.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (total, 4) or out.device != records_dev.device:
        raise ValueError("out must be float32 [%d,4] on %s" % (total, records_dev.device))
    with torch.cuda.device(records_dev.device):
        R.check(R.lib().rpcc_records_unpack(ptr(records_dev) if total else None, total, ptr(out) if total else None, stream()))
    return out

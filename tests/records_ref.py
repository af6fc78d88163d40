"""The NCLT record rule (r-pcc_amd/csrc_records/records_rule.h) restated for the tests, twice: in vectorised numpy
(unpack_ref) and as the reference's literal loop -- one struct.unpack per field, `convert` in Python floats, the preprocessing's
append-zeros-and-astype(float32) (dataset/datasets/nclt_dataset.py:31-33,36-63) -- with the record's intensity byte in the fourth
column, where the reference leaves 0 (unpack_loop).  pack_ref makes record inputs from synthetic sweeps and is used for nothing else.
No GPU, no package import."""
import struct

import numpy as np

RECORD_BYTES = 8
SCALING = 0.005
OFFSET = -100.0
EDGE_VALUES = (0, 19999, 20000, 20001, 65535)      # 20000 is the sensor origin: the one value a fused multiply-add gets wrong


def unpack_ref(records):
    """uint8 [N,8] -> float32 [N,4]: (x, y, z by the rule, the intensity byte)."""
    r = np.ascontiguousarray(records, dtype=np.uint8).reshape(-1, RECORD_BYTES)
    v = r[:, :6].copy().view("<u2").astype(np.float64)
    rows = np.zeros((r.shape[0], 4), np.float32)
    rows[:, :3] = (v * SCALING + OFFSET).astype(np.float32)
    rows[:, 3] = r[:, 6].astype(np.float32)
    return rows


def convert(x_s, y_s, z_s):
    """nclt_dataset.py:57-63, in Python floats."""
    scaling = 0.005
    offset = -100.0
    return x_s * scaling + offset, y_s * scaling + offset, z_s * scaling + offset


def unpack_loop(blob):
    """The bytes of a record file -> float32 [N,4], field by field as load_original_utf8_data reads them."""
    pts, inten = [], []
    pos = 0
    while pos < len(blob):
        x = struct.unpack("<H", blob[pos: pos + 2])[0]
        y = struct.unpack("<H", blob[pos + 2: pos + 4])[0]
        z = struct.unpack("<H", blob[pos + 4: pos + 6])[0]
        i = struct.unpack("B", blob[pos + 6: pos + 7])[0]
        struct.unpack("B", blob[pos + 7: pos + 8])      # the laser byte: read and dropped
        pos += RECORD_BYTES
        pts += [list(convert(x, y, z))]
        inten.append(i)
    pc = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    pc = np.append(pc, np.zeros((pc.shape[0], 1)), axis=1)          # preprocess_original_utf8_to_bin_file
    rows = pc.astype(np.float32)
    rows[:, 3] = np.asarray(inten, dtype=np.float32)
    return rows


def fused_model(v_s):
    """What a contracted rule gives: fma(v_s, 0.005, -100) with ONE rounding to fp64, then the cast.  v_s * 0.005 is formed exactly in
    integers (0.005 as a double is m * 2^-60 with a 53-bit m; v_s < 2^16), the sum too, and rounded once by int -> float division."""
    m, e = np.frexp(np.float64(SCALING))
    mant = int(np.ldexp(m, 53))             # SCALING = mant * 2^(e - 53), exactly
    sh = 53 - int(e)
    out = np.empty(len(v_s), np.float32)
    for k, v in enumerate(np.asarray(v_s, dtype=np.int64).tolist()):
        exact = v * mant - (100 << sh)      # the exact value times 2^sh
        out[k] = np.float32(np.float64(exact / (1 << sh)))      # Python's int / int is correctly rounded to a double
    return out


def pack_ref(xyz, intensity=None, laser=None):
    """Test-only inverse: float [N,3] metres (+ intensity bytes, laser bytes) -> uint8 [N,8] records, clip(rint((v + 100) / 0.005), 0, 65535).
    unpack_ref(pack_ref(unpack_ref(r))) == unpack_ref(r) for all 65 536 field values (tests/test_records_ref.py)."""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    n = xyz.shape[0]
    q = np.clip(np.rint((xyz + 100.0) / SCALING), 0, 65535).astype("<u2")
    r = np.zeros((n, RECORD_BYTES), np.uint8)
    r[:, :6] = q.view(np.uint8).reshape(n, 6)
    r[:, 6] = 0 if intensity is None else np.asarray(intensity, dtype=np.uint8)
    r[:, 7] = 0 if laser is None else np.asarray(laser, dtype=np.uint8)
    return r


def field_sweep(field):
    """All 65 536 values in one field (0: x, 1: y, 2: z), the other two fields running through other values, intensities 0 .. 255 and
    every laser byte: uint8 [65536,8]."""
    v = np.arange(65536, dtype=np.int64)
    cols = [(v * 7 + 3) % 65536, (v * 13 + 11) % 65536, (v * 29 + 5) % 65536]
    cols[field] = v
    r = np.zeros((65536, RECORD_BYTES), np.uint8)
    r[:, :6] = np.stack(cols, 1).astype("<u2").view(np.uint8).reshape(65536, 6)
    r[:, 6] = v % 256
    r[:, 7] = (v // 256) % 256
    return r


def synthetic_records(frame_id, H=32, W=2250, vmax_deg=10.67, vmin_deg=-30.67):
    """A synthetic HDL-32E sweep (rpcc_amd.synth) quantised to records: uint8 [N,8], intensities a hash of the point index."""
    from rpcc_amd import synth
    xyz = synth.make_frame(frame_id, H, W, vmax_deg=vmax_deg, vmin_deg=vmin_deg).numpy()
    k = np.arange(xyz.shape[0], dtype=np.int64)
    return pack_ref(xyz, intensity=(k * 37 + frame_id) % 256, laser=k % 32)

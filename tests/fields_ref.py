"""Chunks and descriptors for rpcc_fields_unpack (include/rpcc_fields.h) out of the files of tests/pointfile_cases.py and out of synthetic
record layouts, and the rows they must give, in numpy.  Shared by the host program's test (tests/test_fields_core_host.py) and the device
tests (tests/test_gpu_fields.py).  No GPU."""
import numpy as np

import lzf_ref as Z

DESC_WORDS = 16
NONE, F32, F64, I8, U8, I16, U16, I32, U32 = range(9)
SIZE = (0, 4, 8, 1, 1, 2, 2, 4, 4)
OK, E_LAYOUT = 0, 1
FILL = 0xC3          # what stands between the frames of a chunk


def desc_of(span_off, span_bytes, n, off, step, types):
    d = np.zeros(DESC_WORDS, np.int64)
    d[0], d[1], d[2] = span_off, span_bytes, n
    d[3:7], d[7:11], d[11:15] = off, step, types
    return d


def case_frame(pointfile, case):
    """(body bytes, Layout-made descriptor relative to the body's first byte, expected rows) of one accepted case of the table: a binary file is
    taken whole (its header stands in front of the span), a compressed body decompressed (tests/lzf_ref.py), an ASCII body as the stored
    rows the table expects."""
    name, fmt, data, want = case
    lay = pointfile.read_layout(data, name=name, fmt=fmt)
    if lay.data == "binary":
        return data, lay.desc(lay.data_off), want
    if lay.data == "binary_compressed":
        comp, uncomp = pointfile.compressed_sizes(lay, data)
        st, raw = Z.decode(data[lay.data_off + 8: lay.data_off + 8 + comp], uncomp)
        assert st == Z.OK and len(raw) == uncomp
        return raw, lay.desc(0), want
    return np.ascontiguousarray(want, dtype=np.float32).tobytes(), pointfile.stored_layout(lay.n).desc(0), want


def build_chunk(frames, align=16, lead=0, abut=False):
    """frames: [(bytes, descriptor relative to the bytes, expected rows)] -> (chunk uint8, desc int64 [B,16], row_offsets int64 [B+1], expected
    rows [total,4]).  Every frame starts at a multiple of `align` plus `lead`; abut: byte to byte behind one another instead."""
    parts, desc, pos = [], [], 0
    for data, d, _ in frames:
        start = pos if abut else (pos + align - 1) // align * align + lead
        parts.append(np.full(start - pos, FILL, np.uint8))
        parts.append(np.frombuffer(bytes(data), np.uint8))
        d = d.copy()
        d[0] += start
        desc.append(d)
        pos = start + len(data)
    chunk = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    desc = np.stack(desc) if desc else np.zeros((0, DESC_WORDS), np.int64)
    offs = np.zeros(len(frames) + 1, np.int64)
    offs[1:] = np.cumsum([f[2].shape[0] for f in frames])
    want = np.concatenate([np.asarray(f[2], np.float32).reshape(-1, 4) for f in frames]) if frames else np.zeros((0, 4), np.float32)
    return chunk, desc, offs, want


TYPE_DT = (None, "<f4", "<f8", "i1", "u1", "<i2", "<u2", "<i4", "<u4")


def record_frame(rng, n, step, types=(F32, F32, F32, F32), offs=None, plane=False):
    """A synthetic frame of n points: random values of the given types in records of `step` bytes (the bytes between the fields random too),
    or with plane=True in four planes one behind the other (step = size).  -> (bytes, descriptor, expected rows)."""
    sizes = [SIZE[t] for t in types]
    if plane:
        offs, acc = [], 0
        for s in sizes:
            offs.append(acc)
            acc += n * s + 3          # planes need not be aligned
        steps, nbytes = sizes, acc
    else:
        if offs is None:
            offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist()
        steps = [step] * 4
        nbytes = n * step
    raw = rng.integers(0, 256, max(nbytes, 1), dtype=np.uint8)[:nbytes].copy()
    want = np.zeros((n, 4), np.float32)
    for c, t in enumerate(types):
        if t == NONE or n == 0:
            continue
        if t == F32:
            vals = rng.uniform(-100, 100, n).astype(np.float32)
        elif t == F64:
            vals = rng.uniform(-100, 100, n)
        else:
            info = np.iinfo(np.dtype(TYPE_DT[t]))
            vals = rng.integers(info.min, int(info.max) + 1, n).astype(TYPE_DT[t])
        col = np.ndarray((n,), dtype=np.dtype(TYPE_DT[t]), buffer=raw, offset=offs[c], strides=(steps[c],))
        col[:] = vals
        want[:, c] = vals.astype(np.float32)
    d = desc_of(0, nbytes, n, [o if t != NONE else 0 for o, t in zip(offs, types)], [s if t != NONE else 0 for s, t in zip(steps, types)], types)
    return raw.tobytes(), d, want

"""The .pcd (PCL v0.7) and .ply point files the reference reads through Open3D (dataset/dataset.py:43-63): headers, layouts, the host
reader and a .pcd writer.  Pure Python and numpy, no GPU: this module is the specification, and its row rule is
stated once more for the kernel and the host test program in csrc_fields/fields_rule.h.

A header yields a Layout: data_off (the byte after the `DATA ...` / `end_header` line), n points, and for each of the four columns x, y,
z, w (w = the field or property named exactly `intensity`) the byte `off` of point 0's element relative to data_off, the `step` from one
point's element to the next and a `type` (NONE, F32, F64, I8, U8, I16, U16, I32, U32; little endian).  In `binary` data every step is the
record size; a decompressed `binary_compressed` body is field-major, so off is the start of the field's plane and step its size.

The row rule: F32 -- the four bytes as they are; F64 -- one round-to-nearest-even conversion to fp32 (numpy's astype); integers -- the
value converted to fp32, round-to-nearest-even; NONE -- +0.0.  ASCII values are read as float64 and then follow the F64 rule.  Rows with
non-finite coordinates are kept as stored (the projection skips them), where some Open3D builds drop them on read.

read_rows() is the host reader every per-frame front end uses; unpack() is the device call (librpcc_fields.so, no CPU fallback) the batch
and streaming paths use on the files' bytes as they are."""
import os
import struct

import numpy as np

NONE, F32, F64, I8, U8, I16, U16, I32, U32 = range(9)
TYPE_NAMES = ("NONE", "F32", "F64", "I8", "U8", "I16", "U16", "I32", "U32")
TYPE_SIZE = (0, 4, 8, 1, 1, 2, 2, 4, 4)
_DTYPE = (None, "<u4", "<f8", "i1", "u1", "<i2", "<u2", "<i4", "<u4")      # (F32 is moved as its bits)
COLUMNS = ("x", "y", "z", "intensity")
DESC_WORDS = 16         # RPCC_FIELDS_DESC_WORDS
MAX_STEP = 256          # RPCC_FIELDS_MAX_STEP
EXTENSIONS = ("pcd", "ply")
HEADER_LIMIT = 1 << 16  # bytes a header may take

_PCD_TYPE = {("F", 4): F32, ("F", 8): F64, ("I", 1): I8, ("U", 1): U8, ("I", 2): I16, ("U", 2): U16, ("I", 4): I32, ("U", 4): U32}
_PLY_TYPE = {"char": I8, "int8": I8, "uchar": U8, "uint8": U8, "short": I16, "int16": I16, "ushort": U16, "uint16": U16,
             "int": I32, "int32": I32, "uint": U32, "uint32": U32, "float": F32, "float32": F32, "double": F64, "float64": F64}

LZF_STATUS = {1: "the LZF stream ends inside a literal run or a match", 2: "an LZF match starts before the first output byte",
              3: "the LZF stream decodes past the stated uncompressed size"}


def is_point_file(name):
    """Whether the file's extension (the reference's rule: the text after the last dot) is one this module reads."""
    return str(name).split(".")[-1] in EXTENSIONS


class Layout:
    """What a header says about its body.  data: "binary" (records), "binary_compressed" (an LZF stream of planes; off / step describe the
    DECOMPRESSED body) or "ascii" (tokens: token_of[c] is the column's token inside a point's tokens, tokens their number; off / step /
    type then describe the stored rows the parsed values are put into).  body_bytes: what the layout needs behind data_off (binary: n
    records; binary_compressed: the decompressed size; ascii: 0, its length is not known from the header)."""

    def __init__(self, name, fmt, data, data_off, n, off, step, types, body_bytes, record=0, token_of=None, tokens=0):
        self.name, self.fmt, self.data, self.data_off, self.n = name, fmt, data, int(data_off), int(n)
        self.off, self.step, self.type = [int(v) for v in off], [int(v) for v in step], [int(v) for v in types]
        self.body_bytes, self.record = int(body_bytes), int(record)
        self.token_of, self.tokens = token_of, int(tokens)

    @property
    def has_intensity(self):
        return self.type[3] != NONE if self.data != "ascii" else self.token_of[3] >= 0

    @property
    def max_step(self):
        return max([s for s, t in zip(self.step, self.type) if t != NONE] or [0])

    def desc(self, span_off, span_bytes=None):
        """The kernel's descriptor (include/rpcc_fields.h) of this layout's body standing at byte span_off of a chunk."""
        d = np.zeros(DESC_WORDS, np.int64)
        d[0], d[1], d[2] = span_off, self.body_bytes if span_bytes is None else span_bytes, self.n
        d[3:7], d[7:11], d[11:15] = self.off, self.step, self.type
        return d


def stored_layout(n, name="rows"):
    """The layout of n stored rows: four F32 at 0 / 4 / 8 / 12, step 16."""
    return Layout(name, "rows", "binary", 0, n, (0, 4, 8, 12), (16,) * 4, (F32,) * 4, 16 * int(n), record=16)


def _refuse(name, why):
    raise ValueError("%s: %s" % (name, why))


def _lines(buf, name, last):
    """The header's lines up to and including the one `last(words)` accepts -> ([words], data_off)."""
    out, pos = [], 0
    buf = bytes(buf[:HEADER_LIMIT])
    limit = len(buf)
    while pos < limit:
        end = buf.find(b"\n", pos, limit)
        if end < 0:
            break
        try:
            text = bytes(buf[pos:end]).decode("ascii").strip()
        except UnicodeDecodeError:
            _refuse(name, "the header is not ASCII text")
        pos = end + 1
        words = text.split()
        if not words:
            continue
        out.append(words)
        if last(words):
            return out, pos
    _refuse(name, "the header does not end (no DATA / end_header line in the first %d bytes)" % limit)


def _ints(name, key, words, count=None):
    try:
        vals = [int(w) for w in words]
    except ValueError:
        _refuse(name, "%s holds %r, not integers" % (key, " ".join(words)))
    if count is not None and len(vals) != count:
        _refuse(name, "%s holds %d values, FIELDS names %d" % (key, len(vals), count))
    if any(v < 0 for v in vals):
        _refuse(name, "%s holds a negative value" % key)
    return vals


def _parse_pcd(buf, name, file_bytes):
    lines, data_off = _lines(buf, name, lambda w: w[0] == "DATA")
    h = {}
    for w in lines:
        if w[0].startswith("#"):
            continue
        h.setdefault(w[0], w[1:])
    for key in ("FIELDS", "SIZE", "TYPE", "WIDTH", "HEIGHT"):
        if key not in h:
            _refuse(name, "the header has no %s line" % key)
    fields = h["FIELDS"]
    size = _ints(name, "SIZE", h["SIZE"], len(fields))
    kind = h["TYPE"]
    if len(kind) != len(fields):
        _refuse(name, "TYPE holds %d values, FIELDS names %d" % (len(kind), len(fields)))
    count = _ints(name, "COUNT", h["COUNT"], len(fields)) if "COUNT" in h else [1] * len(fields)
    width, height = _ints(name, "WIDTH", h["WIDTH"], 1)[0], _ints(name, "HEIGHT", h["HEIGHT"], 1)[0]
    n = _ints(name, "POINTS", h["POINTS"], 1)[0] if "POINTS" in h else width * height
    if n != width * height:
        _refuse(name, "POINTS %d is not WIDTH * HEIGHT = %d * %d" % (n, width, height))
    data = h["DATA"][0] if h["DATA"] else ""
    if data not in ("ascii", "binary", "binary_compressed"):
        _refuse(name, "unknown DATA %r (ascii, binary or binary_compressed)" % data)
    starts = np.concatenate([[0], np.cumsum([s * c for s, c in zip(size, count)])]).astype(np.int64)
    tok_starts = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
    record, tokens = int(starts[-1]), int(tok_starts[-1])
    off, step, types, token_of = [0] * 4, [0] * 4, [NONE] * 4, [-1] * 4
    for c, col in enumerate(COLUMNS):
        if col not in fields:
            if c < 3:
                _refuse(name, "no field %s (FIELDS %s)" % (col, " ".join(fields)))
            continue
        f = fields.index(col)
        if count[f] != 1:
            _refuse(name, "field %s has COUNT %d, not 1" % (col, count[f]))
        t = _PCD_TYPE.get((kind[f], size[f]))
        if t is None:
            _refuse(name, "field %s has SIZE %d TYPE %s: F 4, F 8, I / U 1, 2 or 4 are read" % (col, size[f], kind[f]))
        types[c], token_of[c] = t, int(tok_starts[f])
        if data == "binary":
            off[c], step[c] = int(starts[f]), record
        else:                       # binary_compressed: the field's plane
            off[c], step[c] = n * int(starts[f]), size[f]
    body = file_bytes - data_off
    if data == "binary":
        if body < n * record:
            _refuse(name, "the body holds %d bytes, %d points of %d bytes need %d" % (body, n, record, n * record))
        return Layout(name, "pcd", data, data_off, n, off, step, types, n * record, record=record)
    if data == "binary_compressed":
        if body < 8:
            _refuse(name, "the body holds %d bytes, a compressed body begins with two 32-bit sizes" % body)
        return Layout(name, "pcd", data, data_off, n, off, step, types, n * record, record=record)
    st = stored_layout(n)
    return Layout(name, "pcd", "ascii", data_off, n, st.off, st.step, st.type, 0, record=record, token_of=token_of, tokens=tokens)


def _parse_ply(buf, name, file_bytes):
    lines, data_off = _lines(buf, name, lambda w: w == ["end_header"])
    if lines[0] != ["ply"]:
        _refuse(name, "not a PLY file (first line %r)" % " ".join(lines[0]))
    fmt, element, props, n = None, None, [], None
    for w in lines[1:-1]:
        if w[0] in ("comment", "obj_info"):
            continue
        if w[0] == "format":
            if len(w) != 3 or w[1] not in ("ascii", "binary_little_endian") or w[2] != "1.0":
                _refuse(name, "format %s: ascii 1.0 or binary_little_endian 1.0 are read%s"
                        % (" ".join(w[1:]), " (binary_big_endian is not)" if len(w) > 1 and w[1] == "binary_big_endian" else ""))
            fmt = w[1]
        elif w[0] == "element":
            if len(w) != 3:
                _refuse(name, "element line %r" % " ".join(w))
            if element is None:
                if w[1] != "vertex":
                    _refuse(name, "element %s stands before element vertex: vertex must be the first element" % w[1])
                n = _ints(name, "element vertex", w[2:], 1)[0]
            element = w[1] if element is None else "later"
        elif w[0] == "property":
            if element is None:
                _refuse(name, "a property line stands before the first element")
            if element != "vertex":
                continue
            if len(w) >= 2 and w[1] == "list":
                _refuse(name, "a list property in element vertex")
            if len(w) != 3 or w[1] not in _PLY_TYPE:
                _refuse(name, "property line %r: an unknown scalar type" % " ".join(w))
            props.append((w[2], _PLY_TYPE[w[1]]))
        else:
            _refuse(name, "header line %r" % " ".join(w))
    if fmt is None:
        _refuse(name, "the header has no format line")
    if n is None:
        _refuse(name, "the header has no element vertex")
    names = [p[0] for p in props]
    starts = np.concatenate([[0], np.cumsum([TYPE_SIZE[p[1]] for p in props])]).astype(np.int64)
    record = int(starts[-1])
    off, step, types, token_of = [0] * 4, [0] * 4, [NONE] * 4, [-1] * 4
    for c, col in enumerate(COLUMNS):
        if col not in names:
            if c < 3:
                _refuse(name, "no property %s in element vertex (%s)" % (col, " ".join(names)))
            continue
        f = names.index(col)
        off[c], step[c], types[c], token_of[c] = int(starts[f]), record, props[f][1], f
    if fmt == "ascii":
        st = stored_layout(n)
        return Layout(name, "ply", "ascii", data_off, n, st.off, st.step, st.type, 0, record=record, token_of=token_of, tokens=len(props))
    body = file_bytes - data_off
    if body < n * record:
        _refuse(name, "the body holds %d bytes, %d vertices of %d bytes need %d" % (body, n, record, n * record))
    return Layout(name, "ply", "binary", data_off, n, off, step, types, n * record, record=record)


def read_layout(path_or_bytes, name=None, fmt=None, file_bytes=None):
    """The Layout of a .pcd / .ply file: a path (only the header is read; the format by the extension), or the file's bytes (name: what
    errors call it; fmt: "pcd" / "ply", else by name's extension, else by the first bytes).  file_bytes: the file's length when only its
    head is given.  ValueError naming the file and the reason for a header this module does not read."""
    if isinstance(path_or_bytes, (str, os.PathLike)):
        name = str(path_or_bytes) if name is None else name
        file_bytes = os.path.getsize(path_or_bytes)
        with open(path_or_bytes, "rb") as f:
            buf = f.read(HEADER_LIMIT)
    else:
        buf = path_or_bytes
        name = "<bytes>" if name is None else name
        file_bytes = len(buf) if file_bytes is None else file_bytes
    if fmt is None:
        ext = name.split(".")[-1]
        fmt = ext if ext in EXTENSIONS else ("ply" if bytes(buf[:3]) == b"ply" else "pcd")
    return (_parse_ply if fmt == "ply" else _parse_pcd)(buf, name, file_bytes)


def lzf_decompress(src, dst, name="<bytes>"):
    """src (bytes-like) -> dst (a writable uint8 numpy array of exactly the stated uncompressed size) through librpcc_host.so's
    rpcc_lzf_decompress.  ValueError for every status of the decoder and for a stream that ends short of dst."""
    import ctypes as C
    from . import _lib
    src = np.frombuffer(src, dtype=np.uint8)
    assert dst.dtype == np.uint8 and dst.flags.c_contiguous and dst.flags.writeable
    got = C.c_size_t(0)
    rc = _lib.host_lib().rpcc_lzf_decompress(src.ctypes.data if src.size else None, src.size, dst.ctypes.data if dst.size else None, dst.size,
                                             C.byref(got))
    if rc != 0:
        _refuse(name, LZF_STATUS.get(rc, "LZF decoder status %d" % rc))
    if got.value != dst.size:
        _refuse(name, "the LZF stream decodes to %d bytes, the header states %d" % (got.value, dst.size))
    return dst


def compressed_sizes(layout, buf):
    """(compressed_size, uncompressed_size) of a binary_compressed body, checked against the layout and the file's length."""
    comp, uncomp = struct.unpack_from("<II", buf, layout.data_off)
    if uncomp != layout.body_bytes:
        _refuse(layout.name, "uncompressed_size %d is not %d points of %d bytes = %d" % (uncomp, layout.n, layout.record, layout.body_bytes))
    if len(buf) - layout.data_off - 8 < comp:
        _refuse(layout.name, "the body holds %d bytes, compressed_size states %d" % (len(buf) - layout.data_off - 8, comp))
    return comp, uncomp


def ascii_rows(layout, buf):
    """The stored rows of an ASCII body: the first n * tokens values as float64, the columns' tokens through the F64 rule."""
    toks = bytes(buf[layout.data_off:]).split(None, layout.n * layout.tokens)[: layout.n * layout.tokens]
    if len(toks) < layout.n * layout.tokens:
        _refuse(layout.name, "the body holds %d values, %d points of %d need %d" % (len(toks), layout.n, layout.tokens, layout.n * layout.tokens))
    rows = np.zeros((layout.n, 4), np.float32)
    if layout.n:
        table = np.array(toks, dtype="S").reshape(layout.n, layout.tokens)
        for c in range(4):
            if layout.token_of[c] >= 0:
                try:
                    vals = table[:, layout.token_of[c]].astype(np.float64)
                except ValueError:
                    _refuse(layout.name, "the body holds a value of %s that is no number" % COLUMNS[c])
                with np.errstate(over="ignore"):
                    rows[:, c] = vals.astype(np.float32)
    return rows


def rows_of(layout, body):
    """The row rule in numpy: body (bytes-like; the layout's offsets are relative to its first byte) -> float32 [n,4]."""
    rows = np.zeros((layout.n, 4), np.float32)
    if layout.n == 0:
        return rows
    body = np.frombuffer(body, dtype=np.uint8)
    bits = rows.view(np.uint32)
    for c in range(4):
        t = layout.type[c]
        if t == NONE:
            continue
        col = np.ndarray((layout.n,), dtype=_DTYPE[t], buffer=body, offset=layout.off[c], strides=(layout.step[c],))
        if t == F32:
            bits[:, c] = col
        else:
            with np.errstate(over="ignore"):
                rows[:, c] = col.astype(np.float32)
    return rows


def read_rows(path_or_bytes, name=None, fmt=None):
    """A .pcd / .ply file (path, or its bytes) -> float32 [n,4] rows (x, y, z, intensity; +0.0 where the file has no intensity)."""
    if isinstance(path_or_bytes, (str, os.PathLike)):
        name = str(path_or_bytes) if name is None else name
        with open(path_or_bytes, "rb") as f:
            buf = f.read()
    else:
        buf = path_or_bytes
    layout = read_layout(buf, name=name, fmt=fmt)
    if layout.data == "ascii":
        return ascii_rows(layout, buf)
    view = memoryview(buf)
    if layout.data == "binary_compressed":
        comp, uncomp = compressed_sizes(layout, buf)
        body = np.empty(uncomp, np.uint8)
        lzf_decompress(view[layout.data_off + 8: layout.data_off + 8 + comp], body, layout.name)
        return rows_of(layout, body)
    return rows_of(layout, view[layout.data_off: layout.data_off + layout.body_bytes])


def pcd_header(n, intensity):
    """The header write_pcd writes."""
    k = 4 if intensity else 3
    return ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z%s\nSIZE%s\nTYPE%s\nCOUNT%s\nWIDTH %d\nHEIGHT 1\n"
            "VIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA binary\n" % (" intensity" if intensity else "", " 4" * k, " F" * k, " 1" * k, n, n)).encode()


def write_pcd(path, xyz, intensity=None):
    """xyz [n,>=3] (and intensity [n]) -> a .pcd file: DATA binary, FIELDS x y z [intensity], float32, HEIGHT 1."""
    xyz = np.asarray(xyz)
    body = np.ascontiguousarray(xyz[:, :3], dtype="<f4")
    if intensity is not None:
        w = np.asarray(intensity).reshape(-1)
        if w.shape[0] != body.shape[0]:
            raise ValueError("write_pcd: %d intensities for %d points" % (w.shape[0], body.shape[0]))
        body = np.ascontiguousarray(np.concatenate([body, w.astype("<f4")[:, None]], 1))
    with open(path, "wb") as f:
        f.write(pcd_header(body.shape[0], intensity is not None))
        f.write(body.tobytes())


def unpack_into(chunk_dev, desc_dev, offs_dev, total, rows, status):
    """rpcc_fields_unpack on the caller's device tensors, queued on the current stream: chunk_dev uint8 [nbytes], desc_dev int64 [B,16],
    offs_dev int64 [B+1] (offs_dev[B] == total), rows float32 [>=total,4], status int32 [B].  Nothing is allocated or copied."""
    import torch
    from . import _fields_lib as F
    from ._lib import ptr, stream
    B = int(desc_dev.shape[0])
    assert chunk_dev.dtype == torch.uint8 and desc_dev.dtype == torch.int64 and tuple(desc_dev.shape) == (B, DESC_WORDS)
    assert offs_dev.dtype == torch.int64 and offs_dev.numel() == B + 1 and status.dtype == torch.int32 and status.numel() == B
    assert rows.dtype == torch.float32 and rows.dim() == 2 and rows.shape[1] == 4 and rows.shape[0] >= total
    with torch.cuda.device(chunk_dev.device):
        F.check(F.lib().rpcc_fields_unpack(ptr(chunk_dev) if chunk_dev.numel() else None, chunk_dev.numel(), ptr(desc_dev) if B else None, B,
                                           ptr(offs_dev), int(total), ptr(rows) if total else None, ptr(status) if B else None, stream()))


def unpack(chunk_dev, layouts, out=None):
    """The Python face of rpcc_fields_unpack.  chunk_dev: a uint8 device tensor, the files' bytes (its storage 16-byte aligned);
    layouts: one descriptor per frame -- Layout.desc(span_off) arrays, or an int64 [B,16] array.  -> (rows f32 [total,4], row_offsets
    i64 [B+1], status i32 [B]) on the chunk's device, queued on the current stream; nothing synchronises.  out: the caller's float32
    [>=total,4] tensor, whose first total rows are written.  Raises RpccError without a GPU."""
    import torch
    from ._lib import RpccError
    if not isinstance(chunk_dev, torch.Tensor) or not chunk_dev.is_cuda:
        raise RpccError("pointfile.unpack runs on librpcc_fields.so and needs a GPU tensor; the HIP path has no CPU fallback "
                        "(host arrays: pointfile.read_rows)")
    if chunk_dev.dtype != torch.uint8 or chunk_dev.dim() != 1:
        raise ValueError("the chunk must be a flat uint8 tensor, got %s %s" % (chunk_dev.dtype, tuple(chunk_dev.shape)))
    desc = np.ascontiguousarray(np.asarray(layouts if len(layouts) else np.zeros((0, DESC_WORDS)), dtype=np.int64).reshape(-1, DESC_WORDS))
    B = desc.shape[0]
    offs = np.zeros(B + 1, np.int64)
    offs[1:] = np.cumsum(np.clip(desc[:, 2], 0, None))
    total = int(offs[B])
    dev = chunk_dev.device
    if out is None:
        out = torch.empty((total, 4), dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or out.dim() != 2 or out.shape[1] != 4 or out.shape[0] < total or out.device != dev:
        raise ValueError("out must be float32 [>=%d,4] on %s" % (total, dev))
    desc_dev = torch.from_numpy(desc).to(dev)
    offs_dev = torch.from_numpy(offs).to(dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    unpack_into(chunk_dev, desc_dev, offs_dev, total, out, status)
    return out[:total], offs_dev, status

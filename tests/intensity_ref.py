"""The specification of the intensity channel, stated once: which point owns a pixel, the 8-bit quantiser, the payload and its refusals.
The kernels (r-pcc_amd/csrc/intensity_kernels.h) and the product code follow this file; it is test infrastructure and never imported by
the package.

Owner of a pixel.  One frame, rows i = 0 .. N-1 in input order:
  d_i = sqrtf(x*x + y*y + z*z) in fp32, un-fused; a row whose d_i is not finite is skipped, as rpcc_project skips it
  pix_i = the reference's pixel (cpp_modules.cpp:446-458), taken from oracle/liborpcc.so: orc_project_rowcol
  the reference's loop `if (ri[pix] == 0 || d < ri[pix]) ri[pix] = d` gains one statement: own[pix] = i
  a pixel is non-empty iff its final ri != 0; its owner is the final own                                   (owners_loop)
In closed form (owners_closed): z(pix) = the last i with pix_i == pix and d_i == 0, or -1; the owner is the smallest i > z(pix) with
pix_i == pix and the bits of d_i equal to the bits of ri[pix].

Quantiser.  scale: fp32, finite, > 0.  t = w * scale (one fp32 multiply); r = rintf(t) (half to even); q = 0 unless r >= 0 (NaN,
negatives); q = 255 if r > 255 (+inf); else (uint8)r.  Dequantiser: w' = (float)q / scale, one correctly rounded fp32 division.

Payload 'intensity': uint8 [8 + n] = b"RPI1" | scale as little-endian float32 | q of the non-empty pixels in ascending pixel index;
n = pixels with ri != 0 = pixels whose label is not 1."""
import ctypes as C
import struct

import numpy as np

from oracle import oracle as orc

MAGIC = b"RPI1"


def pixels(xyz, g):
    """-> (d f32 [N], pix i64 [N]; -1 for a row that is skipped)."""
    L = orc.lib()
    fn = L.orc_project_rowcol
    fn.restype = None
    fn.argtypes = [C.c_float] * 3 + [C.c_int] * 2 + [C.c_float] * 3 + [C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    with np.errstate(all="ignore"):
        d = np.sqrt(x * x + y * y + z * z)          # fp32 products, fp32 sums, correctly rounded root
    pix = np.full(xyz.shape[0], -1, np.int64)
    dd, r, c = C.c_float(), C.c_int(), C.c_int()
    hf, vmax, vmin = float(g.horizontal_FOV), float(g.vertical_max), float(g.vertical_min)
    for i in np.flatnonzero(np.isfinite(d)):
        fn(float(x[i]), float(y[i]), float(z[i]), g.H, g.W, hf, vmax, vmin, C.byref(dd), C.byref(r), C.byref(c))
        assert np.float32(dd.value).view(np.uint32) == d[i].view(np.uint32)
        pix[i] = r.value * g.W + c.value
    return d, pix


def owners_loop(d, pix, P):
    """The reference's loop with `own[pix] = i` added -> (ri f32 [P], own i64 [P]; -1 where the pixel is empty)."""
    ri, own = np.zeros(P, np.float32), np.full(P, -1, np.int64)
    for i in np.flatnonzero(pix >= 0):
        p = pix[i]
        if ri[p] == 0 or d[i] < ri[p]:
            ri[p] = d[i]
            own[p] = i
    own[ri == 0] = -1
    return ri, own


def owners_closed(d, pix, ri):
    """The closed form the kernel computes, given the final ri."""
    P = ri.shape[0]
    ok = pix >= 0
    idx = np.arange(pix.shape[0], dtype=np.int64)
    z = np.full(P, -1, np.int64)
    zero = ok & (d == 0)
    np.maximum.at(z, pix[zero], idx[zero])
    cand = ok & ~zero
    cand[cand] = (idx[cand] > z[pix[cand]]) & (d[cand].view(np.uint32) == ri[pix[cand]].view(np.uint32))
    own = np.full(P, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(own, pix[cand], idx[cand])
    own[own == np.iinfo(np.int64).max] = -1
    own[ri == 0] = -1
    return own


def quantise(w, scale):
    w, scale = np.asarray(w, dtype=np.float32), np.float32(scale)
    with np.errstate(all="ignore"):
        r = np.rint(w * scale)                      # fp32 multiply, half to even
        q = np.where(r >= 0, np.where(r > 255, np.float32(255), r), np.float32(0))
    return q.astype(np.uint8)


def dequantise(q, scale):
    return np.asarray(q, dtype=np.uint8).astype(np.float32) / np.float32(scale)


def encode_frame(rows, g, scale):
    """rows f32 [N,4] -> dict(ri [P], own [P], payload uint8 [8+n], image uint8 [P], q uint8 [n])."""
    rows = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, 4)
    P = g.H * g.W
    d, pix = pixels(rows[:, :3], g)
    ri, own = owners_loop(d, pix, P)
    set_ = ri != 0
    q = quantise(rows[own[set_], 3], scale)
    image = np.zeros(P, np.uint8)
    image[set_] = q
    payload = np.frombuffer(MAGIC + struct.pack("<f", np.float32(scale)) + q.tobytes(), dtype=np.uint8)
    return dict(ri=ri, own=own, d=d, pix=pix, payload=payload, image=image, q=q)


def encode_frames(frames, g, scale):
    """encode_frame of every frame of a batch -> a list of its dicts, computed once per distinct array (a batch that repeats a frame holds
    the same array again: the specification is per frame, so the same dict stands at every one of its places)."""
    memo = {}
    out = []
    for f in frames:
        key = (f.__array_interface__["data"][0], f.shape, f.strides)
        if key not in memo:
            memo[key] = encode_frame(f, g, scale)
        out.append(memo[key])
    return out


def parse_payload(data, n):
    """-> (scale f32, q uint8 [n]); ValueError for each of the refusals."""
    data = bytes(data)
    if len(data) < 8 or data[:4] != MAGIC:
        raise ValueError("no magic")
    scale = np.frombuffer(data, "<f4", 1, 4)[0]
    if not (np.isfinite(scale) and scale > 0):
        raise ValueError("bad scale")
    if len(data) != 8 + n:
        raise ValueError("%d bytes for %d pixels" % (len(data), n))
    return scale, np.frombuffer(data, np.uint8, offset=8)


def decode_frame(payload, labels):
    """labels [P] (1 = empty pixel) -> f32 [P], 0 where the label is 1; ValueError when the payload is refused."""
    labels = np.asarray(labels).reshape(-1)
    set_ = labels != 1
    scale, q = parse_payload(payload, int(set_.sum()))
    out = np.zeros(labels.shape[0], np.float32)
    out[set_] = dequantise(q, scale)
    return out

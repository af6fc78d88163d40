"""The specification of the hidden_points channel, stated once: which points share a pixel with its owner, their range and lateral codes,
the order, the per-pixel cap, the payload and its refusals, and the decoder's arithmetic.  The kernels (r-pcc_amd/csrc/hidden_kernels.h)
and the product code follow this file; it is test infrastructure and never imported by the package.

Per frame, evenly spaced beams only; ri is the range image of the frame's rows, step the fp32 quantiser step (accuracy * 2).

Skipped.  A row whose depth d = sqrtf(x*x + y*y + z*z) (fp32, un-fused) is NaN, infinite or 0, as the projection skips it.
Owner.  The intensity channel's (intensity_ref.owners_loop).
Hidden points.  Every other row whose pixel is non-empty: also a row of equal depth bits that comes later in the input, and a row in
front of a later depth-0 row of its pixel (it may be nearer than the owner).  Rows in empty pixels (ri == 0 there) are not carried.
Range code.  k = rintf(d / step): one IEEE fp32 division, half to even.  A point with !(k <= 65535) is not carried; k = 0 is a code like
any other.  The decoded range is (float)k * step, one fp32 multiply: |r - d| <= step * (0.5 + k * 2^-23).
Lateral codes.  bits 0 .. 4.  bits > 0: subpixel_ref.code of the point's own off_az / off_el (subpixel_ref.offsets) against its pixel; else 0.
Order.  key = k << 8 | az << 4 | el; by pixel in raster order, then by key ascending (equal keys are interchangeable).
Cap.  At most the 255 smallest keys of a pixel are carried.
Uncarried.  Hidden points in an empty pixel, with k past 65535, or past the cap, counted per frame.

Payload 'hidden_points': uint8 = b"RPH1" | bits | 0 0 0 | step as little-endian f32 | m as little-endian u32 | count plane [n]: carried
hidden points of every non-empty pixel in raster order | range codes: little-endian u16 [m] | for bits > 0: az codes [m] | el codes [m].
16 + n + 2m bytes, or 16 + n + 4m.

Decoder.  Per pixel in payload order, c points: bits 0: r * tm[pixel], the fp32 multiply of the back-projection; bits > 0: the pixel's
ray turned by the two offsets through the fp64 angle sums of subpixel_ref.decode_frame over subpixel_ref.tables.

Refusals (nothing of the frame is written): fewer than 16 bytes; no magic; bits above 4; a reserved byte that is not 0; a step that is
not finite and > 0; n other than the count of labels != 1; another byte count than the formula; counts that do not sum to m; m above
the caller's capacity; an az / el code >= 2^bits; no tables when bits > 0."""
import struct

import numpy as np

import intensity_ref as IR
import subpixel_ref as SR

MAGIC = b"RPH1"
HEADER = 16
CAP = 255


def range_code(d, step):
    """-> (k f32 (rintf(d / step)), carried bool)."""
    with np.errstate(all="ignore"):
        k = np.rint(np.asarray(d, dtype=np.float32) / np.float32(step))
    assert k.dtype == np.float32
    return k, k <= 65535


def decoded_range(k, step):
    r = np.asarray(k, dtype=np.uint16).astype(np.float32) * np.float32(step)
    assert r.dtype == np.float32
    return r


def payload(bits, step, counts, k, az, el):
    k = np.asarray(k, dtype="<u2")
    head = MAGIC + bytes([bits, 0, 0, 0]) + struct.pack("<f", np.float32(step)) + struct.pack("<I", k.shape[0])
    body = np.asarray(counts, np.uint8).tobytes() + k.tobytes()
    if bits > 0:
        body += np.asarray(az, np.uint8).tobytes() + np.asarray(el, np.uint8).tobytes()
    return np.frombuffer(head + body, dtype=np.uint8)


def encode_frame(rows, g, step, bits, owners=None):
    """rows f32 [N,>=3] -> dict(ri [P], own [P], d, pix, hidden bool [N] (every hidden point), carried i64 [m] (row indices in payload
    order, up to the order of equal keys), pixel i64 [m], k u16 [m], az / el u8 [m], counts u8 [n], uncarried int, n, m, payload).
    owners: (d, pix, ri, own) of these rows where they are already known."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    xyz = np.ascontiguousarray(rows[:, :3])
    N, P = xyz.shape[0], g.H * g.W
    if owners is None:
        d, pix = IR.pixels(xyz, g)
        ri, own = IR.owners_loop(d, pix, P)
        assert np.array_equal(own, IR.owners_closed(d, pix, ri))
    else:
        d, pix, ri, own = owners
    valid = (pix >= 0) & (d != 0)                               # pix < 0: a depth that is not finite
    is_owner = np.zeros(N, bool)
    is_owner[own[own >= 0]] = True
    hidden = valid & ~is_owner
    lit = np.zeros(N, bool)
    lit[valid] = ri[pix[valid]] != 0
    kf, fits = range_code(d, step)
    cand = np.flatnonzero(hidden & lit & fits)
    uncarried = int(hidden.sum()) - cand.shape[0]               # empty pixels and k past 65535; the cap adds below
    k = kf[cand].astype(np.uint32)
    if bits > 0 and cand.shape[0]:
        row, col, off_az, off_el, _ = SR.offsets(xyz[cand], g)
        assert np.array_equal(row * g.W + col, pix[cand])      # orc_project_rowcol's pixel
        az, el = SR.code(off_az, bits).astype(np.uint32), SR.code(off_el, bits).astype(np.uint32)
    else:
        az = el = np.zeros(cand.shape[0], np.uint32)
    key = k << 8 | az << 4 | el
    order = np.lexsort((cand, key, pix[cand]))                  # pixel, then key (then input order: equal keys are interchangeable)
    cand, key, px = cand[order], key[order], pix[cand][order]
    first = np.searchsorted(px, px, side="left")                # start of the pixel's run
    keep = np.arange(px.shape[0]) - first < CAP
    uncarried += int((~keep).sum())
    cand, key, px = cand[keep], key[keep], px[keep]
    set_ = np.flatnonzero(ri != 0)
    counts = np.bincount(px, minlength=P)[set_]
    assert counts.max(initial=0) <= CAP and counts.sum() == cand.shape[0]
    k16, az8, el8 = (key >> 8).astype(np.uint16), (key >> 4 & 15).astype(np.uint8), (key & 15).astype(np.uint8)
    return dict(ri=ri, own=own, d=d, pix=pix, hidden=hidden, carried=cand, pixel=px, key=key, k=k16, az=az8, el=el8, counts=counts.astype(np.uint8),
                uncarried=uncarried, n=set_.shape[0], m=cand.shape[0], payload=payload(bits, step, counts, k16, az8, el8))


def encode_frames(frames, g, step, bits, memo=None):
    """encode_frame of every frame of a batch; the owner pass once per distinct array (memo: a dict shared between calls with other steps / bits)."""
    memo = {} if memo is None else memo
    out = []
    for f in frames:
        key = (f.__array_interface__["data"][0], f.shape, f.strides)
        full = key + (float(np.float32(step)), bits)
        if full not in memo:
            e = encode_frame(f, g, step, bits, owners=memo.get(key))
            memo[key] = (e["d"], e["pix"], e["ri"], e["own"])
            memo[full] = e
        out.append(memo[full])
    return out


def parse_payload(data, n, capacity=None):
    """-> (bits, step f32, counts u8 [n], k u16 [m], az u8 [m], el u8 [m]); ValueError for each of the refusals."""
    data = bytes(data)
    if len(data) < HEADER:
        raise ValueError("%d bytes hold no header" % len(data))
    if data[:4] != MAGIC:
        raise ValueError("no magic")
    bits = data[4]
    if bits > 4:
        raise ValueError("bits %d" % bits)
    if data[5:8] != b"\0\0\0":
        raise ValueError("reserved bytes")
    step = np.frombuffer(data, "<f4", 1, 8)[0]
    if not (np.isfinite(step) and step > 0):
        raise ValueError("bad step")
    m = struct.unpack_from("<I", data, 12)[0]
    if len(data) != HEADER + n + (4 if bits else 2) * m:
        raise ValueError("%d bytes for %d pixels and %d points at %d bits" % (len(data), n, m, bits))
    counts = np.frombuffer(data, np.uint8, n, HEADER)
    if int(counts.sum(dtype=np.int64)) != m:
        raise ValueError("the counts sum to %d, not %d" % (counts.sum(dtype=np.int64), m))
    if capacity is not None and m > capacity:
        raise ValueError("%d points, room for %d" % (m, capacity))
    k = np.frombuffer(data, "<u2", m, HEADER + n)
    if bits:
        lat = np.frombuffer(data, np.uint8, 2 * m, HEADER + n + 2 * m)
        if lat.size and lat.max() >= 1 << bits:
            raise ValueError("code %d at %d bits" % (lat.max(), bits))
        az, el = lat[:m], lat[m:]
    else:
        az = el = np.zeros(m, np.uint8)
    return bits, step, counts, k, az, el


def decode_frame(data, labels, g, tm, tab=None, capacity=None):
    """labels [P] (1 = empty pixel), tm f32 [P,3] -> f32 [m,3] in payload order; ValueError when the payload is refused."""
    labels = np.asarray(labels).reshape(-1)
    set_ = np.flatnonzero(labels != 1)
    bits, step, counts, k, az, el = parse_payload(data, set_.shape[0], capacity)
    p = np.repeat(set_, counts)
    r = decoded_range(k, step)
    if bits == 0:
        out = r[:, None] * np.asarray(tm, dtype=np.float32).reshape(-1, 3)[p]
        assert out.dtype == np.float32
        return out
    tab = SR.tables(g) if tab is None else tab
    H, W = g.H, g.W
    ca, sa, cz, sz = tab[:H], tab[H: 2 * H], tab[2 * H: 2 * H + W], tab[2 * H + W: 2 * H + 2 * W]
    st = tab[2 * H + 2 * W:].reshape(4, SR.TABLE_CODES, 4)[bits - 1]
    h, w = p // W, p % W
    cde, sde, cda, sda = st[el, 0], st[el, 1], st[az, 2], st[az, 3]
    cosalt = ca[h] * cde - sa[h] * sde            # float64 numpy: every product and sum rounded on its own
    sinalt = sa[h] * cde + ca[h] * sde
    cosaz = cz[w] * cda - sz[w] * sda
    sinaz = sz[w] * cda + cz[w] * sda
    r = r.astype(np.float64)
    out = np.zeros((p.shape[0], 3), np.float32)
    out[:, 0] = (r * (cosalt * cosaz)).astype(np.float32)
    out[:, 1] = (r * (cosalt * sinaz)).astype(np.float32)
    out[:, 2] = (r * sinalt).astype(np.float32)
    return out


def error_bound(k, step):
    """|r - d| <= step * (0.5 + k * 2^-23): half a step from the rounding of d / step (the quotient's own rounding moves it by at most
    k * 2^-24 steps before rintf), and k * 2^-24 steps more from the product's rounding."""
    return float(np.float32(step)) * (0.5 + np.asarray(k, dtype=np.float64) * 2.0 ** -23)

"""The specification of the subpixel channel, stated once: where inside its cell the owner of a pixel lies, the 1 .. 4 bit codes, the
payload and its refusals, and the decoder's arithmetic.  The kernels (r-pcc_amd/csrc/subpixel_kernels.h) and the product code follow this
file; it is test infrastructure and never imported by the package.

Owner of a pixel.  The intensity channel's (intensity_ref.owners_loop / owners_closed): the row whose depth the projection keeps.

Offsets.  The owner's fp32 x, y, z through the projection's sequence (csrc/rpcc_hip.hip: project_point), fp32 and un-fused, atan2f the
fdlibm one (beam_table_ref.atan2f = the oracle's orc_atan2f_array):
  az = atan2f(y, x); az < 0 -> (float)((double)az + 2 * 3.14159265); el = atan2f(z, sqrtf(x*x + y*y))
  colf = az / hfov * W;  col = roundf(colf) (half away from zero), then wrapped to [0, W)
  rowf = (el - vmin) / ((vmax - vmin) / (float)(H - 1));  row = clamp(roundf(rowf), 0, H - 1)
  off_az = colf - roundf(colf)      before the wrap: a point that rounds to column W has col = 0 and a negative offset
  off_el = rowf - (float)row        after the clamp: it may lie outside +-0.5
(row, col) are asserted to be orc_project_rowcol's for every row handled.

Code.  bits in 1 .. 4, L = 1 << bits: t = (off + 0.5f) * (float)L (one fp32 add, one fp32 multiply); c = min(max((int)floorf(t), 0), L - 1);
c stands for the offset (c + 0.5) / L - 0.5 cells.

Payload 'subpixel': uint8 [8 + 2n] = b"RPS1" | bits | 0 0 0 | az codes [n] | el codes [n], one byte per code, the non-empty pixels in
ascending pixel index; n = pixels with ri != 0 = pixels whose label is not 1.

Decoder.  No trigonometry per pixel: python-float tables as the transform map is built from them (oracle.transform_map),
  alt_h = vfov * (h / (H-1)) + vmin -> ca, sa [H];   azi_w = hfov * (w / W) -> cz, sz [W]
  de = ((c + 0.5) / L - 0.5) * (vfov / (H-1)) -> cde, sde;   da = ((c + 0.5) / L - 0.5) * (hfov / W) -> cda, sda
and per non-empty pixel (h, w) with codes (a, e) and the reconstructed range r (f32), every fp64 product and sum rounded on its own:
  cosalt = ca*cde - sa*sde; sinalt = sa*cde + ca*sde; cosaz = cz*cda - sz*sda; sinaz = sz*cda + cz*sda
  x = (float)((double)r * (cosalt * cosaz)); y = (float)((double)r * (cosalt * sinaz)); z = (float)((double)r * sinalt)
Empty pixels give +0.0 in all three.

Refusals (the frame decodes to zeros): no magic; bits outside 1 .. 4; a reserved byte that is not 0; another byte count than
8 + 2 * (labels != 1); any code >= L."""
import math

import numpy as np

import beam_table_ref as BR
import intensity_ref as IR

MAGIC = b"RPS1"
TABLE_CODES = 16


def roundf(v):
    """C's roundf on float32 values: half away from zero (exact: v + 0.5 is exact in fp64)."""
    v = np.asarray(v, dtype=np.float32).astype(np.float64)
    return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.float32)


def offsets(xyz, g):
    """The projection's sequence on fp32 [N,3] rows of finite, non-zero depth -> (row i64, col i64, off_az f32, off_el f32, clamped bool: the row
    was clamped)."""
    f = np.float32
    xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    H, W = g.H, g.W
    hfov, vmax, vmin = f(g.horizontal_FOV), f(g.vertical_max), f(g.vertical_min)
    with np.errstate(all="ignore"):
        az = BR.atan2f(y, x)
        az = np.where(az < 0, (az.astype(np.float64) + 2 * 3.14159265).astype(np.float32), az)
        el = BR.atan2f(z, np.sqrt(x * x + y * y))
        colf = az / hfov * f(W)
        vres = (vmax - vmin) / f(H - 1)
        rowf = (el - vmin) / vres
    assert colf.dtype == np.float32 and rowf.dtype == np.float32 and np.float32(vres).dtype == np.float32
    rc, rr = roundf(colf), roundf(rowf)
    col = rc.astype(np.int64)
    col = np.where((col < 0) | (col >= W), np.fmod(col, W), col)          # C's %: the sign of the dividend (az >= 0: never negative)
    row = np.clip(rr.astype(np.int64), 0, H - 1)
    off_az = colf - rc
    off_el = rowf - row.astype(np.float32)
    assert off_az.dtype == np.float32 and off_el.dtype == np.float32
    return row, col, off_az, off_el, rr.astype(np.int64) != row


def code(off, bits):
    L = 1 << bits
    t = (np.asarray(off, dtype=np.float32) + np.float32(0.5)) * np.float32(L)
    assert t.dtype == np.float32
    return np.clip(np.floor(t.astype(np.float64)), 0, L - 1).astype(np.uint8)


def step(c, bits):
    """The offset a code stands for, in cells (python float)."""
    return (c + 0.5) / (1 << bits) - 0.5


def payload(az, el, bits):
    return np.frombuffer(MAGIC + bytes([bits, 0, 0, 0]) + np.asarray(az, np.uint8).tobytes() + np.asarray(el, np.uint8).tobytes(), dtype=np.uint8)


def encode_frame(rows, g, bits, owners=None):
    """rows f32 [N,>=3] -> dict(ri [P], own [P], d, pix, off_az / off_el f32 [n], clamped bool [n] (the row was clamped), az / el uint8 [n],
    codes uint8 [P,2], payload uint8 [8+2n]).  owners: (d, pix, ri, own) of these rows where they are already known (one owner pass per
    distinct frame, whatever the bits)."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    xyz = np.ascontiguousarray(rows[:, :3])
    P = g.H * g.W
    if owners is None:
        d, pix = IR.pixels(xyz, g)
        ri, own = IR.owners_loop(d, pix, P)
        assert np.array_equal(own, IR.owners_closed(d, pix, ri))
    else:
        d, pix, ri, own = owners
    set_ = ri != 0
    o = own[set_]
    row, col, off_az, off_el, clamped = offsets(xyz[o], g)
    assert np.array_equal(row * g.W + col, pix[o]) and np.array_equal(row * g.W + col, np.flatnonzero(set_))    # orc_project_rowcol's pixel
    az, el = code(off_az, bits), code(off_el, bits)
    codes = np.zeros((P, 2), np.uint8)
    codes[set_, 0], codes[set_, 1] = az, el
    return dict(ri=ri, own=own, d=d, pix=pix, off_az=off_az, off_el=off_el, clamped=clamped, az=az, el=el, codes=codes, payload=payload(az, el, bits))


def encode_frames(frames, g, bits, memo=None):
    """encode_frame of every frame of a batch; the owner pass once per distinct array (memo: a dict shared between calls with other bits)."""
    memo = {} if memo is None else memo
    out = []
    for f in frames:
        key = (f.__array_interface__["data"][0], f.shape, f.strides)
        if key not in memo:
            e = encode_frame(f, g, bits)
            memo[key] = (e["d"], e["pix"], e["ri"], e["own"])
            memo[key + (bits,)] = e
        if key + (bits,) not in memo:
            memo[key + (bits,)] = encode_frame(f, g, bits, owners=memo[key])
        out.append(memo[key + (bits,)])
    return out


def tables(g):
    """f64 [2H + 2W + 4 * 16 * 4]: ca, sa [H], cz, sz [W], then per bits 1 .. 4 and code c < L: cos / sin of the elevation step, cos / sin of
    the azimuth step (zeros for c >= L)."""
    H, W, vfov, hfov = g.H, g.W, g.vertical_FOV, g.horizontal_FOV
    alt = [vfov * (h / (H - 1)) + g.vertical_min for h in range(H)]
    azi = [hfov * (w / W) for w in range(W)]
    out = [math.cos(a) for a in alt] + [math.sin(a) for a in alt] + [math.cos(a) for a in azi] + [math.sin(a) for a in azi]
    for bits in (1, 2, 3, 4):
        for c in range(TABLE_CODES):
            if c >= 1 << bits:
                out += [0.0] * 4
                continue
            de, da = step(c, bits) * (vfov / (H - 1)), step(c, bits) * (hfov / W)
            out += [math.cos(de), math.sin(de), math.cos(da), math.sin(da)]
    return np.array(out, dtype=np.float64)


def parse_payload(data, n):
    """-> (bits, az uint8 [n], el uint8 [n]); ValueError for each of the refusals."""
    data = bytes(data)
    if len(data) < 8 or data[:4] != MAGIC:
        raise ValueError("no magic")
    bits = data[4]
    if not 1 <= bits <= 4:
        raise ValueError("bits %d" % bits)
    if data[5:8] != b"\0\0\0":
        raise ValueError("reserved bytes")
    if len(data) != 8 + 2 * n:
        raise ValueError("%d bytes for %d pixels" % (len(data), n))
    codes = np.frombuffer(data, np.uint8, offset=8)
    if codes.size and codes.max() >= 1 << bits:
        raise ValueError("code %d at %d bits" % (codes.max(), bits))
    return bits, codes[:n], codes[n:]


def decode_frame(data, labels, ri_rec, g, tab=None):
    """labels [P] (1 = empty pixel), ri_rec f32 [P] -> f32 [P,3], +0.0 where the label is 1; ValueError when the payload is refused."""
    labels = np.asarray(labels).reshape(-1)
    set_ = labels != 1
    bits, a, e = parse_payload(data, int(set_.sum()))
    tab = tables(g) if tab is None else tab
    H, W = g.H, g.W
    ca, sa, cz, sz = tab[:H], tab[H: 2 * H], tab[2 * H: 2 * H + W], tab[2 * H + W: 2 * H + 2 * W]
    st = tab[2 * H + 2 * W:].reshape(4, TABLE_CODES, 4)[bits - 1]
    p = np.flatnonzero(set_)
    h, w = p // W, p % W
    cde, sde, cda, sda = st[e, 0], st[e, 1], st[a, 2], st[a, 3]
    cosalt = ca[h] * cde - sa[h] * sde            # float64 numpy: every product and sum rounded on its own
    sinalt = sa[h] * cde + ca[h] * sde
    cosaz = cz[w] * cda - sz[w] * sda
    sinaz = sz[w] * cda + cz[w] * sda
    r = np.asarray(ri_rec, dtype=np.float32).reshape(-1)[p].astype(np.float64)
    out = np.zeros((labels.shape[0], 3), np.float32)
    out[p, 0] = (r * (cosalt * cosaz)).astype(np.float32)
    out[p, 1] = (r * (cosalt * sinaz)).astype(np.float32)
    out[p, 2] = (r * sinalt).astype(np.float32)
    return out


def direction_bound(g, bits, el):
    """Half a code bin on each axis as a 3-D distance per unit range, for a pixel whose centre ray has elevation el: the azimuth bin is an
    arc of radius cos(el), the elevation bin an arc of radius 1 -- sqrt((cos(el) * hfov / W)^2 + (vfov / (H-1))^2) / (2 L).  cos(el) is
    taken at the cell's edge nearest to the horizon (cos is largest there), so the bound holds for every point of the cell."""
    L = 1 << bits
    vres = g.vertical_FOV / (g.H - 1)
    c = np.cos(np.maximum(np.abs(el) - vres / 2, 0.0))
    return np.sqrt((c * g.horizontal_FOV / g.W) ** 2 + vres ** 2) / (2 * L)

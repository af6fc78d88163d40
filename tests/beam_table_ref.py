"""The specification of the projection through a per-beam elevation table (rpcc_project_beams, PCTransformer(cfg, channel_distribute_csv)),
stated once, in numpy.  It restates the table branch of the reference's PCTransformer.point_cloud_to_range_image
(dataset/transformer.py:68-91) on float32 [N,3] points, with the two things that branch leaves open pinned by the build:

  * the angle bits: numpy's float32 arctan2 is a SIMD routine whose bits depend on the numpy build; here every angle is the fdlibm atan2f
    sequence the library already carries (oracle: orc_atan2f_array).  On the example sweep no row, column or pixel differs from the
    genuine reference (tests/golden/beam_table_example_64E.npz);
  * a point whose depth is not finite is skipped (the reference would store inf / NaN), as rpcc_project does.

Per point, in input order (va f64 [H] radians: row h of the image = entry h; hfov a python float; everything else float32):
  1. depth = sqrtf(x*x + y*y + z*z); not finite -> skipped
  2. az = atan2f(y, x); az < 0 -> az + (float)(2 pi) in fp32        (numpy's float32 `%`, bit for bit; NOT the even path's double literal)
  3. colf = az / (float)hfov * (float)W
  4. col = rintf(colf), half to even, then mod W
  5. el = atan2f(z, sqrtf(x*x + y*y))
  6. row = the FIRST minimum over h of |va[h] - (double)el| in fp64 (the reference's clamp afterwards is a no-op)
  7. ri[row, col] = depth: the last point in input order wins; empty pixels are 0
"""
import ctypes as C

import numpy as np

TWO_PI_F = np.float32(2 * np.pi)
BEAM_MAX_H = 128


def atan2f(y, x):
    from oracle import oracle as orc
    y = np.ascontiguousarray(y, dtype=np.float32)
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.empty_like(y)
    if y.size:
        orc.lib().orc_atan2f_array(orc._p(y), orc._p(x), orc._p(out), C.c_long(y.size))
    return out


def check_table(va, H=None):
    va = np.asarray(va, dtype=np.float64).reshape(-1)
    if H is not None and va.shape[0] != H:
        raise ValueError("table length %d, RANGE_IMAGE_HEIGHT %d" % (va.shape[0], H))
    if not 1 <= va.shape[0] <= BEAM_MAX_H:
        raise ValueError("1 .. %d rows" % BEAM_MAX_H)
    if not np.isfinite(va).all():
        raise ValueError("non-finite entry")
    return va


def pixels(xyz, va, hfov, W):
    """-> (keep bool [N], row i64 [N], col i64 [N], depth f32 [N]); row / col of a skipped point are 0."""
    va = check_table(va)
    xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    with np.errstate(all="ignore"):
        depth = np.sqrt(x * x + y * y + z * z)                                   # float32 throughout: sqrtf of the fp32 sum
        keep = np.isfinite(depth)
        az = atan2f(y, x)
        az = np.where(az < 0, az + TWO_PI_F, az).astype(np.float32)
        colf = az / np.float32(hfov) * np.float32(W)
        assert colf.dtype == np.float32
        col = np.rint(np.where(keep, colf, np.float32(0))).astype(np.int64) % W
        el = atan2f(z, np.sqrt(x * x + y * y)).astype(np.float64)
        el = np.where(keep, el, 0.0)
        row = np.argmin(np.abs(va[None, :] - el[:, None]), axis=-1).astype(np.int64)    # first minimum
    return keep, np.where(keep, row, 0), np.where(keep, col, 0), depth


def project(xyz, va, hfov, H, W):
    """-> f32 [H,W]: the last point in input order wins its pixel."""
    va = check_table(va, H)
    keep, row, col, depth = pixels(xyz, va, hfov, W)
    ri = np.zeros((H, W), dtype=np.float32)
    ri[row[keep], col[keep]] = depth[keep]        # numpy assigns repeated indices in order: the last one stays
    return ri


def project_batch(xyz, offsets, va, hfov, H, W):
    return np.stack([project(xyz[offsets[b]: offsets[b + 1]], va, hfov, H, W) for b in range(len(offsets) - 1)])


def project_loop(xyz, va, hfov, H, W):
    """The same as an explicit per-point loop with scalar operations (test of the vectorised statement above)."""
    va = check_table(va, H)
    xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    ri = np.zeros((H, W), dtype=np.float32)
    f = np.float32
    az_all, el_all = atan2f(xyz[:, 1], xyz[:, 0]), None
    with np.errstate(all="ignore"):
        el_all = atan2f(xyz[:, 2], np.sqrt(xyz[:, 0] * xyz[:, 0] + xyz[:, 1] * xyz[:, 1]))
        for i in range(xyz.shape[0]):
            x, y, z = f(xyz[i, 0]), f(xyz[i, 1]), f(xyz[i, 2])
            depth = np.sqrt(f(f(f(x * x) + f(y * y)) + f(z * z)))
            if not np.isfinite(depth):
                continue
            az = f(az_all[i])
            if az < 0:
                az = f(az + TWO_PI_F)
            colf = f(f(az / f(hfov)) * f(W))
            r = float(np.floor(float(colf)))             # half to even by hand
            d = float(colf) - r
            if d > 0.5 or (d == 0.5 and int(r) % 2 == 1):
                r += 1.0
            col = int(r) % W
            el = float(el_all[i])
            best, bd = 0, abs(float(va[0]) - el)
            for h in range(1, H):
                dd = abs(float(va[h]) - el)
                if dd < bd:
                    best, bd = h, dd
            ri[best, col] = depth
    return ri


def transform_map(va, hfov, H, W):
    """The ray table of a table lidar: the unit ray of pixel (h, w) has altitude va[h] and azimuth hfov * (w / W); fp64 products of the
    python-float cosines and sines, rounded to fp32 once -- as oracle.transform_map states the even case, an outer product of per-row
    and per-column factors.  Held to the genuine reference's map by the digest in tests/golden/beam_table_example_64E.npz."""
    import math
    va = check_table(va, H)
    rows = np.array([[math.cos(a), math.sin(a)] for a in va])
    cols = np.array([[math.cos(hfov * (w / W)), math.sin(hfov * (w / W))] for w in range(W)])
    tm = np.empty((H, W, 3))
    tm[..., :2] = rows[:, None, :1] * cols[None, :, :]
    tm[..., 2] = rows[:, 1:2]
    return tm.astype(np.float32)


def beam_index(va):
    """The index rpcc_beam_index_build writes (csrc/beam_index.h), from numpy: (va f64, sorted f64, mid f32 with a +inf pad, row i32)."""
    va = check_table(va)
    order = np.argsort(va, kind="stable")
    s = va[order]
    row = order.astype(np.int32)
    for k in range(1, len(s)):
        if s[k] == s[k - 1]:
            row[k] = row[k - 1]
    mid = np.full(len(s), np.inf, dtype=np.float32)
    mid[:-1] = (s[:-1] * 0.5 + s[1:] * 0.5).astype(np.float32)
    return va, s, mid, row


def index_bytes(va):
    a, s, mid, row = beam_index(va)
    return a.tobytes() + s.tobytes() + mid.tobytes() + row.tobytes()


def read_csv(path):
    import csv
    with open(path) as f:
        return np.radians(np.array([float(r["vertical_angle"]) for r in csv.DictReader(f)]))

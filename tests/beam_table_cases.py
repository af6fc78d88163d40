"""The constructed inputs of the per-beam table projection's GPU tests (tests/test_gpu_beam_table.py): small tables at H = 1, 2, 5 and,
per table and width, a few thousand points placed where the pixel decision can go wrong.  tests/test_beam_table_ref.py checks, without a
GPU, that the sets do reach the values they aim at (elevations AT the float32 midpoints and the float32 values around them, pre-rounding
columns at exact halves, 0 and W)."""
import math

import numpy as np

import beam_table_ref as R

HFOV = 360 * (np.pi / 180)


def ray(az, el, r=10.0):
    return [r * math.cos(el) * math.cos(az), r * math.cos(el) * math.sin(az), r * math.sin(el)]


def tables(H):
    """name -> (table, a point whose elevation is an exact fp64 tie between two of its entries or None)"""
    p = np.array([ray(1.0, 0.3, 7.0)], dtype=np.float32)
    el = float(R.atan2f(p[:, 2], np.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2))[0])
    if H == 1:
        return {"single": (np.array([-0.1]), None)}
    if H == 2:
        return {"pair": (np.array([-0.2, 0.05]), None), "descending": (np.array([0.05, -0.2]), None), "equal": (np.array([0.01, 0.01]), None),
                "ulp": (np.array([0.01, np.nextafter(0.01, 1.0)]), None), "tie": (np.array([el + 0.25, el - 0.25]), p[0])}
    base = np.radians([-24.0, -17.5, -9.0, -8.5, 2.0])
    return {"ascending": (base, None), "descending": (base[::-1].copy(), None), "shuffled": (base[[2, 4, 0, 3, 1]].copy(), None),
            "equal": (np.radians([-24.0, -9.0, -17.5, -9.0, 2.0]), None),
            "ulp": (np.array([-0.4, -0.15, np.nextafter(-0.15, 0.0), float(np.nextafter(np.float32(-0.15), np.float32(0))), 0.03]), None),
            "tie": (np.array([-0.4, el - 0.125, 0.9, el + 0.125, -0.2]), p[0])}


def constructed(va, W, tie):
    rng = np.random.default_rng(len(va) * 1000 + W)
    lo, hi = float(va.min()), float(va.max())
    pts = [ray(a, e, r) for a, e, r in zip(rng.uniform(0, 2 * np.pi, 1500), rng.uniform(lo - 0.1, hi + 0.1, 1500), rng.uniform(0.5, 80, 1500))]
    radii = rng.uniform(1.0, 60.0, 48)
    s = np.sort(va)
    for m in (s[:-1] * 0.5 + s[1:] * 0.5):                # elevations at every sorted midpoint and the float32 values around it
        m32 = np.float32(m)
        ulp = float(np.spacing(np.abs(m32))) if m32 != 0 else 1e-45
        for d in (-2, -1, -0.5, 0, 0.5, 1, 2):
            pts += [ray(0.7 + 0.01 * j, float(m) + d * ulp, r) for j, r in enumerate(radii)]
    step = 2 * np.pi / W
    for k in (0.5, 1.5, 2.5, 3.5, W - 0.5, W - 1.5):      # columns at the halves (even and odd neighbours), float32 neighbours included
        for d in (-2, -1, 0, 1, 2):
            a32 = float(np.float32(k * step)) + d * float(np.spacing(np.float32(k * step)))
            pts += [ray(a32, lo, r) for r in radii[:12]]
    pts += [[r, 0.0, 0.0] for r in (3.0, 9.0, 5.0)]        # column 0 exactly; three points on one pixel whose nearest is first
    pts += [[4.0, -0.0, 0.5], [4.0, -1e-30, 0.5], [4.0, -1e-9, 0.5], [4.0, -4e-7, 0.5], [-4.0, -1e-30, 0.5]]   # az -0.0, tiny negative (rounds to W -> 0)
    q = np.array(ray(2.0, hi, 1.0), dtype=np.float32)
    pts += [list(q * 2), list(q * 8), list(q * 4)]         # exact scalings: one pixel, the nearest first, the last one stays
    pts += [[2.0, 0.0, 0.0], [0.0, 0.0, 0.0], [6.0, 0.0, 0.0]]   # a depth-0 point in the middle of its pixel's run
    pts += [[np.nan, 1, 1], ray(3.0, lo, 5.0), [np.inf, 0, 0], [3e19, 3e19, 1.0], ray(3.0, hi, 6.0), [1, -np.inf, 2], [1, 1, np.nan]]
    pts += [ray(4.0, lo - 0.6, 5.0), ray(4.0, hi + 0.6, 5.0), [0.0, 0.0, 3.0], [0.0, 0.0, -3.0], [1e-20, 1e-20, 1e-20], [1e18, 1e18, 1e17]]
    if tie is not None:
        pts += [list(tie), list(tie * 2)]
    return np.array(pts, dtype=np.float32)

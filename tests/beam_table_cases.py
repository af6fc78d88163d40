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


# ---- past the grid caps ------------------------------------------------------------------------------------------------------------------
PAST_H, PAST_W, PAST_N = 16, 512, 8191
PAST_HEAD = 1100                                  # leading points of the seam frame, all uncertain; every second one an elevation tie as well
PAST_THIN = 1024                                  # the seam frame's last points: a fifth uncertain, so a chunk over the frame's end queues less than a drain
PAST_RUN = 200                                    # real points of the (0, 0, 0) pixel in front of the zero that ends the zero-last frame
PAST_TIE_HALF = 2.0 ** -7                         # two table entries are moved to el -+ this around the tie direction's float32 elevation el (exact in fp64)


def past_table():
    """-> (va f64 [16] ascending, tie direction f32 [3]).  The `16 uneven` recipe (sorted uniform draws in +-0.3 rad, fixed seed) with two
    neighbouring entries moved so that the float32 elevation of one direction at azimuth 0 lies exactly between them in fp64 (tables()'s tie
    recipe).  Its y is 0 and may be set to anything below 2^-13 |x|: x*x + y*y then still rounds to x*x and the elevation keeps its bits."""
    va = np.sort(np.random.default_rng(11).uniform(-0.3, 0.3, PAST_H))
    j = int(np.argmax(np.diff(va)))                  # the widest gap (above 0.6 / 15 rad): its two entries move inwards
    p = np.array([ray(0.0, float(va[j] * 0.5 + va[j + 1] * 0.5), 8.0)], dtype=np.float32)
    el = float(R.atan2f(p[:, 2], np.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2))[0])
    va[j], va[j + 1] = el - PAST_TIE_HALF, el + PAST_TIE_HALF
    assert np.all(np.diff(va) > 2e-4), "a gap of the table is too narrow for _past_plain's margins: another seed"
    return va, p[0]


def _past_plain(va, rng, n):
    """Points within a quarter cell of a pixel centre in columns 2 .. W - 2, within a fifth of the way from a table entry to its neighbours'
    midpoints, at 1 .. 60 m: the fast path is certain of every one."""
    h = rng.integers(0, len(va), n)
    gap = np.minimum(np.diff(va, prepend=va[0] - 0.05), np.diff(va, append=va[-1] + 0.05))[h] / 2
    el = va[h] + rng.uniform(-0.2, 0.2, n) * gap
    az = (rng.integers(2, PAST_W - 1, n) + rng.uniform(-0.25, 0.25, n)) * (2 * np.pi / PAST_W)
    r = rng.uniform(1.0, 60.0, n)
    return np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], 1).astype(np.float32)


def _past_seam(va, rng, n):
    """Points within 0.4 cell of column 0 or of column W, which wraps: the fast path refuses both (c0 >= 1, c0 <= W - 1)."""
    el = va[rng.integers(0, len(va), n)] + rng.uniform(-0.004, 0.004, n)
    az = (rng.choice([0.0, float(PAST_W)], n) + rng.uniform(-0.4, 0.4, n)) * (2 * np.pi / PAST_W)
    r = rng.uniform(1.0, 60.0, n)
    return np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], 1).astype(np.float32)


def _past_ties(tie, rng, n):
    """The tie direction scaled by powers of two (exact), y anywhere within 2^-14 |x| on either side of the seam."""
    s = (2.0 ** rng.integers(-2, 3, n)).astype(np.float32)
    out = tie[None, :] * s[:, None]
    out[:, 1] = (rng.uniform(-1, 1, n) * 2.0 ** -14 * out[:, 0]).astype(np.float32)
    return out.astype(np.float32)


def _past_ties_anywhere(tie, rng, n, parity):
    """Exact ties in ordinary columns (those of 2 .. W - 2 with the given parity, within a quarter cell of the centre): x, y with
    sqrtf(x*x + y*y) == |tie.x| in float32, by rejection, and the tie's z, all scaled by a power of two.  The elevation has the tie's bits, so the fast path refuses the row by its
    margin at the midpoint and the exact sequence gives the lower row -- in a pixel that few other points share, so a tie that gets lost
    shows in the image (a point at the seam shares its pixel with thousands)."""
    rho = np.float32(abs(tie[0]))
    out = np.empty((0, 3), np.float32)
    while out.shape[0] < n:
        az = (2 * rng.integers(1, PAST_W // 2 - 1, 4 * n) + parity + rng.uniform(-0.25, 0.25, 4 * n)) * (2 * np.pi / PAST_W)
        x, y = (float(rho) * np.cos(az)).astype(np.float32), (float(rho) * np.sin(az)).astype(np.float32)
        ok = np.sqrt(x * x + y * y) == rho
        out = np.concatenate([out, np.stack([x[ok], y[ok], np.full(int(ok.sum()), tie[2], np.float32)], 1)])
    return out[:n] * (2.0 ** rng.integers(-2, 3, n)).astype(np.float32)[:, None]


def past_the_grid_frames(min_points, min_pixels):
    """-> dict(va, H, W, frames, distinct, which, aimed_fast, tie): the frames zero-last, seam, plain and an empty one (8191 / 8191 / 8191 / 0 points)
    in a cycle until the batch holds at least min_points points and more than min_pixels pixels.
      zero-last  plain points, then PAST_RUN points (d, 0, 0) of the pixel (0, 0, 0) lands in, then (0, 0, 0): the last point wins, the pixel is 0
      seam       PAST_HEAD uncertain points (at the seam; every second one an exact elevation tie, half of those in ordinary columns), then two
                 points in five uncertain (a fifth of the last PAST_THIN), every second of them such a tie in an ordinary column
      plain      seeded points the fast path is certain of"""
    va, tie = past_table()
    rng = np.random.default_rng(12)
    n = PAST_N
    zl = _past_plain(va, rng, n)
    zl[n - 1 - PAST_RUN: n - 1] = np.stack([rng.uniform(1.0, 60.0, PAST_RUN), np.zeros(PAST_RUN), np.zeros(PAST_RUN)], 1).astype(np.float32)
    zl[n - 1] = 0
    zl_fast = np.ones(n, bool)
    zl_fast[n - 1 - PAST_RUN:] = False
    unsure = np.ones(n, bool)
    unsure[PAST_HEAD:] = rng.random(n - PAST_HEAD) < 0.4
    unsure[n - PAST_THIN:] = rng.random(PAST_THIN) < 0.2
    seam = _past_plain(va, rng, n)
    seam[unsure] = _past_seam(va, rng, int(unsure.sum()))
    seam[0: PAST_HEAD: 4] = _past_ties(tie, rng, len(range(0, PAST_HEAD, 4)))
    head, behind = np.arange(2, PAST_HEAD, 4), np.flatnonzero(unsure[PAST_HEAD:])[::2] + PAST_HEAD
    seam[head] = _past_ties_anywhere(tie, rng, head.shape[0], 1)          # (odd columns: no later tie of the frame takes a pixel from them)
    seam[behind] = _past_ties_anywhere(tie, rng, behind.shape[0], 0)
    distinct = [zl, seam, _past_plain(va, rng, n), np.zeros((0, 3), np.float32)]
    fast = [zl_fast, ~unsure, np.ones(n, bool), np.zeros(0, bool)]
    B, points = 0, 0
    while points < min_points or B * PAST_H * PAST_W <= min_pixels:
        points += distinct[B % 4].shape[0]
        B += 1
    which = np.arange(B) % 4
    return dict(va=va, H=PAST_H, W=PAST_W, frames=[distinct[k] for k in which], distinct=distinct, which=which, aimed_fast=fast, tie=tie)


def past_the_grid():
    """About 360 frames and 2.2 M points at 16 x 512: 131 072 points past the cap of beams_pix_kernel, past those of beams_write_kernel and
    beams_fill_kernel (sized from tests/grid_caps.py; tests/test_beam_table_ref.py asserts what the batch reaches)."""
    import grid_caps as GC
    return past_the_grid_frames(max(GC.BEAMS_PIX_CAP * GC.BEAMS_CHUNK + 131072, GC.BEAMS_WRITE_CAP * GC.BEAMS_WRITE_THREADS + 1),
                                GC.BEAMS_FILL_CAP * GC.BEAMS_FILL_THREADS)


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

"""Named, seeded inputs of the intensity tests, shared by the CPU and the GPU files.  CASES[name]() -> a list of batches
dict(g=oracle.LidarGeom, frames=[f32 [N,4] rows, ...], scale=float); expected values come from tests/intensity_ref.py."""
import os

import numpy as np

from oracle import oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TINY = dict(H=4, W=16, hfov_deg=360, vmax_deg=2.0, vmin_deg=-24.9)


def rays(g, row, col, depth, w, jitter=None):
    """Rows (x, y, z, w) aimed at the pixel centres (row, col) -- fractional values aim elsewhere in the cell -- at the given depths."""
    row, col, depth = (np.asarray(v, dtype=np.float64) for v in (row, col, depth))
    if jitter is not None:
        row, col = row + jitter.uniform(-0.4, 0.4, row.shape), col + jitter.uniform(-0.4, 0.4, col.shape)
    el = g.vertical_min + row * (g.vertical_max - g.vertical_min) / (g.H - 1)
    az = col * g.horizontal_FOV / g.W
    out = np.empty(row.shape + (4,), np.float32)
    out[:, 0], out[:, 1], out[:, 2] = depth * np.cos(el) * np.cos(az), depth * np.cos(el) * np.sin(az), depth * np.sin(el)
    out[:, 3] = w
    return out


def cloud(g, n, rng, cols=None):
    """n random rows inside the field of view, intensities k / 100."""
    col = rng.uniform(0, g.W, n) if cols is None else rng.choice(cols, n) + rng.uniform(-0.4, 0.4, n)
    return rays(g, rng.uniform(0, g.H - 1, n), col, rng.uniform(1.0, 60.0, n), rng.integers(0, 100, n) / np.float32(100))


def _batch(g, frames, scale):
    return dict(g=g, frames=[np.ascontiguousarray(f, dtype=np.float32).reshape(-1, 4) for f in frames], scale=float(scale))


def tiny():
    g = orc.LidarGeom(**TINY)
    return [_batch(g, [cloud(g, 200, np.random.default_rng(1))], 255)]


def ties():
    """Rows duplicated exactly (same xyz, other intensity) at several input positions: the first after z(pix) owns."""
    g, rng = orc.LidarGeom(**TINY), np.random.default_rng(2)
    f = cloud(g, 60, rng)
    dup = f[rng.integers(0, 60, 40)].copy()
    dup[:, 3] = rng.integers(0, 100, 40) / np.float32(100)
    f = np.concatenate([dup[:10], f[:30], dup[10:25], f[30:], dup[25:]])
    return [_batch(g, [f, f[::-1]], 255)]


def zeros():
    """(0, 0, 0, w) rows land in column 0 of the row elevation 0 maps to; (d, 0, 0, w) rows are the real points of that pixel."""
    g, rng = orc.LidarGeom(**TINY), np.random.default_rng(3)
    pt = lambda d, w: np.array([[d, 0, 0, w]], np.float32)
    scenes = [[(5, .1), (3, .2), (0, .3)],                                   # a zero last: the pixel is empty, the payload one shorter
              [(3, .1), (0, .2), (5, .3)],                                   # the smaller depth before the zero
              [(5, .1), (0, .2), (7, .3), (3, .4)],                          # the smaller depth after it
              [(2, .1), (0, .2), (4, .3), (0, .4), (6, .5), (6, .6)],        # two zeros, then a tie
              [(5, .1), (0, .2), (5, .3)],                                   # the same depth on both sides of the zero: the later row owns
              [(0, .7)]]                                                     # nothing but a zero
    frames = []
    for sc in scenes:
        other = cloud(g, 40, rng, cols=np.arange(1, g.W - 1))                # (never in column 0)
        parts, cuts = [], np.sort(rng.integers(0, 41, len(sc)))
        last = 0
        for (d, w), c in zip(sc, cuts):
            parts += [other[last:c], pt(d, w)]
            last = c
        frames.append(np.concatenate(parts + [other[last:]]))
    frames.append(cloud(g, 40, rng))                                         # a frame without any zero beside flagged ones
    return [_batch(g, frames, 255)]


def nonfinite():
    """NaN / +-inf coordinates: rows skipped.  NaN, +inf, -inf, -0.0, negative and huge intensities: 0, 255, 0, 0, 0, 255."""
    g, rng = orc.LidarGeom(**TINY), np.random.default_rng(4)
    w = np.array([np.nan, np.inf, -np.inf, -0.0, -3.0, 1e30], np.float32)
    odd = rays(g, [0, 1, 2, 3, 0, 1], [1, 3, 5, 7, 9, 11], [0.5] * 6, w)         # (nearer than every point of cloud(): they own)
    bad = cloud(g, 6, rng)
    bad[0, 0], bad[1, 1], bad[2, 2], bad[3, 0], bad[4, :3], bad[5, 1] = np.nan, np.inf, -np.inf, -np.inf, np.nan, np.nan
    far = rays(g, [2], [13], [3.0e38], [0.5])                                 # x*x overflows: depth inf, skipped
    f = np.concatenate([bad[:3], odd, cloud(g, 30, rng), bad[3:], far])
    return [_batch(g, [f], 255)]


def rounding():
    g, rng = orc.LidarGeom(H=4, W=64, hfov_deg=360, vmax_deg=2.0, vmin_deg=-24.9), np.random.default_rng(5)
    half = rays(g, [0, 1, 2], [1, 2, 3], [5.0] * 3, np.array([0.25, 0.75, 1.25], np.float32))          # scale 2: 0.5, 1.5, 2.5 -> 0, 2, 2
    k = np.arange(100)
    cents = rays(g, k // 50, 2 + k % 50, [7.0] * 100, (k / 100).astype(np.float32))                    # fl(k / 100): bit-exact at scale 100
    return [_batch(g, [half], 2), _batch(g, [cents], 100), _batch(g, [cloud(g, 300, rng)], 255)]


def wrap_clamp():
    """Azimuth just below 2 pi (column W -> 0), elevations beyond both ends (clamped rows), against ordinary points of the same pixels."""
    g, rng = orc.LidarGeom(**TINY), np.random.default_rng(6)
    wrap = rays(g, [0, 1, 2, 3], [g.W - 0.01] * 4, [.3, .9, .3, .9], [.11, .12, .13, .14])          # (all nearer than cloud()'s points)
    col0 = rays(g, [0, 1, 2, 3], [0.01] * 4, [.6] * 4, [.21, .22, .23, .24])
    over = rays(g, [g.H + 3, -5, g.H - 0.6, -0.4], [4, 4, 6, 6], [.2, .2, .8, .8], [.31, .32, .33, .34])
    edge = rays(g, [g.H - 1, 0, g.H - 1, 0], [4, 4, 6, 6], [.5] * 4, [.41, .42, .43, .44])
    f = np.concatenate([wrap, col0, over, edge, cloud(g, 50, rng)])
    return [_batch(g, [f[rng.permutation(f.shape[0])]], 255)]


def frames():
    """B = 5 with N = 0, 1, 63, 64, 4099: an empty frame (the header alone), frame ends inside a wavefront, more than two 2048-point chunks."""
    g, rng = orc.LidarGeom(H=8, W=128, hfov_deg=360, vmax_deg=2.0, vmin_deg=-24.9), np.random.default_rng(7)
    return [_batch(g, [cloud(g, n, rng) for n in (0, 1, 63, 64, 4099)], 255)]


def odd_P():
    """H = 31, W = 997 (P no multiple of 64), B = 3: an empty frame, a dense one (2 P points), one with every other column."""
    g, rng = orc.LidarGeom(H=31, W=997, hfov_deg=360, vmax_deg=10.67, vmin_deg=-30.67), np.random.default_rng(8)
    P = g.H * g.W
    return [_batch(g, [np.zeros((0, 4), np.float32), cloud(g, 2 * P, rng), cloud(g, P // 2, rng, cols=np.arange(0, g.W, 2))], 255)]


def example():
    """The example sweep, 64 x 2000, scale 100: xyz of example_64E.npz, the fourth column k / 100 from intensity_example_64E.npz."""
    g = orc.LidarGeom(**orc.GEOMS["Velodyne64E"])
    xyz = np.load(os.path.join(GOLDEN, "example_64E.npz"))["xyz"]
    k = np.load(os.path.join(GOLDEN, "intensity_example_64E.npz"))["k"]
    rows = np.concatenate([xyz, (k.astype(np.float32) / np.float32(100))[:, None]], 1)
    return [_batch(g, [rows], 100)]


# ---- past the grid caps ------------------------------------------------------------------------------------------------------------------
PAST_GEOM = dict(H=16, W=512, hfov_deg=360, vmax_deg=2.0, vmin_deg=-24.9)
PAST_N = 6001                                     # rows of a frame: odd, so frame ends fall inside wavefronts and chunk boundaries move from cycle to cycle
PAST_HEAD = 700                                   # leading rows of a seam frame that are all aimed at the seam
PAST_DEPTHS = (2.5, 4.0, 6.0, 9.0, 13.0, 19.0, 27.0, 40.0)
PAST_DEPTH_P = (0.01, 0.04, 0.10, 0.17, 0.17, 0.17, 0.17, 0.17)     # the nearest depth is rare: a pixel's owner lies anywhere in its frame
PAST_ZERO_AT, PAST_RUN = 320, 300                 # the constructed zero of the `zero` frame and the run of its own pixel's rows behind it


def _past_w(n):
    """n intensities that all differ, q = (97 i) mod 256 at scale 255: rows 1 .. 255 places apart never share a byte."""
    i = np.arange(n)
    return (((i * 97) % 256 + 0.3 * i / max(n, 1)) / 255).astype(np.float32)


def _past_pool(g, rng):
    """Seam directions: f32 [H, depths, 4 aims, 3], every one within 0.4 cell of column 0 or of column W (which wraps) and a quarter cell of its
    row.  Rows drawn from the pool repeat exactly, so equal depths in one pixel are bit-equal and only the input position tells them apart."""
    H, D = g.H, len(PAST_DEPTHS)
    row = np.repeat(np.arange(H), D * 4) + rng.uniform(-0.25, 0.25, H * D * 4)
    col = rng.choice([0.0, float(g.W)], H * D * 4) + rng.uniform(-0.4, 0.4, H * D * 4)
    dep = np.tile(np.repeat(np.asarray(PAST_DEPTHS), 4), H)
    return rays(g, row, col, dep, 0.0)[:, :3].reshape(H, D, 4, 3)


def _past_seam(pool, rng, n, rows=None):
    rows = rng.integers(0, pool.shape[0], n) if rows is None else np.asarray(rows)
    return pool[rows, rng.choice(len(PAST_DEPTHS), n, p=PAST_DEPTH_P), rng.integers(0, 4, n)]


def _past_plain(g, rng, n):
    """Rows aimed within a quarter cell of a pixel centre in columns 2 .. W - 2 at 1 .. 60 m: the screened fast path is certain of every one."""
    row = rng.integers(0, g.H, n) + rng.uniform(-0.25, 0.25, n)
    col = rng.integers(2, g.W - 1, n) + rng.uniform(-0.25, 0.25, n)
    return rays(g, row, col, rng.uniform(1.0, 60.0, n), 0.0)[:, :3]


def _past_seam_frame(g, pool, rng):
    """-> (rows f32 [PAST_N,4], aimed_fast bool [PAST_N]).  The first PAST_HEAD rows all at the seam, every image row among them; behind them
    three rows in four at the seam, at random, and the fourth an ordinary one."""
    n = PAST_N
    seam = np.ones(n, bool)
    seam[PAST_HEAD:] = rng.random(n - PAST_HEAD) < 0.75
    rows = np.empty((n, 4), np.float32)
    head_rows = rng.permutation(np.arange(PAST_HEAD) % g.H)
    rows[:PAST_HEAD, :3] = _past_seam(pool, rng, PAST_HEAD, head_rows)
    rest = np.flatnonzero(seam[PAST_HEAD:]) + PAST_HEAD
    rows[rest, :3] = _past_seam(pool, rng, rest.shape[0])
    rows[~seam, :3] = _past_plain(g, rng, int((~seam).sum()))
    rows[:, 3] = _past_w(n)
    return rows, ~seam


def past_zero_pixel(g):
    """The pixel (0, 0, 0) lands in: column 0 of the row elevation 0 maps to."""
    import intensity_ref as R
    return int(R.pixels(np.zeros((1, 3), np.float32), g)[1][0])


def _past_zero_frame(g, pool, rng):
    """A seam frame with (0, 0, 0, w) rows sprinkled in.  The constructed one stands at PAST_ZERO_AT with PAST_RUN seam rows of its own pixel
    behind it; rows of the nearest depth of that pixel stand before it (10 rows from 100 on) and inside the run, so the pixel's owner is
    another row with and without the rule about zeros.  The other zeros all come later, and none behind row 5000."""
    rows, fast = _past_seam_frame(g, pool, rng)
    r0 = past_zero_pixel(g) // g.W
    own = lambda n: _past_seam(pool, rng, n, np.full(n, r0))
    nearest = pool[r0, 0, 1]
    rows[PAST_ZERO_AT + 1: PAST_ZERO_AT + 1 + PAST_RUN, :3] = own(PAST_RUN)
    rows[100:110, :3] = nearest
    rows[PAST_ZERO_AT + 40: PAST_ZERO_AT + 44, :3] = nearest
    rows[5500:5510, :3] = nearest
    fast[5500:5510] = False
    zeros_at = np.concatenate([[PAST_ZERO_AT], rng.choice(np.arange(PAST_HEAD, 5000), 12, replace=False)])
    rows[zeros_at, :3] = 0
    fast[zeros_at] = False
    return rows, fast


def past_the_grid_frames(min_rows, min_pixels):
    """-> the batch: the four distinct frames (seam, plain, zero, empty) in a cycle until the batch holds at least min_rows rows and more than
    min_pixels pixels.  Besides g / frames / scale: distinct (the four frames; batch position b holds distinct[which[b]], the same array),
    which, aimed_fast (per distinct frame: the rows the fast path is certain of by construction)."""
    g, rng = orc.LidarGeom(**PAST_GEOM), np.random.default_rng(9)
    pool = _past_pool(g, rng)
    seam, seam_fast = _past_seam_frame(g, pool, rng)
    plain = np.concatenate([_past_plain(g, rng, PAST_N), _past_w(PAST_N)[:, None]], 1).astype(np.float32)
    zero, zero_fast = _past_zero_frame(g, pool, rng)
    distinct = [np.ascontiguousarray(f, dtype=np.float32) for f in (seam, plain, zero, np.zeros((0, 4), np.float32))]
    fast = [seam_fast, np.ones(PAST_N, bool), zero_fast, np.zeros(0, bool)]
    B, rows = 0, 0
    while rows < min_rows or B * g.H * g.W <= min_pixels:
        rows += distinct[B % 4].shape[0]
        B += 1
    which = np.arange(B) % 4
    return dict(g=g, frames=[distinct[k] for k in which], scale=255.0, distinct=distinct, which=which, aimed_fast=fast)


def past_the_grid():
    """B = 247 frames of 6001 / 6001 / 6001 / 0 rows at 16 x 512: 1 116 186 rows and 2 023 424 pixels, the smallest batch of this cycle that takes
    intensity_fill_kernel and intensity_owner_kernel<false> through a second trip and the fix-up pass through a third, 65 536 rows past
    the cap of the owner pass (sized from tests/grid_caps.py; tests/test_intensity_ref.py asserts what the batch reaches)."""
    import grid_caps as GC
    return [past_the_grid_frames(GC.INT_OWNER_CAP * GC.INT_THREADS + 65536, GC.INT_FILL_CAP * GC.INT_FILL_THREADS)]


CASES = dict(tiny=tiny, ties=ties, zeros=zeros, nonfinite=nonfinite, rounding=rounding, wrap_clamp=wrap_clamp, frames=frames, odd_P=odd_P,
             example=example, past_the_grid=past_the_grid)
SMALL = tuple(n for n in CASES if n not in ("odd_P", "example", "past_the_grid"))     # the cases whose reference takes milliseconds


def offsets(frames_):
    o = np.zeros(len(frames_) + 1, np.int64)
    o[1:] = np.cumsum([f.shape[0] for f in frames_])
    return o

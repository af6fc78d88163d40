"""Named, seeded inputs of the subpixel tests, shared by the CPU and the GPU files.  CASES[name]() -> one batch
dict(g=oracle.LidarGeom, frames=[f32 [N,4] rows, ...] (B = 3, the middle one empty), pad=(rows before offsets[0], rows behind
offsets[B]) or None, hostile=dict or None); expected values come from tests/subpixel_ref.py.

The hostile table (hostile_rows): rows found by search whose fp32 offsets, through the exact sequence of subpixel_ref.offsets, are exactly
k / 16 - 0.5 cells for every k = 0 .. 15 on either axis -- t = (off + 0.5) * L is then an integer for every bits with L | k, and k = 0 is the
offset -0.5 -- plus the offset only a clamped row can have (+0.5, at the top), a row clamped just below row 0, a point that rounds to column W, rows
clamped above and below by more than a cell, two points of equal depth bits in one pixel with different offsets, NaN / inf rows, and the
depth-0 scenes of the flagged-frame pass.  Every hostile row is nearer than every row of cloud(), so it owns its pixel."""
import os

import numpy as np

import intensity_cases as IC
import subpixel_ref as S
from oracle import oracle as orc

GOLDEN = IC.GOLDEN
SMALL = dict(H=4, W=24, hfov_deg=360, vmax_deg=2.0, vmin_deg=-24.9)
ROUND2 = dict(H=5, W=1000, hfov_deg=360, vmax_deg=2.0, vmin_deg=-24.9)      # P = 5000: a second round of 1024 x 4 pixels with a partial tail
STEPS = 16                # offsets k / 16 - 0.5: every code boundary of bits 1 .. 4
TRIES = 64                # candidates per (axis, k)


def _exact(g, axis, k, rng, pixels):
    """Rows aimed at offset k / 16 - 0.5 on `axis` of random pixels among `pixels` [(row, col)], the other axis anywhere inside the cell,
    at 0.3 .. 0.9 m -> (rows f32 [n,4], pix i64 [n]) of those whose fp32 offset is exactly that value and whose row is not clamped."""
    at = pixels[rng.integers(0, len(pixels), TRIES)]
    want = k / STEPS - 0.5
    other = rng.uniform(-0.4, 0.4, TRIES)
    row = at[:, 0] + (want if axis == "el" else other)
    col = at[:, 1] + (want if axis == "az" else other)
    rows = IC.rays(g, row, col, rng.uniform(0.3, 0.9, TRIES), 0.0)
    r, c, off_az, off_el, clamped = S.offsets(rows[:, :3], g)
    hit = ((off_az if axis == "az" else off_el) == np.float32(want)) & ~clamped
    return rows[hit], (r * g.W + c)[hit]


def hostile_rows(g, seed):
    """-> (rows f32 [n,4], dict(exact={(axis, k): index into rows}, clamp_top, clamp_bottom, wrap, far_above, far_below, tie=(i, j))): every
    row in a pixel of its own except the tie pair, none in column 0's zero pixel."""
    rng = np.random.default_rng(seed)
    H, W = g.H, g.W
    zero_pix = IC.past_zero_pixel(g)
    tie_col = W // 8                                                  # azimuth 45 degrees: the centre of this column (W is a multiple of 8)
    free = np.array([(r, c) for r in range(1, H - 1) for c in range(1, W - 1) if c != tie_col and r * W + c != zero_pix])
    taken, rows, where = set(), [], dict(exact={})

    def add(row, key=None):
        rows.append(row)
        if key is not None:
            where[key] = len(rows) - 1
        return len(rows) - 1

    for axis in ("az", "el"):
        for k in range(STEPS):
            for _ in range(8):                                        # (a search: most draws hold several exact rows)
                cand, pix = _exact(g, axis, k, rng, free)
                new = [i for i in range(len(pix)) if int(pix[i]) not in taken]
                if new:
                    taken.add(int(pix[new[0]]))
                    where["exact"][(axis, k)] = add(cand[new[0]])
                    break
    ray = lambda row, col, depth: IC.rays(g, [row], [col], [depth], 0.0)[0]
    # +0.5 exists only where the row is clamped at the top (rowf = H - 1 + 0.5 rounds to H): searched around column 2
    cand = IC.rays(g, np.full(4000, H - 0.5), 2 + rng.uniform(-0.3, 0.3, 4000), rng.uniform(0.3, 0.9, 4000), 0.0)
    _, _, _, off_el, clamped = S.offsets(cand[:, :3], g)
    add(cand[np.flatnonzero(clamped & (off_el == np.float32(0.5)))[0]], "clamp_top")
    add(ray(-0.6, 3, 0.5), "clamp_bottom")                            # just below row 0: clamped, offset about -0.6 (exactly -0.5 is the unclamped k = 0)
    add(ray(1, W - 0.3, 0.5), "wrap")                                 # rounds to column W: column 0, offset about -0.3
    add(ray(H + 0.8, 5, 0.5), "far_above")                            # clamped by more than a cell: el codes L - 1 / 0
    add(ray(-1.7, 6, 0.5), "far_below")
    # two rows of equal depth bits in one pixel: (x, y, z) and (y, x, z) around azimuth 45 degrees (x*x + y*y is the same fp32 sum)
    a = ray(1, tie_col - 0.2, 0.7)
    b = a.copy()
    b[0], b[1] = a[1], a[0]
    where["tie"] = (add(a), add(b))
    return np.array(rows, np.float32), where


def _scene(g, seed):
    """B = 3: [hostile + cloud + depth-0 scene `a real point behind the zero`, empty, cloud + ties + NaN / inf + depth-0 `zero last`]."""
    rng = np.random.default_rng(seed)
    host, where = hostile_rows(g, seed + 100)
    n = min(3 * g.H * g.W, 6000)
    zr, zc = divmod(IC.past_zero_pixel(g), g.W)
    inpix = lambda depth, d_row, d_col: IC.rays(g, [zr + d_row], [zc + d_col], [depth], 0.0)      # a row of the zero pixel (column 0: d_col >= 0 keeps it there)
    zero = np.zeros((1, 4), np.float32)
    c0 = IC.cloud(g, n, rng)
    # nearer before the zero (it would own without the rule), the zero, two farther rows behind it: the nearer of those owns
    f0 = np.concatenate([host, c0[: n // 3], inpix(0.4, 0.2, 0.3), c0[n // 3: n // 2], zero, inpix(0.8, -0.3, 0.1), c0[n // 2:], inpix(0.6, 0.1, 0.4)])
    c2 = IC.cloud(g, n // 2, rng)
    dup = c2[rng.integers(0, c2.shape[0], 40)].copy()                                              # exact duplicates: the lower index owns (same codes)
    bad = IC.cloud(g, 6, rng)
    bad[0, 0], bad[1, 1], bad[2, 2], bad[3, 0], bad[4, :3], bad[5, 1] = np.nan, np.inf, -np.inf, -np.inf, np.nan, np.nan
    far = IC.rays(g, [1], [7], [3.0e38], [0.5])                                                     # x*x overflows: depth inf, skipped
    tie = host[list(where["tie"])][::-1]                                                            # the pair in the other order: the other row owns
    f2 = np.concatenate([bad[:3], c2[:100], tie, dup, c2[100:], bad[3:], far, inpix(0.4, 0.2, 0.3), zero])   # the zero last: its pixel is empty
    frames = [np.ascontiguousarray(f, dtype=np.float32) for f in (f0, np.zeros((0, 4), np.float32), f2)]
    # rows in front of offsets[0] and behind offsets[B]: nearer than anything, they would own their pixels if they were counted
    pad = (IC.rays(g, [1, 2, 1], [3, 4, 9], [0.05] * 3, 0.0), IC.rays(g, [2, 1], [8, 2], [0.05] * 2, 0.0))
    return dict(g=g, frames=frames, pad=pad, hostile=dict(where, n=host.shape[0]))


def small():
    return _scene(orc.LidarGeom(**SMALL), 1)


def round2():
    return _scene(orc.LidarGeom(**ROUND2), 2)


def example():
    """The example sweep, 64 x 2000: [its rows, empty, every third row of it]."""
    g = orc.LidarGeom(**orc.GEOMS["Velodyne64E"])
    xyz = np.load(os.path.join(GOLDEN, "example_64E.npz"))["xyz"]
    rows = np.concatenate([xyz, np.zeros((xyz.shape[0], 1), np.float32)], 1).astype(np.float32)
    return dict(g=g, frames=[rows, np.zeros((0, 4), np.float32), np.ascontiguousarray(rows[::3])], pad=None, hostile=None)


PAST_GEOM = dict(H=16, W=512, hfov_deg=360, vmax_deg=2.0, vmin_deg=-24.9)


def past_the_grid():
    """The smallest batch of [cloud, cloud', empty] frames in a cycle at 16 x 512 whose B * P pixels take workgroup 0 of subpixel_code_kernel through
    a second trip (sized from tests/subpixel_grid_caps.py).  Besides g / frames: distinct, which."""
    import subpixel_grid_caps as GC
    g, rng = orc.LidarGeom(**PAST_GEOM), np.random.default_rng(5)
    P = g.H * g.W
    distinct = [np.ascontiguousarray(IC.cloud(g, 3000, rng), dtype=np.float32), np.ascontiguousarray(IC.cloud(g, 1501, rng), dtype=np.float32),
                np.zeros((0, 4), np.float32)]
    B = GC.SUB_CODE_CAP * GC.SUB_THREADS // P + 1
    which = np.arange(B) % 3
    return dict(g=g, frames=[distinct[k] for k in which], pad=None, hostile=None, distinct=distinct, which=which)


CASES = dict(small=small, round2=round2, example=example, past_the_grid=past_the_grid)
offsets = IC.offsets

"""Generators of the cases that take the radius outlier removal (librpcc_filter.so) through partial tiles and frame borders, onto
the keep threshold and the edges of its comparisons, past one round of its tile list and over non-finite points (numpy only).
Every generator returns its inputs and a dict of the facts it claims about itself; tests/test_filter_cases.py asserts those facts
on the CPU, so a case cannot silently stop exercising what it is for, and tests/test_gpu_radius_filter.py runs the cases on the
device.

A case is (xyz f32 [total,3] or [total,4], offsets i64 [B+1], nb_points, radius), facts."""
import os

import numpy as np

import radius_filter_ref as R
from tile_cases import _step, box_bound, d2f, screen_bounds  # noqa: F401 (box_bound: for the tests)

F32 = np.float32
TILE, TILE_LIST = 256, 256      # RPCC_FILTER_TILE, RPCC_FILTER_TILE_LIST (include/rpcc_filter.h)
HERE = os.path.dirname(os.path.abspath(__file__))


def offsets_of(sizes):
    o = np.zeros(len(sizes) + 1, np.int64)
    o[1:] = np.cumsum(sizes)
    return o


def tile_of(offsets):
    """int [total]: the tile of every point as the library cuts them (256 consecutive points of one frame), and the tile count."""
    out, t = [], 0
    for b in range(len(offsets) - 1):
        n = int(offsets[b + 1] - offsets[b])
        out.append(t + np.arange(n) // TILE)
        t += -(-n // TILE)
    return (np.concatenate(out) if out else np.zeros(0, np.int64)), t


def tile_boxes(xyz, offsets):
    """(lo, hi f32 [T,3], finite points [T]) per tile over its FINITE points; a tile without one gets lo = +inf, hi = -inf."""
    tile, T = tile_of(offsets)
    p = np.asarray(xyz, F32)[:, :3]
    fin = np.isfinite(p).all(1)
    lo, hi = np.full((T, 3), np.inf, F32), np.full((T, 3), -np.inf, F32)
    np.minimum.at(lo, tile[fin], p[fin])
    np.maximum.at(hi, tile[fin], p[fin])
    return lo, hi, np.bincount(tile[fin], minlength=T)


def blob_cloud(n, seed, spread=None):
    """n points: nine tenths in Gaussian blobs (sigma 0.5 m), one tenth uniform over the scene, in random list order.  The scene grows
    with n, so at (3, 1.0) some points are kept and some removed at every size."""
    rng = np.random.default_rng(seed)
    blobs = max(1, n // 40)
    L = spread if spread is not None else 3.0 * blobs ** (1.0 / 3.0) + 2.0
    c = rng.uniform(-L, L, (blobs, 3))
    p = c[rng.integers(0, blobs, n)] + rng.normal(0, 0.5, (n, 3))
    m = n // 10
    p[:m] = rng.uniform(-2 * L, 2 * L, (m, 3))
    return p[rng.permutation(n)].astype(F32)


# ------------------------------------------------------------------------------------------------
# frame sizes
# ------------------------------------------------------------------------------------------------
FRAME_SIZES = (1, 255, 256, 257, 513)
BATCH_SIZES = (300, 0, 257, 1)


def single_frame(n, seed=3):
    xyz = blob_cloud(n, seed + n)
    return (xyz, offsets_of([n]), 3, 1.0), dict(n=n, tiles=-(-n // TILE), partial=n % TILE != 0)


def mixed_batch(seed=11):
    """Frames of 300, 0, 257 and 1 points over the same scene: an empty frame, and tiles that would straddle two frames if the list were
    cut every 256 points globally (300 and 557 are no multiples of 256).  The frames overlap in space, so a search that ran over the
    frame borders would count more."""
    frames = [blob_cloud(n, seed + i, spread=4.0) if n else np.zeros((0, 3), F32) for i, n in enumerate(BATCH_SIZES)]
    offsets = offsets_of(BATCH_SIZES)
    return (np.concatenate(frames), offsets, 3, 1.0), dict(sizes=BATCH_SIZES, tiles=tile_of(offsets)[1])


def twin_frames(nb_points=3, radius=1.0):
    """Two frames whose last and first points coincide: frame 0 ends with nb_points copies of p, frame 1 starts with one more.  In one
    list the copies would have nb_points + 1 neighbours and be kept; frame by frame all of them are removed.  Both frames also hold a
    kept group far away."""
    p = np.array([5.0, 5.0, 1.0], F32)
    far = np.tile(np.array([-20.0, 0.0, 0.0], F32), (nb_points + 1, 1))
    f0 = np.concatenate([far, np.tile(p, (nb_points, 1))])
    f1 = np.concatenate([p[None], far + F32(1.5)])
    offsets = offsets_of([len(f0), len(f1)])
    twins = np.arange(len(f0) - nb_points, len(f0) + 1)
    return (np.concatenate([f0, f1]), offsets, nb_points, radius), dict(twins=twins)


# ------------------------------------------------------------------------------------------------
# the keep threshold
# ------------------------------------------------------------------------------------------------
THRESHOLD_NB = (0, 1, 3, 50)
THRESHOLD_N = 900     # four tiles, the last partial


def threshold_groups(nb_points, radius=1.0, seed=17):
    """One frame of THRESHOLD_N points: isolated filler points 10 radii apart, and groups 20 radii apart whose members lie within
    0.2 radius of their centre per axis (all within the radius of each other): one of nb_points members (removed; none for nb_points = 0), one
    of nb_points + 1 (kept), one of 60 exact duplicates (kept while nb_points < 60), and one of max(nb_points + 1, 3) members spread over three
    different tiles (kept only when the search leaves its own tile).  -> case, facts with the groups' list positions."""
    rng = np.random.default_rng(seed + nb_points)
    n = THRESHOLD_N
    sizes = dict(below=nb_points, at=nb_points + 1, dup=60, spread=max(nb_points + 1, 3))
    xyz = np.zeros((n, 3), F32)
    k = np.arange(n)
    xyz[:, 0] = (k % 30) * 10.0 * radius          # filler lattice, z = 0
    xyz[:, 1] = (k // 30) * 10.0 * radius
    free = rng.permutation(n)
    groups, used = {}, 0
    for gi, (name, m) in enumerate(sizes.items()):
        centre = np.array([20.0 * radius * gi, -30.0 * radius, 5.0 * radius])
        if name == "spread":      # members in tiles 0, 1 and 3 (the partial one), round robin
            pools = [np.setdiff1d(np.arange(lo, hi), free[:used + sizes["below"] + sizes["at"] + sizes["dup"]])
                     for lo, hi in ((0, 256), (256, 512), (768, n))]
            pos = np.array([pools[i % 3][i // 3] for i in range(m)])
        else:
            pos = free[used:used + m]
            used += m
        pts = centre + (0 if name == "dup" else rng.uniform(-0.2, 0.2, (m, 3)) * radius)
        xyz[pos] = pts.astype(F32)
        groups[name] = pos
    return (xyz, offsets_of([n]), nb_points, radius), dict(groups=groups, sizes=sizes, spread_tiles=sorted(set((groups["spread"] // TILE).tolist())))


# ------------------------------------------------------------------------------------------------
# the boundary and the screen: partners a few fp32 ulps either side of the radius
# ------------------------------------------------------------------------------------------------
BAND_RADII = (0.05, 0.45, 1.0, 6.0)
BAND_STEPS = (-3, -2, -1, 0, 1, 2, 3)


def band_pairs(radius, nb_points=3, seed=31):
    """One group per stepped axis (x, y, z) and step: nb_points copies of a point p and one partner p + radius * e_k whose stepped
    coordinate is moved by -3 ... +3 fp32 ulps, so the partner decides whether the copies are kept (nb_points + 1 neighbours) or removed.
    p[k] = float32(-0.5 * radius), so the partner sits near +0.5 radius, one ulp of its coordinate is at most 2^-24 of the radius and three of
    them move d^2 by less than the screen's half width of 8 * 2^-24 r^2: every pair lies strictly inside the band; the other coordinates
    of p and its partner are equal.  Groups are 4 radii apart.  Where float32(radius) == radius (1.0, 6.0) the unmoved partner sits at
    d^2 == r^2 exactly: the pair planted at equality (not a neighbour, the rule is strict).  List positions are random over 600 points
    (three tiles), the rest being isolated filler, so a point and its partner usually sit in different tiles.
    -> case, facts: per group 'p', 'q', 'copies', 'partner' (list positions), 'd2f', 'in_band' (strictly between the screen's lo and hi),
    'd2', 'neighbour' (the fp64 rule), 'fp32_neighbour' (d2f < float32(r^2)), 'planted' (d2 == r^2)."""
    rng = np.random.default_rng(seed)
    radius = float(radius)
    r2 = radius * radius
    lo, hi = screen_bounds(radius)
    n = 600
    xyz = np.zeros((n, 3), F32)
    k = np.arange(n)
    xyz[:, 0] = -(10.0 + (k % 25) * 10.0) * radius      # filler: x < 0, the groups have x >= 0
    xyz[:, 1] = (k // 25) * 10.0 * radius
    groups = []
    pos = rng.choice(n, 3 * len(BAND_STEPS) * (nb_points + 1), replace=False).reshape(-1, nb_points + 1)
    for g in range(3 * len(BAND_STEPS)):
        axis, step = g // len(BAND_STEPS), BAND_STEPS[g % len(BAND_STEPS)]
        p = np.zeros(3, F32)
        p[(axis + 1) % 3] = F32(4.0 * radius * (g + 1))
        p[axis] = F32(-0.5 * radius)
        q = p.copy()
        q[axis] = _step(F32(float(p[axis]) + radius), step)
        xyz[pos[g, :-1]] = p
        xyz[pos[g, -1]] = q
        d = float(R.d2(p.astype(np.float64), q.astype(np.float64)))
        groups.append(dict(p=p, q=q, axis=axis, step=step, copies=pos[g, :-1], partner=int(pos[g, -1]), d2f=d2f(p, q),
                           in_band=bool(lo < d2f(p, q) < hi), d2=d, neighbour=bool(d < r2), fp32_neighbour=bool(d2f(p, q) < F32(r2)),
                           planted=bool(d == r2)))
    return (xyz, offsets_of([n]), nb_points, radius), dict(radius=radius, lo=lo, hi=hi, groups=groups, exact_planted=float(F32(radius)) == radius)


def band_expected(case, facts):
    """keep of the frame of band_pairs by the specification, from the facts alone: copies are kept when their partner is a neighbour
    (nb_points copies + the partner > nb_points); partners (nb_points + 1 neighbours when the copies count, else 1) likewise; filler is
    removed."""
    xyz, _, nb_points, _ = case
    keep = np.zeros(xyz.shape[0], bool)
    for g in facts["groups"]:
        keep[g["copies"]] = g["neighbour"] and nb_points >= 1
        keep[g["partner"]] = g["neighbour"] and nb_points >= 1
    if nb_points == 0:
        keep[:] = True
    return keep


# ------------------------------------------------------------------------------------------------
# far tiles: more tiles than one round of the candidate list holds
# ------------------------------------------------------------------------------------------------
FAR_TILES = TILE_LIST + 2                 # 258 tiles: the second round holds the last full tile and the partial one
FAR_N = (FAR_TILES - 1) * TILE + 100
FAR_OUTLIER = np.array([0.0, 0.0, 1.0], F32)
FAR_LONER = np.array([10.0, 10.0, 1.0], F32)


def far_tiles(nb_points=3, radius=1.0, seed=43):
    """One frame of FAR_N points in random list order: about 20 points per cubic metre over 40 x 40 x 2 m, so every tile's box spans the
    scene -- every tile passes the box filter of every query, and the first round of the list is full.  Two holes of 2.5 m are cut:
    FAR_OUTLIER sits alone in one (list position 300: removed, after its workgroup has been through every tile), and in the other
    nb_points copies of FAR_LONER at the list positions 0 .. nb_points - 1 with ONE more copy at the last list position, in the last,
    partial tile, which only the second round of the list reaches: without it the copies have nb_points neighbours and are removed."""
    rng = np.random.default_rng(seed)
    n = FAR_N
    p = np.empty((0, 3))
    while p.shape[0] < n:
        c = rng.uniform((-20, -20, 0), (20, 20, 2), (n, 3))
        ok = (np.linalg.norm(c - FAR_OUTLIER, axis=1) > 2.5) & (np.linalg.norm(c - FAR_LONER, axis=1) > 2.5)
        p = np.concatenate([p, c[ok]])
    xyz = p[:n].astype(F32)
    loners = np.array(list(range(nb_points)) + [n - 1])
    xyz[loners] = FAR_LONER
    xyz[300] = FAR_OUTLIER
    return (xyz, offsets_of([n]), nb_points, radius), dict(n=n, tiles=FAR_TILES, loners=loners, outlier=300)


# ------------------------------------------------------------------------------------------------
# non-finite points
# ------------------------------------------------------------------------------------------------
BAD_VALUES = (np.nan, np.inf, -np.inf)


def nonfinite(nb_points=3, radius=1.0):
    """One tile of stored rows (x, y, z, intensity).  Group A: nb_points finite copies of a point, and around them nine points that have
    NaN, +Inf or -Inf in one coordinate and the group's values in the others: were a bad point counted, or its finite coordinates, A
    would be kept.  Group B: nb_points + 1 finite copies, two of them with NaN intensity (kept: the fourth float is never interpreted).
    Isolated filler between them.  -> case with [N,4] rows, facts."""
    a, b = np.array([3.0, 4.0, 1.0], F32), np.array([-8.0, 2.0, 0.5], F32)
    rows = []
    for i in range(40):
        rows.append([50.0 + 10.0 * i, 0.0, 0.0, 0.1 * i])
    A = list(range(len(rows), len(rows) + nb_points))
    rows += [[*a, 0.5]] * nb_points
    bad = []
    for axis in range(3):
        for v in BAD_VALUES:
            r = [*a, 0.25]
            r[axis] = v
            bad.append(len(rows))
            rows.append(r)
    Bg = list(range(len(rows), len(rows) + nb_points + 1))
    rows += [[*b, np.nan], [*b, np.nan]] + [[*b, 0.75]] * (nb_points - 1)
    xyz = np.array(rows, F32)
    perm = np.random.default_rng(5).permutation(len(rows))      # bad points among the finite ones
    inv = np.argsort(perm)
    return (xyz[perm], offsets_of([len(rows)]), nb_points, radius), dict(A=inv[A], B=inv[Bg], bad=inv[bad])


# ------------------------------------------------------------------------------------------------
# the example sweep and its slices
# ------------------------------------------------------------------------------------------------
def example_sweep():
    return np.load(os.path.join(HERE, "golden", "example_64E.npz"))["xyz"].astype(F32)


def sweep_slices():
    """{'columns': the points of a 128-column sector of the 64 x 2000 range image, 'beams': the points of two adjacent beams}, in stored
    order -- a few thousand points each, picked by azimuth and elevation of the points (the projection's rounding does not matter here)."""
    xyz = example_sweep()
    az = np.mod(np.arctan2(xyz[:, 1].astype(np.float64), xyz[:, 0]), 2 * np.pi)
    el = np.arctan2(xyz[:, 2].astype(np.float64), np.hypot(xyz[:, 0].astype(np.float64), xyz[:, 1]))
    col = az / (2 * np.pi) * 2000
    row = (el - np.deg2rad(-24.9)) / np.deg2rad(26.9) * 63
    return {"columns": xyz[(col >= 900) & (col < 1028)], "beams": xyz[(row >= 29.5) & (row < 31.5)]}


def ordered_and_shuffled(xyz, seed=7):
    """-> (stored-order case, shuffled case, perm): shuffled xyz = xyz[perm]."""
    perm = np.random.default_rng(seed).permutation(xyz.shape[0])
    o = offsets_of([xyz.shape[0]])
    return (xyz, o, 3, 1.0), (xyz[perm], o, 3, 1.0), perm


def golden():
    z = np.load(os.path.join(HERE, "golden", "radius_filter_example_64E.npz"))
    n = int(z["n"])
    return dict(keep=np.unpackbits(z["keep_bits"])[:n].astype(bool), removed=z["removed"], n=n, boundary_pairs=z["boundary_pairs"])


"""numpy reference of the radius outlier removal (include/rpcc_filter.h): the one statement of the
specification the tests compare with.  Its search is not the library's: the points are bucketed in a grid and every point is
compared, in fp64, with the points of its own and the 26 adjacent buckets.

Rules: the input is narrowed to float32 first; q is a neighbour of p when ((dx*dx) + (dy*dy)) + (dz*dz) < radius*radius in fp64,
un-fused, dx = double(xp) - double(xq) (strict; the point itself counts; duplicates are ordinary points); a point is kept when
its count is > nb_points; a point with a non-finite coordinate is removed and is nobody's neighbour; frames never see each other.

The buckets have side radius * (1 + 2^-20), a hair more than the radius: two neighbours differ by at most radius * (1 + 2^-50)
per axis (the fp64 test rounds), so their quotients by the side differ by less than 1 - 2^-21 in real numbers, the two rounded
divisions move them by 2^-34 at most below the clip, and their floors differ by at most one.  Bucket numbers are clipped at
+-2^19, which is monotone and only ever merges buckets."""
import numpy as np

LIM = 1 << 19
K = 2 * LIM + 3
PAIRS_PER_CHUNK = 1 << 22


def narrow(xyz):
    return np.ascontiguousarray(np.asarray(xyz)[:, :3], dtype=np.float32)


def d2(p, q):
    """The specification's squared distance of fp64 arrays [...,3]."""
    dx, dy, dz = p[..., 0] - q[..., 0], p[..., 1] - q[..., 1], p[..., 2] - q[..., 2]
    return ((dx * dx) + (dy * dy)) + (dz * dz)


def _buckets(p, radius):
    """p f64 [n,3], finite -> (order, key, P, ukey, start, num): the points in bucket order (stable: list order inside a bucket), their
    bucket keys, and the first point and size of every occupied bucket."""
    side = float(radius) * (1.0 + 2.0 ** -20)
    c = np.clip(np.floor(p / side), -LIM, LIM).astype(np.int64) + (LIM + 1)      # 1 .. 2 LIM + 1: a neighbour bucket never wraps
    key = (c[:, 0] * K + c[:, 1]) * K + c[:, 2]
    order = np.argsort(key, kind="stable")
    key = key[order]
    ukey, start, num = np.unique(key, return_index=True, return_counts=True)
    return order, key, p[order], ukey, start, num


OFFSETS = sorted(((dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)), key=lambda o: sum(abs(v) for v in o))   # own bucket first


def _neighbour_bucket(key, ukey, start, num, off):
    """(first point, size) of the bucket at offset off from every key; size 0 where it is not occupied."""
    nk = key + ((off[0] * K + off[1]) * K + off[2])
    j = np.minimum(np.searchsorted(ukey, nk), ukey.size - 1)
    return start[j], np.where(ukey[j] == nk, num[j], 0)


def _pairs(P, q, s, m):
    """Yields (lo, hi, qi, ci, d): for the queries q[lo:hi] (positions in P) the fp64 d^2 of query q[lo + qi] to candidate ci, over the
    candidates s[i] .. s[i] + m[i] - 1 of every query i, in chunks of about PAIRS_PER_CHUNK pairs."""
    cum = np.cumsum(m)
    a = 0
    while a < q.size:
        b = max(a + 1, int(np.searchsorted(cum, cum[a] - m[a] + PAIRS_PER_CHUNK, side="right")))
        reps = m[a:b]
        tot = int(reps.sum())
        if tot:
            qi = np.repeat(np.arange(b - a), reps)
            ci = np.repeat(s[a:b] - (np.cumsum(reps) - reps), reps) + np.arange(tot)
            yield a, b, qi, ci, d2(P[q[a + qi]], P[ci])
        a = b


CAP_SLICE = 32   # candidates per query and step when the counts are capped: most points of a dense bucket are done after the first


def frame_counts(xyz, radius, cap=None):
    """int64 [N]: the neighbours of every point of ONE frame, itself included; 0 for a non-finite point.  cap: the counts are only
    needed up to cap (values >= cap mean "cap or more"): a point that has reached it is not looked at again, which is what keeps a
    whole sweep cheap."""
    p = narrow(xyz).astype(np.float64)
    out = np.zeros(p.shape[0], np.int64)
    idx = np.nonzero(np.isfinite(p).all(1))[0]
    if idx.size == 0:
        return out
    r2 = float(radius) * float(radius)
    order, key, P, ukey, start, num = _buckets(p[idx], radius)
    cnt = np.zeros(idx.size, np.int64)
    for off in OFFSETS:
        q = np.arange(idx.size) if cap is None else np.nonzero(cnt < cap)[0]
        s, m = _neighbour_bucket(key[q], ukey, start, num, off)
        while q.size:
            take = m if cap is None else np.minimum(m, CAP_SLICE)
            for lo, hi, qi, _, d in _pairs(P, q, s, take):
                cnt[q[lo:hi]] += np.bincount(qi, weights=d < r2, minlength=hi - lo).astype(np.int64)
            if cap is None:
                break
            s, m = s + take, m - take
            go = (m > 0) & (cnt[q] < cap)
            q, s, m = q[go], s[go], m[go]
    out[idx[order]] = cnt
    return out


def counts(xyz, offsets, radius, cap=None):
    """int64 [total]: frame_counts per frame of the batch (offsets [B+1])."""
    xyz = narrow(xyz)
    out = np.zeros(xyz.shape[0], np.int64)
    for b in range(len(offsets) - 1):
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        out[lo:hi] = frame_counts(xyz[lo:hi], radius, cap)
    return out


def radius_filter(xyz, offsets=None, nb_points=3, radius=1.0, full=False):
    """-> dict(keep bool [total], count int32 [total] clipped at nb_points + 1, kept int64 [B], index int64: positions of the kept points;
    full=True adds 'full', the unclipped counts, which costs every pair of adjacent buckets)."""
    xyz = narrow(xyz)
    if offsets is None:
        offsets = np.array([0, xyz.shape[0]], np.int64)
    offsets = np.asarray(offsets, np.int64)
    c = counts(xyz, offsets, radius, None if full else nb_points + 1)
    keep = c > nb_points
    kept = np.array([int(keep[offsets[b]:offsets[b + 1]].sum()) for b in range(len(offsets) - 1)], np.int64)
    out = dict(keep=keep, count=np.minimum(c, nb_points + 1).astype(np.int32), kept=kept, index=np.nonzero(keep)[0].astype(np.int64))
    if full:
        out["full"] = c
    return out


def masked(xyz, keep):
    """The library's masked output for float32 [N,3] or [N,4] rows: x, y, z of every removed point quiet NaN, a fourth column untouched."""
    out = np.array(xyz, np.float32, copy=True)
    out[~np.asarray(keep, bool), :3] = np.float32(np.nan)
    return out


def brute_counts(xyz, radius):
    """frame_counts by the dense distance matrix (small frames only): the check of the grid search itself."""
    p = narrow(xyz).astype(np.float64)
    assert p.shape[0] <= 6000
    fin = np.isfinite(p).all(1)
    q = np.where(fin[:, None], p, 0.0)
    nb = (d2(q[:, None], q[None]) < float(radius) * float(radius)) & fin[:, None] & fin[None]
    return nb.sum(1).astype(np.int64)


def near_boundary(xyz, radius, ulps=4):
    """int64 [n,2]: the unordered pairs (positions in the list, i < j) of one frame whose fp64 d^2 lies within `ulps` fp64 ulps of
    radius^2 (d^2 == r^2 included): the pairs a search with another boundary rule (cKDTree: <=) or another rounding may decide the other
    way.  Every pair of adjacent buckets is looked at."""
    p = narrow(xyz).astype(np.float64)
    idx = np.nonzero(np.isfinite(p).all(1))[0]
    r2 = float(radius) * float(radius)
    lo, hi = r2, r2
    for _ in range(ulps):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
    found = [np.zeros((0, 2), np.int64)]
    if idx.size:
        order, key, P, ukey, start, num = _buckets(p[idx], radius)
        q = np.arange(idx.size)
        for off in OFFSETS:
            s, m = _neighbour_bucket(key, ukey, start, num, off)
            for a, _, qi, ci, d in _pairs(P, q, s, m):
                hit = np.nonzero((d >= lo) & (d <= hi))[0]
                found.append(np.stack([idx[order[a + qi[hit]]], idx[order[ci[hit]]]], 1))
    pairs = np.concatenate(found)
    return np.unique(pairs[pairs[:, 0] < pairs[:, 1]], axis=0)

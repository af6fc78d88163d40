"""The scenes of tests/test_gpu_assign_sums.py (numpy and the CPU oracle only; tests/test_assign_sums_cases.py asserts without a GPU that
every scene holds what its case is there for).

The fused batch adds the point model's range sums in assign_kernel (one round of a wavefront per distinct cluster label of its 8 x 32
tile) and counts the labels in the count-only form of model_hist_kernel.  What can go wrong there is a matter of which labels and
ranges a TILE holds, so the scenes are range images written pixel by pixel and turned into one point per pixel, on the pixel's own ray:
the projection (nearest pixel by rounding) puts every point back where it came from.

Every frame has an injected ground plane (z = -1.7 m).  The oracle runs once per (shape, scene, cluster count); the results are
shared and never written to."""
import functools
import math

import numpy as np

VMAX_DEG, VMIN_DEG = 3.0, -25.0
GROUND = np.array([0.0, 0.0, -1.0, -1.7])          # a x + b y + c z + d = 0: the plane z = -1.7
NAN_ROW = 0xFFC00000                               # the mean of a label without pixels (x86's default NaN of 0.0 / 0)
WINDOW_LO, WINDOW_HI = 0.03125, 256.0              # the fixed-point window [2^-5, 2^8) of the range sums
TILE_ROWS, TILE_COLS = 8, 32                       # assign_kernel's tile


def geom_of(H, W):
    from oracle import oracle as orc
    return orc.LidarGeom(H, W, 360.0, VMAX_DEG, VMIN_DEG)


@functools.lru_cache(maxsize=8)
def shape(H, W):
    """(oracle geometry, transform map) of an H x W image."""
    from oracle import oracle as orc
    g = geom_of(H, W)
    return g, orc.transform_map(g)


def rays(H, W):
    """Unit vectors of the pixel centres, float64 [H,W,3] (the angles of the transform map)."""
    g = geom_of(H, W)
    el = np.array([g.vertical_FOV * (h / (H - 1)) + g.vertical_min for h in range(H)])
    az = np.array([g.horizontal_FOV * (w / W) for w in range(W)])
    return np.stack([np.cos(el)[:, None] * np.cos(az)[None, :], np.cos(el)[:, None] * np.sin(az)[None, :],
                     np.repeat(np.sin(el)[:, None], W, 1)], -1)


def points_of(image):
    """One point per non-empty pixel of a range image (float64 [H,W], 0 = empty), on the pixel's ray: float32 [N,3], row-major."""
    H, W = image.shape
    keep = image != 0
    return np.ascontiguousarray((image[..., None] * rays(H, W))[keep].astype(np.float32))


def ground_image(H, W):
    """The range at which every pixel's ray meets the ground plane; 0 (empty) for rays that do not, or only beyond 120 m."""
    dz = rays(H, W)[..., 2]
    with np.errstate(divide="ignore"):
        r = np.where(dz < 0, -1.7 / np.minimum(dz, -1e-12), 0.0)
    return np.where(r < 120.0, r, 0.0)


@functools.lru_cache(maxsize=16)
def synth_image(H, W, k):
    """Scene k of a shape: the synthetic sweep (ground, boxes, cylinders, empty pixels) as the range image the oracle projects it to."""
    from oracle import oracle as orc
    from rpcc_amd import synth
    f = synth.make_frame(400 + k, H, W, vmax_deg=VMAX_DEG, vmin_deg=VMIN_DEG).numpy()
    return orc.project(f, geom_of(H, W)).astype(np.float64)


def window_image(H, W, k):
    """Scene k with cluster pixels outside the fixed-point window: a run of returns at 0.02 m (below 2^-5; next to the sensor, far above
    the ground) in row 1 and a run at 300 .. 330 m (at or above 2^8) in the top row, both inside one tile column and away from column 0."""
    im = synth_image(H, W, k).copy()
    im[1, 36:41] = 0.02
    im[H - 1, 40:44] = 300.0 + 10.0 * np.arange(4)
    return im


def packed_image(H, W, f0=0.20, df=0.04):
    """Flat ground and, in the tile of rows 0 .. 7 and columns 32 .. 63, sixteen blocks of 2 x 8 pixels at sixteen heights above the
    ground (ranges f0, f0 + df, ... of the ground's along the same ray): every non-ground return of the frame lies in that one tile, so
    the FPS packs its centres into it."""
    im = ground_image(H, W)
    for bi in range(4):
        for bj in range(4):
            im[2 * bi:2 * bi + 2, 32 + 8 * bj:40 + 8 * bj] *= f0 + df * (bi * 4 + bj)
    return im


def hollow_image(H, W):
    """packed_image with the blocks farther out (0.50 .. 0.80 of the ground's range) and pixel 0 empty.  Empty pixels are points at the
    origin and count as non-ground (utils/segment_utils.py:119-127), so the FPS starts at pixel 0 and its first centre is the origin; every
    return of the frame is nearer to a block's centre or to the ground: the first cluster label owns no pixel."""
    im = packed_image(H, W, 0.50, 0.02)
    im[0, 0] = 0.0
    return im


# ------------------------------------------------------------------------------------------------
# the cases: name -> (H, W, cluster count, frames as (kind, scene number))
# ------------------------------------------------------------------------------------------------
CASES = {
    # H % 8 != 0, W % 32 != 0 (partial tiles, a padding wavefront in the last workgroup: 6 tiles of 4 per workgroup), P = 864 < 1024
    "ragged": (12, 72, 6, (("synth", 0), ("synth", 1), ("synth", 2))),
    "vector": (16, 2048, 20, (("synth", 0), ("synth", 1))),                  # whole tiles, 32 scatter tiles per frame, 4-pixel label loads
    "w2250": (8, 2250, 20, (("synth", 0), ("synth", 1))),                    # W % 32 != 0 on one tile row, P = 18000
    "scalar": (7, 301, 9, (("synth", 0), ("synth", 1))),                     # P % 4 != 0: the element-wise form of the histogram
    "window": (12, 72, 6, (("synth", 0), ("window", 1), ("synth", 2))),      # the middle frame leaves the fixed-point window
    # > 3 cluster labels in one tile; in the second frame also a cluster label without pixels
    "packed": (16, 96, 12, (("packed", 0), ("hollow", 0), ("synth", 0))),
    "uint16": (16, 2048, 300, (("synth", 0), ("synth", 1))),                 # uint16 labels (assign_kernel<uint16_t, 8>)
    # workspace reuse: the second call of the pair, on the first one's workspace ("window" first: its flag and sums must not stay)
    "reuse": (12, 72, 6, (("synth", 3), ("synth", 4), ("synth", 0))),
}
# one rpcc_compress_batch_mixed: two geometry groups with one cluster count; the second group takes the element-wise histogram form
MIXED = (("window", 12, 72), ("mixed-scalar", 7, 301))
CASES["mixed-scalar"] = (7, 301, 6, (("synth", 0), ("synth", 1)))
PACKED_TILE = (slice(0, 8), slice(32, 64))


def image_of(kind, H, W, k):
    return {"synth": lambda: synth_image(H, W, k), "window": lambda: window_image(H, W, k), "packed": lambda: packed_image(H, W),
            "hollow": lambda: hollow_image(H, W)}[kind]()


@functools.lru_cache(maxsize=32)
def frame(kind, H, W, k):
    """The points of a frame: float32 [N,3]."""
    return points_of(image_of(kind, H, W, k))


@functools.lru_cache(maxsize=32)
def expected(kind, H, W, k, M):
    """The oracle on a frame: range image, labels, counts, model rows (float32 [K,4]), quantised integers, and the reference's own
    sequential float64 range sums per label (what the rows must equal where the fixed-point sums do not apply)."""
    from oracle import oracle as orc
    g, tm = shape(H, W)
    o = orc.compress_frame(frame(kind, H, W, k), g, tm, GROUND, dict(orc.DEFAULT_CFG, cluster_num=M))
    assert len(set(o["fps_pix"].tolist())) == M, (kind, H, W, k, "the frame must hold M distinct centres")
    seg = o["seg_idx"].astype(np.int64)
    return dict(ri=o["range_image"], seg=seg, counts=np.bincount(seg.reshape(-1), minlength=M + 2).astype(np.int32),
                model=np.asarray(o["model_param"]).astype(np.float32), q=o["q"].astype(np.int16), pix=o["fps_pix"],
                cen=o["centers"].astype(np.float32))


def case_expected(name):
    H, W, M, frames = CASES[name]
    return [expected(kind, H, W, k, M) for kind, k in frames]


def case_frames(name):
    H, W, M, frames = CASES[name]
    return [frame(kind, H, W, k) for kind, k in frames]


def outside_window(e):
    """Cluster pixels (label >= 2) of an oracle result whose range lies outside the fixed-point window -> (below, at or above)."""
    r, c = e["ri"].reshape(-1), e["seg"].reshape(-1) >= 2
    return int((c & (r < WINDOW_LO)).sum()), int((c & (r >= WINDOW_HI)).sum())


def tile_cluster_labels(e, rows, cols):
    """The distinct cluster labels of a block of the label image."""
    t = e["seg"][rows, cols]
    return sorted(set(t[t >= 2].tolist()))


def empty_labels(e):
    """Cluster labels that own no pixel."""
    return [k for k in range(2, e["counts"].shape[0]) if e["counts"][k] == 0]


def sequential_mean(e, k):
    """float32(sum of label k's ranges in row-major order in float64 / count): cpp_modules.cpp:514."""
    s = 0.0
    for v in e["ri"].reshape(-1)[e["seg"].reshape(-1) == k]:
        s += float(v)
    return np.float32(s / float(e["counts"][k]))


def kpad(M):
    """Labels per row of the workspace's sums block (kpad, rpcc_hip.hip): M + 2 rounded up to 64."""
    return (M + 2 + 63) // 64 * 64


assert math.isclose(WINDOW_LO, 2.0 ** -5)

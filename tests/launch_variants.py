"""The launch rules of r-pcc_amd/csrc/rpcc_hip.hip restated in Python, and the tables of small cases that take every kernel variant those
rules can pick (numpy only; tests/test_launch_variants.py asserts on the CPU that the tables reach every variant, and
tests/test_gpu_launch_variants.py runs them on the device).

The launch code does not pick one kernel per stage but one template instantiation, by quantities the rest of the suite hardly varies
together: the frames that share a launch, the FPS tile count, the width modulo four, the alignment of the caller's arrays, whether the
planar ray table exists, the length of a key-point chunk, the label type.  Every constant of the rules is read from the sources by
regular expression at import (a changed constant moves the tables' expectations, one that is no longer found raises here); the rules
themselves cite the lines they restate.  Every case carries the pick it is in the table for, written out next to it."""
import functools
import os
import re
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "r-pcc_amd", "csrc")


# ------------------------------------------------------------------------------------------------
# constants, from the sources
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _find(name, pattern, what):
    m = re.search(pattern, _text(name), re.M)
    if m is None:
        raise AssertionError("tests/launch_variants.py: %s is no longer found in r-pcc_amd/csrc/%s (pattern %r): restate the rule" % (what, name, pattern))
    return m


def _define(name, macro):
    return int(_find(name, r"^#define[ \t]+%s[ \t]+\(?(-?\d+)\)?" % macro, "#define " + macro).group(1))


FPS_TILE = _define("fps_kernels.h", "FPS_TILE")                        # points of a list tile
FPS_TROWS = _define("fps_kernels.h", "FPS_TROWS")                      # rows of a range-image tile (32 columns)
FPS_TILED_MAX_TILES = _define("fps_kernels.h", "FPS_TILED_MAX_TILES")  # fps_prunable
FPS_TT_SMALL = _define("fps_kernels.h", "FPS_TT_SMALL")
FPS_TT_BATCH = _define("fps_kernels.h", "FPS_TT_BATCH")
FPS_THREADS = _define("fps_kernels.h", "FPS_THREADS")
FPS_SMALL_FRAMES = int(_find("rpcc_hip.hip", r"tt = frames <= (\d+) \? FPS_TT_SMALL : FPS_TT_BATCH", "the frame count of fps_pick_pruned").group(1))
FPS_TILE_COLS = int(_find("fps_kernels.h", r"g\.tcols = \(W \+ (\d+)\) / (\d+);", "the tile width of fps_tiling_range").group(2))
FEAT_RQ = _define("feature_kernels.h", "FEAT_RQ")
FEAT_ROW_SEGS = _define("feature_kernels.h", "FEAT_ROW_SEGS")
FEAT_ROW_FLAT = _define("feature_kernels.h", "FEAT_ROW_FLAT")
FEAT_GPW = _define("feature_kernels.h", "FEAT_GPW")
FEAT_THREADS = _define("feature_kernels.h", "FEAT_THREADS")
FEAT_ROWMODE = _define("feature_kernels.h", "FEAT_ROWMODE")
_m = _find("rpcc_hip.hip", r"if \(W <= 64 \* (\d+) \* \(FEAT_THREADS / 64\)\) FEAT_LAUNCH_G\(Q_, (\d+), F_\);", "the narrow group count of FEAT_LAUNCH")
assert _m.group(1) == _m.group(2), "FEAT_LAUNCH: the width test and the template argument name different group counts"
FEAT_G_NARROW = int(_m.group(1))
FEAT_Q_STEPS = [(int(a), int(b)) for a, b in re.findall(r"else if \(need <= (\d+)\) FEAT_LAUNCH\((\d+), true\);", _text("rpcc_hip.hip"))]
assert FEAT_Q_STEPS and all(a == b for a, b in FEAT_Q_STEPS), ("the key-point ladder of launch_features is no longer found", FEAT_Q_STEPS)
_find("rpcc_hip.hip", r"else FEAT_LAUNCH\(0, true\);", "the LDS-key form of launch_features")
_m = _find("rpcc_hip.hip", r"sizeof\(L\) == 1\) assign_kernel<L, (\d+)>.*\n\s*else if \(M <= (\d+)\)\s+assign_kernel<L, (\d+)>.*\n\s*else\s+assign_kernel<L, (\d+)>",
           "the screening rounds of launch_assign")
ASSIGN_ROUNDS_U8, ASSIGN_MID_M, ASSIGN_ROUNDS_MID, ASSIGN_ROUNDS_TOP = (int(v) for v in _m.groups())
MAX_CLUSTERS = int(_find(os.path.join("..", "..", "include", "rpcc_hip.h"), r"^#define[ \t]+RPCC_MAX_CLUSTERS[ \t]+(\d+)", "RPCC_MAX_CLUSTERS").group(1))
FPS_BRUTEFORCE, FPS_MODE_BITS = 1, 2 | 4 | 8     # RPCC_FPS_BRUTEFORCE; RPCC_FPS_FMA1 | RPCC_FPS_FMA2 | RPCC_FPS_TIE_CUDA (include/rpcc_hip.h)

# the FPS families (enum FpsFamily, rpcc_hip.hip:2244)
MODES, ONE_PASS, LDS_TABLE, REG_TABLE, PLANAR, PLANAR2 = "modes", "one pass", "LDS table", "register table", "planar", "planar2"
VEC, EDGE = False, True      # third field of a pick (`unaligned`): 16-byte accesses / the EDGE (range image, register table) or element-wise form


# ------------------------------------------------------------------------------------------------
# the rules
# ------------------------------------------------------------------------------------------------
def fps_tiles_range(H, W):
    """fps_tiling_range (fps_kernels.h:44-47): tiles of FPS_TROWS rows x 32 columns."""
    return -(-H // FPS_TROWS) * -(-W // FPS_TILE_COLS)


def fps_tiles_list(N):
    """fps_tiling_list (fps_kernels.h:49-52)."""
    return -(-N // FPS_TILE)


def range_quads16(W, aligned=True):
    """range_quads16 (rpcc_hip.hip:1872-1874); aligned: ri, temp and tm all 16-byte aligned."""
    return W % 4 == 0 and aligned


def fps_pick_pruned(T, frames, quads16, planar):
    """fps_pick_pruned (rpcc_hip.hip:2247-2251) -> (family, threads, unaligned)."""
    tt = FPS_TT_SMALL if frames <= FPS_SMALL_FRAMES else FPS_TT_BATCH
    if T > (2 if planar else 1) * tt:
        f = LDS_TABLE
    elif not planar:
        f = REG_TABLE
    else:
        f = PLANAR if T <= tt else PLANAR2
    return (f, tt, not quads16)


def fps_pick_range(H, W, frames, flags=0, quads16=None, planar=True):
    """fps_pick_range (rpcc_hip.hip:2253-2258).  quads16 None: arrays as torch allocates them, so the width decides."""
    T = fps_tiles_range(H, W)
    if flags & FPS_MODE_BITS:
        return (MODES, FPS_THREADS, False)
    if (flags & FPS_BRUTEFORCE) or T > FPS_TILED_MAX_TILES:
        return (ONE_PASS, FPS_THREADS, False)
    return fps_pick_pruned(T, frames, range_quads16(W) if quads16 is None else quads16, planar)


def fps_pick_list(N, lists, aligned=True, brute=False):
    """fps_xyz_impl (rpcc_hip.hip:2294-2306): the pruned pick of the lists the probe marks coherent; the others (and every list of a
    brute-force or too long call) take the one-pass kernel."""
    T = fps_tiles_list(N)
    if brute or T > FPS_TILED_MAX_TILES:
        return (ONE_PASS, FPS_THREADS, False)
    return fps_pick_pruned(T, lists, N % 4 == 0 and aligned, False)


def fused_refuses(H, W, frames, flags=0):
    """check_batch_io (rpcc_hip.hip): the one-pass kernel reads 16 bytes at frame bases, so a frame that takes it needs P % 4 == 0."""
    return (H * W) % 4 != 0 and fps_pick_range(H, W, frames, flags, True, True)[0] == ONE_PASS


def mixed_fps_picks(groups):
    """mixed_fps (rpcc_hip.hip).  groups: [(H, W, frames, quads16)] of tile-pruned, untimed groups -> per group
    (shares the common launch, pick).  The groups whose pick for a launch of ALL the frames is the planar kernel share one
    fps_regtab_planar_multi_kernel of that thread count, each with its own EDGE flag; every other group runs alone, with the pick of its
    own frame count (run_stage's ST_FPS case, rpcc_hip.hip)."""
    total = sum(g[2] for g in groups)
    out = []
    for (H, W, frames, quads16) in groups:
        k = fps_pick_range(H, W, total, 0, quads16, True)
        out.append((True, k) if k[0] == PLANAR else (False, fps_pick_range(H, W, frames, 0, quads16, True)))
    return out


def feature_pick(W, feature_region, segments, flat_num, feat=True):
    """launch_features (rpcc_hip.hip:3443-3467) -> (Q, G, compact), or None where the entry refuses the width.  feat: a curvature image
    is wanted (the stage entries; the fused entry passes NULL)."""
    if not (1 <= feature_region <= 16 and segments >= 1 and W <= 64 * FEAT_GPW * (FEAT_THREADS // 64)):
        return None
    chunk = (W - 2 * feature_region) // segments
    rowmode = chunk <= 16 * FEAT_RQ and segments <= FEAT_ROW_SEGS and flat_num - 1 <= FEAT_ROW_FLAT
    G = FEAT_G_NARROW if W <= 64 * FEAT_G_NARROW * (FEAT_THREADS // 64) else FEAT_GPW
    if rowmode:
        return (FEAT_ROWMODE, G, not feat)
    need = (chunk + 63) // 64
    for top, q in FEAT_Q_STEPS:
        if need <= top:
            return (q, G, False)
    return (0, G, False)


def label_bytes(M):
    """ops.is_wide: byte labels up to RPCC_MAX_CLUSTERS clusters, uint16 above."""
    return 1 if M <= MAX_CLUSTERS else 2


def assign_rounds(nbytes, M):
    """launch_assign (rpcc_hip.hip:2629-2638): screening rounds of 64 centres."""
    return ASSIGN_ROUNDS_U8 if nbytes == 1 else ASSIGN_ROUNDS_MID if M <= ASSIGN_MID_M else ASSIGN_ROUNDS_TOP


# ------------------------------------------------------------------------------------------------
# scenes: synth.make_frame(300 + k, H, W, vmax 3 deg, vmin -25 deg); at most five per shape, in rotation over a batch
# ------------------------------------------------------------------------------------------------
VMAX_DEG, VMIN_DEG, SCENE0 = 3.0, -25.0, 300
_IMPORT_LOCK = threading.Lock()


def n_scenes(H, W, B):
    """Distinct scenes of a batch of B frames: five for small images, three from 60 000 pixels on (the oracle's and the generator's cost),
    never more than frames -- and never a count that makes the last frame the same scene as the first."""
    n = min(B, 5 if H * W < 60000 else 3)
    while B > 1 and (B - 1) % n == 0:
        n -= 1
    return max(n, 1)


def scene_of(i, n):
    return i % n


def row_end_columns(W):
    """The columns of a row's last quad when the width is no multiple of four (one, two or three pixels: the quad the EDGE kernels cut
    short), else the last column."""
    return list(range(W - (W % 4 or 1), W))


@functools.lru_cache(maxsize=8)
def scene_frame(H, W, k):
    """The points of scene k of shape H x W: float32 [N,3] (host).  The synthetic sweep, with the returns of the row-end columns replaced by
    far, isolated ones (112 .. 140 m along the pixel's own ray, every row another range): the FPS then takes row-end pixels as centres, so a
    kernel that mis-reads a row-end quad changes the FPS pixels, not only a value of temp that no output shows."""
    with _IMPORT_LOCK:          # (the tests call this from worker threads; the package's first import is not re-entrant)
        from rpcc_amd import synth
    f = synth.make_frame(SCENE0 + k, H, W, vmax_deg=VMAX_DEG, vmin_deg=VMIN_DEG).numpy()
    cols = row_end_columns(W)
    az = np.mod(np.arctan2(f[:, 1].astype(np.float64), f[:, 0].astype(np.float64)), 2 * np.pi) / (2 * np.pi) * W
    f = f[(az > 1.0) & (az < cols[0] - 1.0)]                # (a margin of a column on both sides, and the wrap to column 0)
    hh, cc = np.meshgrid(np.arange(H), np.asarray(cols), indexing="ij")
    el = np.radians(VMIN_DEG + (VMAX_DEG - VMIN_DEG) * hh / (H - 1))
    a = 2 * np.pi * cc / W
    r = 140.0 - 2.5 * (W - 1 - cc) - 5.0 * ((3 * hh + 2 * k) % 5)     # the last column farthest, every row another range
    far = np.stack([r * np.cos(el) * np.cos(a), r * np.cos(el) * np.sin(a), r * np.sin(el)], -1).reshape(-1, 3)
    return np.ascontiguousarray(np.concatenate([f, far.astype(np.float32)]))


def geom_of(H, W):
    from oracle import oracle as orc
    return orc.LidarGeom(H, W, 360.0, VMAX_DEG, VMIN_DEG)


@functools.lru_cache(maxsize=8)
def list_points(H, W, k, N):
    """The first N non-empty pixels, in row-major order, of scene k of shape H x W as points: float32 [N,3].  The images are wide (a row holds
    many tiles of 256 points), so consecutive points are neighbours and rpcc_fps_xyz's probe marks the list coherent."""
    from oracle import oracle as orc
    g = geom_of(H, W)
    ri = orc.project(scene_frame(H, W, k), g)
    pc = orc.backproject(ri, orc.transform_map(g)).reshape(-1, 3)
    return np.ascontiguousarray(pc[ri.reshape(-1) > 0][:N], dtype=np.float32)


PROBE_TILES = int(_find("rpcc_hip.hip", r"^#define[ \t]+FPS_PROBE_TILES[ \t]+(\d+)", "FPS_PROBE_TILES").group(1))
PROBE_CUT = float(_find("rpcc_hip.hip", r"streamed = !\(tot < ([0-9.]+)f \* \(float\)FPS_PROBE_TILES \* all\)", "the break-even of fps_list_probe_kernel").group(1))


def list_order_measure(pts):
    """fps_list_probe_kernel (rpcc_hip.hip:1993-2037): mean over PROBE_TILES sampled tiles of the squared box diagonal, over the squared
    diagonal of the sample's box.  Below PROBE_CUT the list takes the tile-pruned kernel, otherwise the one-pass kernel."""
    n = pts.shape[0]
    T = fps_tiles_list(n)
    boxes = []
    for j in range(PROBE_TILES):
        t = (j * T) // PROBE_TILES
        p = pts[np.minimum(t * FPS_TILE + np.arange(FPS_TILE), n - 1)].astype(np.float64)
        boxes.append((p.min(0), p.max(0)))
    tot = sum(((hi - lo) ** 2).sum() for lo, hi in boxes)
    lo, hi = np.min([b[0] for b in boxes], 0), np.max([b[1] for b in boxes], 0)
    return tot / (PROBE_TILES * ((hi - lo) ** 2).sum())


def default_m(H, W):
    """Centres per frame: 20; 9 for 7 x 301 and 10 for the images of about 819 200 pixels (the scenes hold that many distinct ones)."""
    return 9 if H * W < 2500 else 10 if H * W > 800000 else 20


# ------------------------------------------------------------------------------------------------
# FPS case tables.  pick = (family, threads, unaligned) written out per case; the CPU test recomputes it with the rules above.
# ------------------------------------------------------------------------------------------------
# fused entry (the planar table exists): (H, W, frames, pick)
FPS_FUSED = [
    (7, 301, 3, (PLANAR, 1024, EDGE)), (7, 301, 129, (PLANAR, 512, EDGE)),                       # 10 tiles
    (8, 512, 3, (PLANAR, 1024, VEC)), (8, 512, 129, (PLANAR, 512, VEC)),                         # 16 tiles
    (9, 8209, 3, (PLANAR, 1024, EDGE)), (9, 8209, 128, (PLANAR, 1024, EDGE)), (9, 8209, 129, (PLANAR2, 512, EDGE)),   # 514 tiles
    (9, 8212, 3, (PLANAR, 1024, VEC)), (9, 8212, 129, (PLANAR2, 512, VEC)),
    (2, 32801, 3, (PLANAR2, 1024, EDGE)), (2, 32801, 129, (LDS_TABLE, 512, EDGE)),               # 1026 tiles
    (2, 32804, 3, (PLANAR2, 1024, VEC)), (2, 32804, 129, (LDS_TABLE, 512, VEC)),
    # widths that leave a row-end quad of two or three pixels (every width above that is no multiple of four leaves one pixel)
    (8, 514, 3, (PLANAR, 1024, EDGE)), (8, 514, 129, (PLANAR, 512, EDGE)),                       # 17 tiles
    (9, 8211, 3, (PLANAR, 1024, EDGE)), (9, 8211, 129, (PLANAR2, 512, EDGE)),                    # 514 tiles
    # boundaries, one tile row
    (8, 16384, 129, (PLANAR, 512, VEC)), (8, 16385, 129, (PLANAR2, 512, EDGE)),                  # 512 / 513 tiles
    (8, 32768, 2, (PLANAR, 1024, VEC)), (8, 32769, 2, (PLANAR2, 1024, EDGE)),                    # 1024 / 1025 tiles
    (8, 32768, 129, (PLANAR2, 512, VEC)), (8, 32769, 129, (LDS_TABLE, 512, EDGE)),
    (8, 65536, 2, (PLANAR2, 1024, VEC)), (8, 65537, 2, (LDS_TABLE, 1024, EDGE)),                 # 2048 / 2049 tiles
    (8, 102400, 2, (LDS_TABLE, 1024, VEC)), (8, 102399, 2, (LDS_TABLE, 1024, EDGE)),             # 3200 tiles: the largest prunable image
    (8, 102401, 2, (ONE_PASS, FPS_THREADS, False)),                                                    # 3201 tiles
]
# more than 3200 tiles and an odd pixel count: check_batch_io refuses it (RPCC_ERR_ARG), every output buffer stays as it was
FPS_FUSED_REFUSED = [(9, 51201, 2)]

# stage entries (rpcc_ground_mask with and without the tile table, rpcc_fps_range; no planar table): (H, W, frames, pick)
FPS_STAGE = [
    (7, 301, 3, (REG_TABLE, 1024, EDGE)), (8, 512, 3, (REG_TABLE, 1024, VEC)),
    (7, 301, 129, (REG_TABLE, 512, EDGE)), (8, 512, 129, (REG_TABLE, 512, VEC)),
    (9, 8209, 129, (LDS_TABLE, 512, EDGE)), (9, 8212, 129, (LDS_TABLE, 512, VEC)),
    (2, 32801, 2, (LDS_TABLE, 1024, EDGE)), (2, 32804, 2, (LDS_TABLE, 1024, VEC)),
    (8, 514, 3, (REG_TABLE, 1024, EDGE)), (8, 514, 129, (REG_TABLE, 512, EDGE)),                 # a row-end quad of two pixels
    # widths that are no multiple of four with a pixel count that is one: the brute-force entry takes them, so the final temp of the
    # EDGE / element forms has a witness that is not a pruned kernel
    (8, 513, 129, (REG_TABLE, 512, EDGE)),                                                       # 17 tiles
    (4, 16402, 129, (LDS_TABLE, 512, EDGE)), (2, 32802, 2, (LDS_TABLE, 1024, EDGE)),             # 513 / 1026 tiles
]

# lists (rpcc_fps_xyz): (N, lists, image (H, W) whose non-empty pixels in row-major order are the list, pick of the coherent lists).
# One list of every call is a shuffled copy, which the probe hands to the one-pass kernel.
FPS_LISTS = [
    (4000, 129, (8, 32768), (REG_TABLE, 512, VEC)), (3999, 129, (8, 32768), (REG_TABLE, 512, EDGE)),        # 16 tiles
    (131332, 129, (8, 32768), (LDS_TABLE, 512, VEC)), (131329, 129, (8, 32768), (LDS_TABLE, 512, EDGE)),    # 514 tiles
    (4000, 2, (8, 32768), (REG_TABLE, 1024, VEC)), (3999, 2, (8, 32768), (REG_TABLE, 1024, EDGE)),
    (262404, 2, (8, 65536), (LDS_TABLE, 1024, VEC)), (262401, 2, (8, 65536), (LDS_TABLE, 1024, EDGE)),      # 1026 tiles
]
LIST_M = 20

# one rpcc_compress_batch_mixed of 130 frames: (H, W, frames, shares the common launch, pick).  The first two share
# fps_regtab_planar_multi_kernel<512>, one with the EDGE flag and one without; the third would take planar2 in a launch of 130 frames, so
# it leaves the common launch and runs alone (30 frames: the 1024-thread planar kernel).  Alone, every group has at most 128 frames.
MIXED_M = 9
FPS_MIXED = [(7, 301, 60, True, (PLANAR, 512, EDGE)), (8, 512, 40, True, (PLANAR, 512, VEC)), (9, 8209, 30, False, (PLANAR, 1024, EDGE))]
# and the 1024-thread multi kernel with an EDGE and an aligned group (a mixed call of 6 frames)
FPS_MIXED_SMALL = [(7, 301, 3, True, (PLANAR, 1024, EDGE)), (8, 512, 3, True, (PLANAR, 1024, VEC))]


def fps_variants_wanted():
    """Every reachable FPS variant: ('range' | 'list' | 'multi', family, threads, unaligned) and ('range', one pass)."""
    want = {("range", f, t, u) for f in (PLANAR, PLANAR2, REG_TABLE, LDS_TABLE) for t in (FPS_TT_SMALL, FPS_TT_BATCH) for u in (VEC, EDGE)}
    want |= {("list", f, t, u) for f in (REG_TABLE, LDS_TABLE) for t in (FPS_TT_SMALL, FPS_TT_BATCH) for u in (VEC, EDGE)}
    want |= {("multi", PLANAR, t, u) for t in (FPS_TT_SMALL, FPS_TT_BATCH) for u in (VEC, EDGE)}
    want.add(("range", ONE_PASS, FPS_THREADS, False))
    return want


def fps_variants_reached():
    """What the tables reach, by the rules above (not by the picks written in the tables)."""
    got = {("range",) + fps_pick_range(H, W, B, 0, None, True) for (H, W, B, _) in FPS_FUSED}
    got |= {("range",) + fps_pick_range(H, W, B, 0, None, False) for (H, W, B, _) in FPS_STAGE}
    got |= {("list",) + fps_pick_list(N, B) for (N, B, _, _) in FPS_LISTS}
    for table in (FPS_MIXED, FPS_MIXED_SMALL):
        picks = mixed_fps_picks([(H, W, B, range_quads16(W)) for (H, W, B, _, _) in table])
        common = [k for c, k in picks if c]
        if len({k[2] for k in common}) == 2:        # an aligned and an EDGE group in the same launch
            got |= {("multi",) + k for k in common}
        got |= {("range",) + k for c, k in picks if not c}
    return got


# ------------------------------------------------------------------------------------------------
# data arrays at their natural alignment: the shapes of section 3 (8 x 512: a pixel count that is a multiple of four, only the pointer decides)
# ------------------------------------------------------------------------------------------------
ALIGN_SHAPES = [(5, 300), (8, 512)]
ALIGN_LIST_N = 3000       # points of the rpcc_fps_xyz case: a multiple of four


# ------------------------------------------------------------------------------------------------
# key-point features: the cases live in tests/feature_cases.py (no source scraping: the reference pin imports them too)
# ------------------------------------------------------------------------------------------------
from feature_cases import (ROW, FEATURE_CASES, FEATURE_REFUSED_W, FEATURE_CASES_WIDE, FEATURE_FUSED, FEATURE_CHUNK_PAIRS,  # noqa: E402,F401
                           FEATURE_PIN_DRAWS, feature_chunk, feature_image)
assert ROW == FEAT_ROWMODE, "tests/feature_cases.py writes row mode as %d, feature_kernels.h as %d" % (ROW, FEAT_ROWMODE)


def feature_variants_wanted():
    qs = [ROW] + [q for _, q in FEAT_Q_STEPS] + [0]
    want = {("u8", q, g, False) for q in qs for g in (FEAT_G_NARROW, FEAT_GPW)}
    want |= {("u16", q, FEAT_G_NARROW, False) for q in qs}
    want |= {("fused", ROW, g, True) for g in (FEAT_G_NARROW, FEAT_GPW)} | {("fused-full",)}
    return want


def feature_variants_reached(fused_widths):
    """fused_widths: lidar name -> W (oracle.GEOMS)."""
    got = {("u8",) + feature_pick(c[0], c[1], c[2], c[5]) for c in FEATURE_CASES}
    got |= {("u16",) + feature_pick(c[0], c[1], c[2], c[5]) for c in FEATURE_CASES_WIDE}
    for name, kp, _ in FEATURE_FUSED:
        k = feature_pick(fused_widths[name], kp["feature_region"], kp["segments"], kp["flat_num"], feat=False)
        got.add(("fused",) + k if k[2] else ("fused-full",))
    return got


# ------------------------------------------------------------------------------------------------
# assignment: (M, label bytes, screening rounds), all on one 16 x 1800 frame
# ------------------------------------------------------------------------------------------------
ASSIGN_SHAPE = (16, 1800)
ASSIGN_CASES = [(254, 1, 4), (255, 2, 8), (510, 2, 8), (511, 2, 16)]

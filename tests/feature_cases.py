"""The key-point cases of tests/launch_variants.py: one small image per chunk-length class of the feature kernel, width per wavefront and
class boundary, with the (Q, G) each is in the table for.  numpy only and no look at the sources, so tests/test_oracle_vs_ref.py can pin the
same settings against the reference's C++ whatever becomes of the launch constants; tests/launch_variants.py recomputes the picks."""
import numpy as np

# ------------------------------------------------------------------------------------------------
# key-point features: (W, feature_region, segments, sharp, less_sharp, flat, (Q, G)) with a curvature image, H = 4
# ------------------------------------------------------------------------------------------------
ROW = -1          # FEAT_ROWMODE (feature_kernels.h); tests/launch_variants.py asserts that they agree
FEATURE_CASES = [
    # G = 8 (W <= 2048): every class
    (1500, 3, 8, 4, 8, 6, (ROW, 8)),
    (2048, 3, 33, 2, 4, 3, (2, 8)),           # 33 segments: chunk 61
    (1030, 3, 8, 4, 8, 10, (2, 8)),           # flat_num 10: chunk 128 ...
    (1038, 3, 8, 4, 8, 10, (4, 8)),           # ... and 129
    (1030, 3, 4, 4, 8, 10, (4, 8)),           # chunk 256 ...
    (1034, 3, 4, 4, 8, 10, (6, 8)),           # ... and 257
    (1030, 3, 4, 4, 8, 6, (ROW, 8)),          # chunk 256 / 257 with the default flat_num: the end of row mode
    (1034, 3, 4, 4, 8, 6, (6, 8)),
    (1542, 3, 4, 4, 8, 6, (6, 8)),            # chunk 384 / 385
    (1546, 3, 4, 4, 8, 6, (8, 8)),
    (1030, 3, 2, 4, 8, 6, (8, 8)),            # chunk 512 / 513
    (1032, 3, 2, 4, 8, 6, (0, 8)),
    # W 2048 / 2049: G = 8 / 16 in row mode and in a register class
    (2048, 3, 8, 4, 8, 6, (ROW, 8)), (2049, 3, 8, 4, 8, 6, (ROW, 16)),
    (2048, 3, 4, 4, 8, 6, (8, 8)), (2049, 3, 4, 4, 8, 6, (8, 16)),
    # G = 16: every class, and the widest image
    (3000, 3, 16, 4, 8, 6, (ROW, 16)),
    (3000, 3, 32, 4, 8, 10, (2, 16)),
    (4096, 3, 33, 2, 4, 3, (2, 16)),
    (3000, 3, 16, 4, 8, 10, (4, 16)),
    (3000, 3, 8, 4, 8, 6, (6, 16)),
    (3000, 3, 6, 4, 8, 6, (8, 16)),
    (3000, 3, 4, 4, 8, 6, (0, 16)),
    (4096, 3, 8, 4, 8, 6, (8, 16)), (4096, 3, 16, 4, 8, 6, (ROW, 16)),
]
FEATURE_REFUSED_W = 4097
# the same classes at G = 8 on uint16 labels (rpcc_extract_features_wide)
FEATURE_CASES_WIDE = [c for c in FEATURE_CASES if c[0] in (1500, 1030, 1038, 1034, 1546, 1032)]
# the fused non-uniform entry (no curvature image): (lidar of oracle.GEOMS, settings, (Q, G, compact))
FEATURE_FUSED = [
    ("VelodyneVLP16", dict(feature_region=3, segments=8, sharp_num=4, less_sharp_num=8, flat_num=6), (ROW, 8, True)),       # W = 1800
    ("Velodyne32E", dict(feature_region=3, segments=16, sharp_num=4, less_sharp_num=8, flat_num=6), (ROW, 16, True)),       # W = 2250
    ("VelodyneVLP16", dict(feature_region=3, segments=4, sharp_num=4, less_sharp_num=8, flat_num=6), (8, 8, False)),        # chunk 448
]
FEATURE_CHUNK_PAIRS = [(128, 129), (256, 257), (384, 385), (512, 513)]


def feature_chunk(case):
    return (case[0] - 2 * case[1]) // case[2]


def feature_image(W, params, nlab=20, H=4):
    """(seg int32 [H,W], ri f32 [H,W]) of a key-point case, as tests/test_gpu_parity.py's test_features_edge_rows builds them: runs of five
    equal labels, a smooth range profile with noise and steps (the occlusion gate); row 0 constant (every curvature 0: ties), row 1 without a
    valid pixel, row 2 with too few.  nlab > 256: labels that need uint16."""
    rng = np.random.default_rng(1500 + 13 * W + 7 * params[1] + params[4])
    seg = np.repeat(rng.integers(0, nlab, (H, (W + 4) // 5)), 5, axis=1)[:, :W].astype(np.int32)
    ri = (15 + 4 * np.sin(np.arange(W) / 9.0)[None, :] + rng.normal(0, 0.03, (H, W))).astype(np.float32)
    ri[:, ::53] += 2.5
    ri[0, :] = 20.0
    seg[1, :] = 0
    seg[2, 10:] = 1
    ri[seg == 1] = 0
    return seg, ri


# the parameter tuples this module adds to the pin of orc.extract_features_with_segment against the reference's C++
# (tests/test_oracle_vs_ref.py): (W, (feature_region, segments, sharp, less_sharp, flat))
FEATURE_PIN_DRAWS = [(c[0], tuple(c[1:6])) for c in FEATURE_CASES]

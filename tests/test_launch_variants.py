"""The case tables of tests/launch_variants.py reach every kernel variant the launch code of librpcc_hip can pick, each case takes the
pick written next to it, and every scene of the tables is one the oracle is defined on (M distinct FPS centres, a ground fit that has
its 800 candidates).  CPU only: the rules are restated from the sources, tests/test_gpu_launch_variants.py runs the cases."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import launch_variants as lv
from oracle import oracle as orc


def _names(variants):
    return sorted(" ".join(str(v) for v in k) for k in variants)


def test_constants_are_read_from_the_sources():
    """The constants the rules use are the sources' (a value this test names moved: look at the tables again), and a macro that is no
    longer there raises instead of leaving a stale copy behind."""
    assert (lv.FPS_TT_SMALL, lv.FPS_TT_BATCH, lv.FPS_SMALL_FRAMES, lv.FPS_TILED_MAX_TILES) == (1024, 512, 128, 3200)
    assert (lv.FPS_TROWS, lv.FPS_TILE_COLS, lv.FPS_TILE, lv.FPS_THREADS) == (8, 32, 256, 1024)
    assert (lv.FEAT_ROWMODE, lv.FEAT_RQ, lv.FEAT_ROW_SEGS, lv.FEAT_ROW_FLAT, lv.FEAT_GPW, lv.FEAT_G_NARROW, lv.FEAT_THREADS) == (-1, 16, 32, 8, 16, 8, 256)
    assert lv.FEAT_Q_STEPS == [(2, 2), (4, 4), (6, 6), (8, 8)]
    assert (lv.ASSIGN_ROUNDS_U8, lv.ASSIGN_MID_M, lv.ASSIGN_ROUNDS_MID, lv.ASSIGN_ROUNDS_TOP, lv.MAX_CLUSTERS) == (4, 510, 8, 16, 254)
    with pytest.raises(AssertionError, match="no longer found"):
        lv._define("fps_kernels.h", "FPS_NO_SUCH_MACRO")


def test_fps_tables_take_the_picks_written_next_to_them():
    for (H, W, B, pick) in lv.FPS_FUSED:
        assert lv.fps_pick_range(H, W, B, 0, None, True) == pick, (H, W, B)
        assert not lv.fused_refuses(H, W, B), (H, W, B)
    for (H, W, B) in lv.FPS_FUSED_REFUSED:
        assert lv.fused_refuses(H, W, B) and lv.fps_tiles_range(H, W) > lv.FPS_TILED_MAX_TILES and (H * W) % 2 == 1, (H, W, B)
    for (H, W, B, pick) in lv.FPS_STAGE:
        assert lv.fps_pick_range(H, W, B, 0, None, False) == pick, (H, W, B)
    for (N, B, (H, W), pick) in lv.FPS_LISTS:
        assert lv.fps_pick_list(N, B) == pick, (N, B)
    for table in (lv.FPS_MIXED, lv.FPS_MIXED_SMALL):
        got = lv.mixed_fps_picks([(H, W, B, lv.range_quads16(W)) for (H, W, B, _, _) in table])
        assert got == [(c, k) for (_, _, _, c, k) in table], table
        assert all(B <= lv.FPS_SMALL_FRAMES for (_, _, B, _, _) in table)     # alone, every group takes the 1024-thread kernels
    assert sum(B for (_, _, B, _, _) in lv.FPS_MIXED) == 130
    # the planar2 pick that takes the third group out of the common launch
    assert lv.fps_pick_range(9, 8209, 130, 0, False, True) == (lv.PLANAR2, 512, lv.EDGE)


def test_fps_tables_state_the_issue_s_tile_counts_and_boundaries():
    """The shapes the tables must hold whatever else reaches the same pick (several rows repeat a pick on purpose: a boundary's other side, a
    row-end quad of another length), so removing one of THOSE rows is named here, by shape, not by test_fps_tables_reach_every_variant."""
    tiles = {(H, W): lv.fps_tiles_range(H, W) for (H, W, _, _) in lv.FPS_FUSED}
    want = [(7, 301, 3), (7, 301, 129), (8, 512, 3), (8, 512, 129), (9, 8209, 3), (9, 8209, 128), (9, 8209, 129), (9, 8212, 3), (9, 8212, 129),
            (2, 32801, 3), (2, 32801, 129), (2, 32804, 3), (2, 32804, 129), (8, 514, 3), (8, 514, 129), (9, 8211, 3), (9, 8211, 129),
            (8, 16384, 129), (8, 16385, 129), (8, 32768, 2), (8, 32769, 2), (8, 32768, 129), (8, 32769, 129), (8, 65536, 2), (8, 65537, 2),
            (8, 102400, 2), (8, 102399, 2), (8, 102401, 2)]
    missing = sorted(set(want) - {c[:3] for c in lv.FPS_FUSED})
    assert not missing, "FPS_FUSED no longer holds (H, W, frames): %s" % missing
    want = [(7, 301, 3), (8, 512, 3), (7, 301, 129), (8, 512, 129), (9, 8209, 129), (9, 8212, 129), (2, 32801, 2), (2, 32804, 2), (8, 514, 3),
            (8, 514, 129), (8, 513, 129), (4, 16402, 129), (2, 32802, 2)]
    missing = sorted(set(want) - {c[:3] for c in lv.FPS_STAGE})
    assert not missing, "FPS_STAGE no longer holds (H, W, frames): %s" % missing
    # every EDGE / element form of the stage entries has a case the brute-force entry takes (P % 4 == 0): a witness for the final temp
    for k in {k for (_, _, _, k) in lv.FPS_STAGE if k[2] == lv.EDGE}:
        assert any(c[3] == k and (c[0] * c[1]) % 4 == 0 for c in lv.FPS_STAGE), ("no case with P % 4 == 0 takes", k)
    assert tiles[(7, 301)] == 10 and tiles[(8, 512)] == 16 and tiles[(9, 8209)] == tiles[(9, 8212)] == 514
    assert tiles[(2, 32801)] == tiles[(2, 32804)] == 1026
    assert (tiles[(8, 16384)], tiles[(8, 16385)], tiles[(8, 32768)], tiles[(8, 32769)], tiles[(8, 65536)], tiles[(8, 65537)]) == (512, 513, 1024, 1025, 2048, 2049)
    assert tiles[(8, 102399)] == tiles[(8, 102400)] == lv.FPS_TILED_MAX_TILES and tiles[(8, 102401)] == lv.FPS_TILED_MAX_TILES + 1
    assert [lv.fps_tiles_list(N) for (N, _, _, _) in lv.FPS_LISTS] == [16, 16, 514, 514, 16, 16, 1026, 1026]
    for a, b in zip(lv.FPS_LISTS[::2], lv.FPS_LISTS[1::2]):     # a multiple of four, and the same tile count a little below it
        assert a[0] % 4 == 0 and b[0] % 4 != 0 and a[0] - 3 <= b[0] < a[0] and a[1:3] == b[1:3], (a, b)
    # the EDGE cases leave row-end quads of one, two and three pixels
    assert {W % 4 for (_, W, _, k) in lv.FPS_FUSED if k[0] in (lv.PLANAR, lv.PLANAR2) and k[2] == lv.EDGE} == {1, 2, 3}
    assert {W % 4 for (_, W, _, k) in lv.FPS_STAGE if k[0] == lv.REG_TABLE and k[2] == lv.EDGE} >= {1, 2}
    # every batch of more than one frame ends on another scene than it began with, and has at most five
    for (H, W, B, _) in lv.FPS_FUSED + lv.FPS_STAGE:
        n = lv.n_scenes(H, W, B)
        assert 1 <= n <= 5 and (B == 1 or lv.scene_of(B - 1, n) != lv.scene_of(0, n)), (H, W, B)


def test_fps_tables_reach_every_variant():
    """{planar, planar2, register table, LDS table} x {1024, 512} x {16-byte, EDGE / element} for range images, {register table, LDS table}
    x the same for lists, the multi kernel at both thread counts with an aligned and an EDGE group in one launch, and the one-pass
    pick above 3200 tiles.  Removing the last row that reaches a variant names that variant here; a row whose pick another row repeats is
    named by shape in test_fps_tables_state_the_issue_s_tile_counts_and_boundaries."""
    missing = lv.fps_variants_wanted() - lv.fps_variants_reached()
    assert not missing, "no case of tests/launch_variants.py reaches: " + "; ".join(_names(missing))


def test_feature_tables_reach_every_variant():
    widths = {name: orc.GEOMS[name]["W"] for name, _, _ in lv.FEATURE_FUSED}
    for c in lv.FEATURE_CASES:
        assert lv.feature_pick(c[0], c[1], c[2], c[5]) == c[6] + (False,), c
    for name, kp, pick in lv.FEATURE_FUSED:
        assert lv.feature_pick(widths[name], kp["feature_region"], kp["segments"], kp["flat_num"], feat=False) == pick, name
    assert sorted(widths.values()) == [1800, 2250]
    missing = lv.feature_variants_wanted() - lv.feature_variants_reached(widths)
    assert not missing, "no case of tests/launch_variants.py reaches: " + "; ".join(_names(missing))
    # the class boundaries: both sides of every chunk length at which the class changes, of W = 2048 / 2049, and the widest image
    chunks = {lv.feature_chunk(c): c[6][0] for c in lv.FEATURE_CASES if c[5] == 10 or c[6][0] != lv.ROW}
    for a, b in lv.FEATURE_CHUNK_PAIRS:
        assert a in chunks and b in chunks and chunks[a] != chunks[b], (a, b)
    row = {lv.feature_chunk(c) for c in lv.FEATURE_CASES if c[6][0] == lv.ROW}
    assert 256 in row and chunks[257] == 6                     # the end of row mode with the default flat_num
    assert {c[0] for c in lv.FEATURE_CASES} >= {2048, 2049, 4096}
    assert lv.feature_pick(4096, 3, 8, 6) is not None and lv.feature_pick(lv.FEATURE_REFUSED_W, 3, 8, 6) is None
    # Q = 2 and Q = 4 are reached both ways the rule allows: more than 32 segments, and flat_num 10
    assert any(c[2] > lv.FEAT_ROW_SEGS and c[6][0] == 2 for c in lv.FEATURE_CASES) and any(c[5] == 10 and c[6][0] == 4 for c in lv.FEATURE_CASES)


def test_feature_images_hold_the_edge_rows():
    """Row 0 constant, row 1 without a valid pixel, row 2 with too few; the oracle finds key points in what is left."""
    for c in lv.FEATURE_CASES:
        seg, ri = lv.feature_image(c[0], c[1:6])
        assert np.ptp(ri[0][seg[0] != 1]) == 0 and not seg[1].any() and (seg[2] != 1).sum() <= 10, c
        _, kp = orc.extract_features_with_segment(ri, seg, *c[1:6])
        assert kp.max() >= 1 and not kp[1].any() and not kp[2].any(), c
    seg, _ = lv.feature_image(1500, (3, 8, 4, 8, 6), nlab=600)
    assert seg.max() > 255


def test_assignment_cases():
    assert [(M, lv.label_bytes(M), lv.assign_rounds(lv.label_bytes(M), M)) for (M, _, _) in lv.ASSIGN_CASES] == lv.ASSIGN_CASES
    assert {M for (M, _, _) in lv.ASSIGN_CASES} == {lv.MAX_CLUSTERS, lv.MAX_CLUSTERS + 1, lv.ASSIGN_MID_M, lv.ASSIGN_MID_M + 1}


def _scene_facts(args):
    H, W, k, M = args
    g = lv.geom_of(H, W)
    tm = orc.transform_map(g)
    f = lv.scene_frame(H, W, k)
    ri = orc.project(f, g)
    cand = orc.ground_candidates(ri, tm).shape[0]
    s = orc.segment(ri, tm, orc.ground_model(ri, tm, seed=7 + k), dict(orc.DEFAULT_CFG, cluster_num=M))
    ends = [p for p in s["fps_pix"].tolist() if p % W in lv.row_end_columns(W)]
    return args, cand, len(set(s["fps_pix"].tolist())), len(ends), sum(p % W == W - 1 for p in ends)


def _scenes():
    """Every distinct (H, W, scene, M) of the tables."""
    out = set()
    for (H, W, B, _) in lv.FPS_FUSED + lv.FPS_STAGE:
        out |= {(H, W, k, lv.default_m(H, W)) for k in range(lv.n_scenes(H, W, B))}
    for (H, W, B) in lv.FPS_FUSED_REFUSED:
        out |= {(H, W, k, lv.default_m(H, W)) for k in range(lv.n_scenes(H, W, B))}
    for (H, W, B, _, _) in lv.FPS_MIXED + lv.FPS_MIXED_SMALL:
        out |= {(H, W, k, lv.MIXED_M) for k in range(lv.n_scenes(H, W, B))}
    for (H, W) in lv.ALIGN_SHAPES:
        out |= {(H, W, k, lv.default_m(H, W)) for k in range(2)}
    out |= {lv.ASSIGN_SHAPE + (0, M) for (M, _, _) in lv.ASSIGN_CASES}
    return sorted(out)


def test_every_scene_has_m_distinct_centres_and_a_ground_fit():
    """No scene of any table may have fewer than M distinct FPS centres (the reference is undefined there) or fewer than 800 ground
    candidates (the batch fit would take the ground-less path)."""
    with ThreadPoolExecutor(8) as ex:
        for args, cand, distinct, ends, last in ex.map(_scene_facts, _scenes()):
            assert distinct == args[3], (args, distinct)
            assert cand >= 800, (args, cand)
            # centres in the row-end quads, and in the last column (a short quad's last valid element): what makes a mis-read row end visible
            assert ends >= 1 and last >= 1, (args, ends, last)


def test_every_list_has_m_distinct_centres_and_the_order_the_probe_wants():
    """The lists are non-empty pixels of a synthetic image in row-major order, cut to N points: each holds LIST_M distinct centres and is,
    by a margin far above fp32 rounding, on the coherent side of the probe's measure (so the pruned kernel takes it); shuffled it is on the other side."""
    for (N, B, (H, W), _) in lv.FPS_LISTS:
        for k in range(lv.n_scenes(H, W, B)):
            pts = lv.list_points(H, W, k, N)
            assert pts.shape == (N, 3), (N, H, W, k)
            assert len(set(orc.fps(pts, lv.LIST_M).tolist())) == lv.LIST_M, (N, k)
            assert lv.list_order_measure(pts) < 0.8 * lv.PROBE_CUT, (N, k, lv.list_order_measure(pts))
            assert lv.list_order_measure(pts[np.random.default_rng(N).permutation(N)]) > 1.25 * lv.PROBE_CUT, (N, k)

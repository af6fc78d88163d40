"""The numpy reference of the radius outlier removal (tests/radius_filter_ref.py) pins every rule of DESIGN.md section 17 on hand
fixtures and, where scipy is present, agrees with cKDTree.  No GPU needed."""
import numpy as np
import pytest

import filter_cases as FC
import radius_filter_ref as R

F32 = np.float32


def keep(xyz, nb_points=3, radius=1.0, offsets=None):
    return R.radius_filter(np.array(xyz, F32), offsets, nb_points, radius)["keep"].tolist()


def test_boundary_is_strict():
    """d^2 == r^2 is no neighbour; one fp32 step closer is."""
    assert keep([[0, 0, 0], [1, 0, 0]], nb_points=1) == [False, False]
    assert keep([[0, 0, 0], [np.nextafter(F32(1), F32(0)), 0, 0]], nb_points=1) == [True, True]
    assert keep([[0, 0, 0], [0, 3, 4]], nb_points=1, radius=5.0) == [False, False]


def test_count_of_nb_points_is_removed_and_one_more_is_kept():
    three = [[0, 0, 0], [0.1, 0, 0], [0, 0.1, 0]]
    assert keep(three) == [False] * 3
    assert keep(three + [[0, 0, 0.1]]) == [True] * 4
    r = R.radius_filter(np.array(three + [[0, 0, 0.1], [0.1, 0.1, 0]], F32), None, 3, 1.0)
    assert r["count"].tolist() == [4] * 5 and r["kept"].tolist() == [5] and r["index"].tolist() == [0, 1, 2, 3, 4]      # clipped at nb_points + 1


def test_the_point_itself_counts():
    assert R.frame_counts(np.array([[7, 7, 7]], F32), 1.0).tolist() == [1]
    assert keep([[0, 0, 0], [0.5, 0, 0]], nb_points=1) == [True, True]      # itself + one other > 1


def test_duplicates_count():
    assert keep([[2, 2, 2]] * 4) == [True] * 4 and keep([[2, 2, 2]] * 3) == [False] * 3


def test_nb_points_zero_keeps_every_finite_point():
    assert keep([[0, 0, 0], [100, 0, 0], [np.nan, 0, 0], [0, np.inf, 0]], nb_points=0) == [True, True, False, False]


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_nonfinite_points_are_removed_and_invisible(bad):
    for axis in range(3):
        b = [0.0, 0.0, 0.0]
        b[axis] = bad
        assert keep([[0, 0, 0], [0.1, 0, 0], [0, 0.1, 0], b]) == [False] * 4      # were b seen, the three would be kept
        assert R.frame_counts(np.array([[0, 0, 0], b], F32), 1.0).tolist() == [1, 0]


def test_a_twin_in_the_neighbouring_frame_does_not_count():
    pts = [[0, 0, 0], [0.1, 0, 0], [0, 0.1, 0], [0, 0, 0]]
    assert keep(pts) == [True] * 4
    assert keep(pts, offsets=np.array([0, 3, 4])) == [False] * 4


def test_wider_inputs_are_narrowed_first():
    """In fp64 the pair is 1 - 1e-12 apart (a neighbour); narrowed to float32 it is exactly 1 apart (none)."""
    pts = np.array([[0, 0, 0], [1 - 1e-12, 0, 0]], np.float64)
    assert R.radius_filter(pts, None, 1, 1.0)["keep"].tolist() == [False, False]


def test_grid_search_equals_the_dense_matrix():
    for seed, radius in ((0, 1.0), (1, 0.45), (2, 6.0), (3, 0.05)):
        xyz = FC.blob_cloud(1500, seed) * F32(radius)
        xyz[::97] = np.nan
        want = R.brute_counts(xyz, radius)
        assert np.array_equal(R.frame_counts(xyz, radius), want)
        for cap in (1, 4, 51):
            assert np.array_equal(np.minimum(R.frame_counts(xyz, radius, cap), cap), np.minimum(want, cap))
    far = np.array([[1e30, 0, 0], [1e30, 0.5, 0], [-3e38, 0, 0], [3e38, 0, 0], [0, 0, 0]], F32)      # past the bucket clip
    assert R.frame_counts(far, 1.0).tolist() == [2, 2, 1, 1, 1]


def _tree_counts(xyz, radius):
    from scipy.spatial import cKDTree
    p = xyz.astype(np.float64)
    return cKDTree(p).query_ball_point(p, radius, return_length=True)


def test_reference_against_ckdtree_on_the_example_sweep():
    """cKDTree counts d <= r: the one pair of the sweep within 4 fp64 ulps of r^2 (tests/golden/gen_golden_radius_filter.py found it by
    looking at every pair of adjacent buckets) is ruled out first."""
    pytest.importorskip("scipy")
    xyz = FC.example_sweep()
    g = FC.golden()
    other = np.setdiff1d(np.arange(xyz.shape[0]), g["boundary_pairs"].reshape(-1))
    tree = _tree_counts(xyz, 1.0)
    for nb in (3, 20):
        r = R.radius_filter(xyz, None, nb, 1.0)
        assert np.array_equal(np.minimum(tree, nb + 1)[other], r["count"][other])
    assert np.array_equal(tree > 3, g["keep"])


@pytest.mark.parametrize("seed", range(4))
def test_reference_against_ckdtree_random(seed):
    pytest.importorskip("scipy")
    radius = (1.0, 0.45, 6.0, 0.05)[seed]
    xyz = FC.blob_cloud(4000, 100 + seed) * F32(radius)
    pairs = R.near_boundary(xyz, radius, ulps=4)
    other = np.setdiff1d(np.arange(xyz.shape[0]), pairs.reshape(-1))
    assert np.array_equal(_tree_counts(xyz, radius)[other], R.frame_counts(xyz, radius)[other])

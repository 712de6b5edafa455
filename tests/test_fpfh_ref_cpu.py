"""The FPFH restatement (tests/fpfh_ref.py) against hand cases worked from the reference's lines (src/gtsam_points/features/fpfh_estimation.cpp:58-93, :196-307), and
the input check of tests/test_fpfh_gpu.py: every cloud those tests use is at least 99 % settled by the reference alone, under the cap and without it.  The device's
binding the restatement stands for must exist (the first test): the restatement alone is no feature."""
import numpy as np
import pytest

import fpfh_ref as R


def test_the_device_entry_the_restatement_stands_for_exists():
    import gtsam_points_amd as gpa

    assert callable(gpa.estimate_fpfh_gpu) and gpa.FPFHEstimationParams().search_radius == 5.0
    assert hasattr(gpa.load(), "gp_estimate_fpfh")


@pytest.fixture(scope="module")
def refs(fpfh_entry_exists):
    return {(name, cap): R.estimate(*R.cloud(name), cap) for name in R.CLOUDS for cap in (10000, R.CAP)}


@pytest.fixture(scope="module")
def fpfh_entry_exists():
    import gtsam_points_amd as gpa

    assert callable(gpa.estimate_fpfh_gpu)


def test_pair_features_hand_cases(fpfh_entry_exists):
    z = np.array([0.0, 0.0, 1.0])
    x = np.array([1.0, 0.0, 0.0])
    o = np.zeros(3)
    # coincident points: d == 0 (:61-63)
    assert np.array_equal(R.compute_pair_features(o, z, o, x), [0.0, 0.0, 0.0])
    # both normals along the direction: |angle1| = |angle2| = 1, no swap, ndp x n1 = 0, v = 0 / 0 is not finite (:83-86)
    assert np.array_equal(R.compute_pair_features(o, z, 2.0 * z, z), [0.0, 0.0, 0.0])
    # no swap: n1 = z is nearer the direction than n2 = x.  ndp = (0, 0.6, 0.8): angle1 = 0.8, angle2 = 0
    f = R.compute_pair_features(o, z, np.array([0.0, 3.0, 4.0]), x)
    v = np.array([0.6, 0.0, 0.0]) / 0.6  # ndp x n1 = (0.6, 0, 0)
    assert f[2] == 0.8 and f[1] == v @ x == 1.0
    assert f[0] == np.arctan2(np.cross(z, v) @ x, 0.0) == 0.0
    # forced swap: the same pair with the normals exchanged: angle1 = 0 < angle2 = 0.8 -> n1 := z, n2 := x, ndp := -ndp, alpha = -0.8 (:76-81)
    f = R.compute_pair_features(o, x, np.array([0.0, 3.0, 4.0]), z)
    assert f[2] == -0.8
    v = np.array([-0.6, 0.0, 0.0]) / 0.6  # (-ndp) x z
    assert f[1] == v @ x == -1.0 and f[0] == np.arctan2(np.cross(z, v) @ x, 0.0)
    # alpha = 1 and theta = pi land on the upper edge and are clamped into bin 10 (:238)
    b, _ = R.bins_of(np.array([[np.pi, 1.0, 1.0], [-np.pi, -1.0, -1.0], [0.0, 0.0, 0.0], [np.nan, np.nan, 0.5]]))
    assert b.tolist() == [[10, 10, 10], [0, 0, 0], [5, 5, 5], [0, 0, 8]]
    f = R.compute_pair_features(o, _unit([1e-3, 0.0, 1.0]), 2.0 * z, _unit([-1e-3, 0.0, -1.0]))  # n2 = -n1: theta = atan2(+0 or tiny, -1) = pi
    assert abs(abs(f[0]) - np.pi) < 1e-12 and R.bins_of(f[None])[0][0, 0] in (0, 10)


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def test_two_points_have_three_single_100s(refs):
    r = refs[("two", 10000)]
    assert r.n.tolist() == [2, 2]
    for k in range(2):
        for c in range(3):
            block = r.spfh[k, 11 * c : 11 * c + 11]
            assert sorted(block.tolist()) == [0.0] * 10 + [100.0]
    # FPFH of a two-point cloud: the other point's SPFH times 1 / d2, normalised by its first block: the same three 100s
    assert np.array_equal(r.fpfh[0], r.spfh[1]) and np.array_equal(r.fpfh[1], r.spfh[0])


def test_a_point_alone_and_coincident_copies(refs):
    r = refs[("one", 10000)]
    assert r.n.tolist() == [1] and not r.spfh.any() and not r.fpfh.any()
    p = np.tile(np.array([[0.5, 0.25, -1.0]], np.float32), (3, 1))
    n = np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (3, 1))
    c = R.estimate(p, n, 0.8)
    assert c.n.tolist() == [3, 3, 3]
    # every pair returns zero (d == 0): bin 5 of each block; every sq_dist is 0, the sum is empty, 0 * (100 / 0) = NaN (:263-275)
    assert all(c.hist[k].tolist() == ([0] * 5 + [2] + [0] * 5) * 3 for k in range(3))
    assert np.isnan(c.fpfh).all()


def test_the_radius_is_strict(fpfh_entry_exists):
    p = np.array([[0.0, 0.0, 0.0], [0.75, 0.0, 0.0], [0.0, 0.5, 0.0]], np.float32)  # d2 = 0.5625 = 0.75 * 0.75 exactly
    n = np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (3, 1))
    c = R.estimate(p, n, 0.75)
    assert c.neighbors[0].tolist() == [0, 2] and c.neighbors[1].tolist() == [1] and not c.settled[0] and not c.settled[1]
    c = R.estimate(p, n, np.nextafter(0.75, 1.0))
    assert sorted(c.neighbors[0].tolist()) == [0, 1, 2]


def test_every_block_of_an_spfh_sums_to_100(refs):
    for name in ("random600", "plane400", "sphere400", "cell65"):
        r = refs[(name, 10000)]
        rows = r.n > 1
        assert rows.any()
        for c in range(3):
            assert np.array_equal(r.hist[rows, 11 * c : 11 * c + 11].sum(axis=1), r.n[rows] - 1)  # the point itself is among its neighbours
            assert np.allclose(r.spfh[rows, 11 * c : 11 * c + 11].sum(axis=1), 100.0, rtol=1e-13, atol=0.0)


def test_the_walk_order_under_the_cap(fpfh_entry_exists):
    # four points in four cells around the query's cell (r = 1): the walk takes (dz, dy, dx) ascending, dx fastest, then the index
    p = np.array([[0.5, 0.5, 0.5], [1.1, 0.5, 0.5], [0.5, -0.1, 0.5], [0.5, 0.5, -0.1], [0.6, 0.5, 0.5], [-0.1, 0.5, 0.5]], np.float32)
    n = np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (6, 1))
    c = R.estimate(p, n, 1.0)
    assert c.neighbors[0].tolist() == [3, 2, 5, 0, 4, 1]
    c = R.estimate(p, n, 1.0, max_num_neighbors=3)
    assert c.neighbors[0].tolist() == [3, 2, 5] and c.n[0] == 3 and c.num_truncated == 6  # the point itself is cut off; the pairs still count


@pytest.mark.parametrize("name", R.CLOUDS)
def test_every_gpu_cloud_is_settled_by_the_reference_alone(refs, name):
    for cap in (10000, R.CAP):
        r = refs[(name, cap)]
        assert r.settled.mean() >= 0.99 and r.row_settled.mean() >= 0.99, (name, cap, r.settled.mean(), r.row_settled.mean())


def test_the_trial_figures_of_the_random_cloud(refs):
    r = refs[("random600", 10000)]
    assert 16.0 < r.n.mean() < 18.0 and 30 <= r.n.max() <= 36
    assert r.settled.all() and r.min_bin_margin > 1e-6 and r.min_swap_margin > 1e-6
    assert refs[("random600", R.CAP)].num_truncated > 300  # the cap binds for most points


def test_plane_and_sphere_are_settled_through_the_both_branches_rule(refs):
    plane, sphere = refs[("plane400", 10000)], refs[("sphere400", 10000)]
    assert plane.settled.all() and plane.num_ties == int((plane.n - 1).sum())  # every pair of the plane ties exactly
    assert not R.estimate(*R.cloud("plane400"), tie_rule=False).settled.any()
    assert sphere.settled.all() and sphere.num_ties > 0  # (f32 points: most pairs miss the exact tie by their rounding, some do not)


def test_height_field_features_match_their_own_copies(fpfh_entry_exists):
    tp, tn, sp, sn, T, radius = R.height_field()
    assert np.array_equal((T[:3, :3] @ sp.astype(np.float64).T).T + T[:3, 3], tp.astype(np.float64))  # the pose is exact on the f32 points
    a, b = R.estimate(tp, tn, radius), R.estimate(sp, sn, radius)
    assert np.array_equal(a.hist, b.hist) and np.array_equal(a.n, b.n)
    d = ((a.fpfh[:, None, :] - b.fpfh[None, :, :]) ** 2).sum(axis=-1)
    own = np.arange(len(tp))
    assert (d.argmin(axis=1) == own).mean() >= 0.9 and (d.argmin(axis=0) == own).mean() >= 0.9

"""The FPFH restatement (tests/fpfh_ref.py) against hand cases worked from the reference's lines (src/gtsam_points/features/fpfh_estimation.cpp:58-93, :196-307), and
the input check of tests/test_fpfh_gpu.py and tests/test_fpfh_edges_gpu.py: every cloud those tests use is at least 99 % settled by the reference alone, under the
caps and without them, and the edge clouds have the ties, batches, clamped cells and wrapped probes they are there for.  The device's
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


# ---- what tests/test_fpfh_edges_gpu.py rests on: the edge clouds, certified by the restatement alone ------------------------------------------------------------------


@pytest.mark.parametrize("name", R.EDGE_CLOUDS)
def test_every_edge_cloud_is_settled_by_the_reference_alone(fpfh_entry_exists, name):
    for cap in R.EDGE_CAPS[name]:
        r = R.edge_ref(name, cap)
        assert r.settled.mean() >= 0.99 and r.row_settled.mean() >= 0.99, (name, cap, r.settled.mean(), r.row_settled.mean())
        assert r.finite.sum() >= len(r.n) - 4 and len(r.neighbors) == len(r.n)  # n and the walk order are there for every point


def test_the_lattice_ties_exactly_and_only_the_exact_rule_settles_it(fpfh_entry_exists):
    p, n, radius = R.edge_cloud("lattice384")
    r = R.edge_ref("lattice384")
    ties = R.exact_ties(p, radius)  # counted in integers
    assert len(ties) == r.num_exact_ties == 5472
    assert r.settled.all() and r.n.max() == 93
    assert (R.cell_of(p, radius).min(axis=0) == -1).all()  # cells on both sides of zero
    assert not R.estimate(p, n, radius).settled.any()  # every point has a partner at d2 == r * r: without the rule nothing is settled
    # the strict rule leaves every tie partner out
    assert all(j not in r.neighbors[i].tolist() for i, j in ties)
    # the next radius up has a rounded r * r: the guard refuses it, ties or none
    with pytest.raises(ValueError):
        R.estimate(p, n, np.nextafter(radius, 1.0), exact_edges=True)


def test_the_exactness_guard(fpfh_entry_exists):
    for name in R.EXACT_CLOUDS:
        R.assert_exact(*[R.edge_cloud(name)[i] for i in (0, 2)])
    p, n, radius = R.cloud("random600")
    with pytest.raises(ValueError):
        R.assert_exact(p, radius)  # 0.8 * 0.8 is rounded
    with pytest.raises(ValueError):
        R.assert_exact(p, 0.75)  # ... and with an exact r * r the squared distances of 24-bit coordinates are
    with pytest.raises(ValueError):
        R.estimate(p, n, radius, exact_edges=True)  # the option cannot be had without the guard
    # exact, yet within MARGIN of r * r without being on it: the point stays unsettled under exact_edges
    q = np.array([[0.0, 0.0, 0.0], [0.75, 0.0, 0.0], [0.0, 0.0, 0.75 + 2.0**-23]], np.float32)
    c = R.estimate(q, np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (3, 1)), 0.75, exact_edges=True)
    assert c.num_exact_ties == 2 and c.n.tolist() == [1, 1, 1] and c.settled.tolist() == [True, True, True]
    h = np.array([[0.0, 0.0, 0.0], [0.5, 2.0**-17, 0.0]], np.float32)  # d2 = 0.25 + 2^-34, exact, 2.3e-10 relative beyond r * r = 0.25
    c = R.estimate(h, np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (2, 1)), 0.5, exact_edges=True)
    assert c.num_exact_ties == 0 and not c.settled.any() and c.n.tolist() == [1, 1]


def test_the_dense_cloud_fills_every_lane_and_every_cap_cuts_inside_a_cell(fpfh_entry_exists):
    r = R.edge_ref("dense1500")
    assert r.n.min() > 200 and r.num_truncated == 0  # pass 2: every lane adds more than three terms
    for cap in (64, 65, 100, 200):
        assert R.edge_ref("dense1500", cap).num_truncated == 1500
    one = R.edge_ref("dense1500", 1)
    assert (one.n == 1).all() and not one.spfh.any() and not one.fpfh.any() and one.num_truncated == 1500
    for cap in (65, 129):
        ends = [R.walk_end(R.edge_ref("dense1500", cap), k) for k in range(1500)]
        assert sum(batch == 1 and more > 0 for batch, more in ends) > 100 and sum(batch >= 2 and more > 0 for batch, more in ends) > 100  # (base > begin)


@pytest.mark.parametrize("name", ("clamp400", "clamp400neg"))
def test_the_clamp_clouds_reach_and_pass_the_clamped_cell(fpfh_entry_exists, name):
    p, _, radius = R.edge_cloud(name)
    x = p[:, 0].astype(np.float64)
    sign = -1 if name.endswith("neg") else 1
    assert (np.sign(x) == sign).all()
    assert (R.cell_of(x, radius) == sign * R.CELL_LIMIT).sum() > 100  # in the clamped cell ...
    assert (sign * np.floor(x / radius) > R.CELL_LIMIT).sum() > 100  # ... most of them from beyond it
    assert (sign * R.cell_of(x, radius) < R.CELL_LIMIT).sum() > 100
    assert R.edge_ref(name, R.CAP).num_truncated > 100
    # the header's claim, on this cloud: no true neighbours more than one (clamped) cell apart
    r = R.edge_ref(name)
    assert all(np.abs(r.cells[js] - r.cells[k]).max() <= 1 for k, js in enumerate(r.neighbors))


def test_the_wrap_cloud_probes_across_the_end_of_the_table(fpfh_entry_exists):
    p, _, radius = R.edge_cloud("wrap2000")
    t = R.table_placement(p, radius)
    mask = t["mask"]
    assert mask == 4095 and 0.45 < len(t["keys"]) / (mask + 1.0) <= 0.5
    assert (t["home"] >= mask - 1).sum() >= 3 and t["wrapped"].sum() >= 2 and t["probes"].max() >= 4
    # the planted points come first, so their cells are keys 0 .. 4: three singles, then A and B
    assert np.array_equal(t["cells"][:5], R.cell_of(p[[0, 1, 2, 3, 6]], radius))
    assert t["wrapped"][3] and t["wrapped"][4] and np.abs(t["cells"][3] - t["cells"][4]).sum() == 1
    r = R.edge_ref("wrap2000")
    a, b = R.WRAP_PLANTED["a"], R.WRAP_PLANTED["b"]
    for i in a + b:
        assert sorted(r.neighbors[i].tolist()) == sorted(a + b)  # the six points of A and B are each other's neighbours
    assert R.edge_ref("wrap2000", R.CAP).num_truncated >= 80
    # the restated hash against values worked by hand from the device's lines: key of cell (0, 0, 0), and the finaliser of 1
    assert int(R.pack_cell(0, 0, 0)) == (1 << 62) | (1 << 41) | (1 << 20) and int(R.pack_cell(-1, 1, 2)) == ((1 << 20) - 1 << 42) | ((1 << 20) + 1 << 21) | ((1 << 20) + 2)
    k = 1
    for mul in (0xFF51AFD7ED558CCD, 0xC4CEB9FE1A85EC53):
        k = ((k ^ (k >> 33)) * mul) & ((1 << 64) - 1)
    assert int(R.hash_key(1)[0]) == (k ^ (k >> 33)) & 0xFFFFFFFF
    assert [R.fpfh_slots(n) for n in (1, 512, 513, 2040, 2048, 2049)] == [1024, 1024, 2048, 4096, 4096, 8192]


def test_far_and_dirty_clouds_are_what_they_say(fpfh_entry_exists):
    p, _, _ = R.edge_cloud("far600")
    assert np.abs(p).min() > 2.9e4 and p.dtype == np.float32
    p, n, _ = R.edge_cloud("dirty300")
    d = R.DIRTY
    assert np.isnan(p[d["nan_point"], 1]) and p[d["pos_inf"], 0] == np.inf and p[d["neg_inf"], 2] == -np.inf and p[d["huge"]].tolist() == [np.float32(3e38), np.float32(-3e38), np.float32(3e38)]
    assert not n[list(d["zero_normals"])].any() and (~np.isfinite(p).all(axis=1)).sum() == 3
    assert [len(v) for v in R.dirty_copies().values()] == list(d["copies"])
    r = R.edge_ref("dirty300")
    for i in (d["nan_point"], d["pos_inf"], d["neg_inf"]):
        assert r.n[i] == 0 and not r.spfh[i].any() and not r.fpfh[i].any()
    assert r.n[d["huge"]] == 1 and not r.fpfh[d["huge"]].any()
    assert all(i not in js.tolist() for k, js in enumerate(r.neighbors) for i in (d["nan_point"], d["pos_inf"], d["neg_inf"], d["huge"]) if k != i)
    for s, copies in R.dirty_copies().items():
        assert r.hist[s][5] >= len(copies) and set(copies) <= set(r.neighbors[s].tolist())


def test_zero_normal_hand_cases(fpfh_entry_exists):
    z, o = np.array([0.0, 0.0, 1.0]), np.zeros(3)
    q = np.array([0.0, 3.0, 4.0])  # ndp = (0, 0.6, 0.8)
    # n1 = 0: angle1 = 0 < angle2 = 0.8, the swap (:76-81): n1 := z, n2 := 0, ndp := -ndp, alpha = -0.8.  v = (-ndp) x z = (-0.6, 0, 0) / 0.6; phi = v . 0 = 0;
    # theta = atan2(w . 0, z . 0) = atan2(+-0, +0) = +-0 (:88-91)
    f = R.compute_pair_features(o, o, q, z)
    assert f[2] == -0.8 and f[1] == 0.0 and f[0] == 0.0
    assert R.bins_of(f[None])[0].tolist() == [[5, 5, 1]]
    # n2 = 0: angle2 = 0, no swap; v = ndp x z = (0.6, 0, 0) / 0.6; phi = 0, theta = atan2(+-0, +0), alpha = 0.8
    f = R.compute_pair_features(o, z, q, o)
    assert f[2] == 0.8 and f[1] == 0.0 and f[0] == 0.0
    assert R.bins_of(f[None])[0].tolist() == [[5, 5, 9]]
    # both zero: angle1 = angle2 = 0, no swap, v = ndp x 0 = 0, 0 / 0 is not finite: the zero return (:83-86)
    assert np.array_equal(R.compute_pair_features(o, o, q, o), [0.0, 0.0, 0.0])
    # n1 with three negative components against n2 = 0: n1 . n2 = (-0 + -0) + -0 = -0, and atan2(+-0, -0) = +-pi: bin 10 or 0, by IEEE 754's rule
    m = -np.array([1.0, 2.0, 2.0]) / 3.0
    rule = []
    f = R.pair_features_branch(o, m, q, o, [False], rule)[0][0]
    assert abs(f[0]) == np.pi and f[1] == 0.0 and rule[0].tolist() == [True]
    assert R.bins_of(f[None])[0][0, 0] == (10 if f[0] > 0 else 0)
    # ... and in a cloud such a pair is settled although nf * 11 sits on an integer
    c = R.estimate(np.stack([o, q]).astype(np.float32), np.stack([m, o]).astype(np.float32), 6.0)
    assert c.n.tolist() == [2, 2] and c.settled.all() and c.hist[0, [0, 10]].sum() == 1


def test_three_points_with_one_duplicate(fpfh_entry_exists):
    p = np.array([[0.25, 0.5, 1.0], [0.25, 0.5, 1.0], [0.75, 0.5, 1.0]], np.float32)  # d2 = 0.25, 1 / d2 = 4: every scaling below is exact
    n = np.stack([_unit([0.1, 0.2, 1.0]), _unit([0.3, -0.2, 0.9]), _unit([-0.2, 0.1, 1.0])]).astype(np.float32)
    c = R.estimate(p, n, 0.8)
    assert c.n.tolist() == [3, 3, 3] and c.settled.all()
    for k in (0, 1):
        for b in range(3):
            block = c.hist[k, 11 * b : 11 * b + 11]
            assert block.sum() == 2 and block[5] >= 1  # the copy's pair returns zero (d == 0): bin 5 of each block; it counts in size (100 / 2 per pair)
        assert c.spfh[k, 5] >= 50.0
        # the copy has d2 == 0 and is skipped in the sum (:263-268): what is left is the third point's row, times 4, times 100 / 400
        assert np.array_equal(c.fpfh[k], c.spfh[2])
    assert np.array_equal(c.fpfh[2], (c.spfh[0] + c.spfh[1]) * 0.5)

"""The inputs of the registration edge tests (tests/registration_edges.py, rr.make_small_case) held to the conditions their exact device comparisons rest on, and the
rules those tests pin (lowest index at a tie, strictly greater in the stop rule, <= in the zero-feature rule, the wrap of a probe chain) flipped on the restatement to
show that the comparison notices.  No device.

The conditions are conditions, not measurements: an input that breaks one is changed (seed, place), never the cap."""
import numpy as np
import pytest

import ransac_ref as rr
import registration_edges as re_


# ---- occupancy ---------------------------------------------------------------------------------------------------------------------------------------------------------
def test_occ_hash_is_its_definition_and_gives_a_consistent_table():
    assert rr.occ_hash(0) == 0 and rr.occ_hash(1) == (0x9E3779B97F4A7C15 ^ 0x9E3779B9) & 0xFFFFFFFF
    k = (1 << 63) - 1
    h = (k * 0x9E3779B97F4A7C15) % (1 << 64)
    assert rr.occ_hash(k) == (h ^ (h >> 32)) % (1 << 32)
    assert rr.home_slot(k, 64) == rr.occ_hash(k) % 64 and rr.home_slot(k, 1 << 20) == rr.occ_hash(k) % (1 << 20)
    # the `wide` cloud of tests/test_occupancy_gpu.py: every block key is found again by the walk that stored it, at half load, and the homes spread over the table
    rng = np.random.default_rng(17)
    for n in (1, 63, 64, 65, 257):
        rng.normal(size=(n, 3))
    wide = (rng.random((5000, 3)) * [120, 120, 20] - [60, 60, 10]).astype(np.float32)
    keys = sorted({k >> 9 for k in rr.cell_keys(wide, np.eye(4), 0.5)[0]})
    assert len(keys) > 600
    slots = 64
    while slots < 2 * len(keys):
        slots *= 2
    table = rr.probe_table(keys, slots)
    assert sorted(k for k in table if k is not None) == keys
    for k in keys:  # the lookup's walk: from the home slot, wrapping, the key before a free slot
        s = rr.home_slot(k, slots)
        while table[s] != k:
            assert table[s] is not None
            s = (s + 1) % slots
    homes = np.bincount([rr.home_slot(k, slots) for k in keys], minlength=slots)
    assert homes.max() <= 6 and (homes > 0).sum() > 0.7 * len(keys) * (1 - len(keys) / (2.0 * slots))  # a multiplicative hash of packed coordinates, not a constant


@pytest.mark.parametrize("slots", [64, 128])
def test_planted_collisions_share_their_home_slots_and_wrap(slots):
    c = re_.wrap_case(slots)
    n = len(c["inserted"])
    assert n == 24 * slots // 64 and 64 <= slots and 2 * n <= slots < 4 * n  # the device sizes its table 2 n rounded up to a power of two (at least 64): `slots`
    for pts, keys in ((c["inserted"], c["keys"]), (c["same_blocks"], c["keys"]), (c["same_homes"], c["other_keys"]), (c["second"], c["second_keys"])):
        got, ok = rr.cell_keys(pts, np.eye(4), re_.RES)
        assert ok.all() and [k >> 9 for k in got] == keys and rr.band_count(pts, np.eye(4), re_.RES) == 0
    assert len(set(c["keys"]) | set(c["other_keys"]) | set(c["second_keys"])) == n + 8 + n + 8
    for table_slots in (slots, 2 * slots):
        assert all(rr.home_slot(k, table_slots) >= table_slots - 2 for k in c["keys"] + c["other_keys"])
        table = rr.probe_table(c["keys"], table_slots)
        assert table[table_slots - 2] is not None and table[table_slots - 1] is not None and all(table[s] is not None for s in range(n - 2))  # the chain wraps to slot 0
    assert 2 * (n + len(c["second"])) > slots and 2 * (n + len(c["second"])) <= 2 * slots  # the second insert doubles the table, once
    # a lookup that stops at the table's end instead of wrapping would miss every key stored behind slot 0
    table = rr.probe_table(c["keys"], slots)
    no_wrap_found = sum(k in table[rr.home_slot(k, slots):] for k in c["keys"])
    assert no_wrap_found <= 2 < n
    # a rehash that dropped the cell words would keep the blocks and lose the first cloud's cells: the count after the growth tells
    kept = rr.OccupancySet(re_.RES).insert(c["inserted"]).insert(c["second"])
    dropped = rr.OccupancySet(re_.RES).insert(c["second"])
    assert kept.calc_overlap(c["inserted"]) == n and dropped.calc_overlap(c["inserted"]) == 0


def test_growth_full_block_and_scoring_inputs():
    clouds, misses = re_.growth_clouds()
    assert [len(c) for c in clouds] == list(re_.GROWTH_SIZES) and max(re_.GROWTH_SIZES) <= 5120
    ref = rr.OccupancySet(re_.RES)
    total = 0
    for c in clouds:
        assert rr.band_count(c, np.eye(4), re_.RES) == 0
        ref.insert(c)
        total += len(c)
        assert ref.num_blocks() == total == ref.num_occupied_cells()  # one point per block, all blocks distinct
    assert rr.band_count(misses, np.eye(4), re_.RES) == 0 and ref.calc_overlap(misses) == 0
    pts, neighbour = re_.full_block()
    assert len(pts) == 4096 and rr.band_count(pts, np.eye(4), re_.RES) == 0 and rr.band_count(neighbour, np.eye(4), re_.RES) == 0
    one = rr.OccupancySet(re_.RES).insert(pts)
    assert one.num_occupied_cells() == 512 and one.num_blocks() == 1 and one.calc_overlap(neighbour) == 0 and len(neighbour) == 512
    cloud = re_.score_cloud()
    for k in range(re_.SCORE_POSES):
        assert rr.band_count(cloud, re_.score_pose(k), re_.RES) == 0
    hits = [rr.OccupancySet(re_.RES).insert(cloud).calc_overlap(cloud, re_.score_pose(k)) for k in range(re_.SCORE_POSES)]
    assert len(set(hits)) == re_.SCORE_POSES and min(hits) > 0  # the poses are told apart by their counts


def test_far_points_alias_with_near_cells_and_lie_off_the_faces():
    c = re_.alias_case()
    eye = np.eye(4)
    for name in ("far", "near", "unrelated"):
        assert rr.band_count(c[name], eye, re_.FAR_RES) == 0, name
    assert rr.band_count(c["far"], eye, 1.0) == len(c["far"])  # at a power-of-two resolution the integer-valued far points sit exactly on faces
    far, ok = rr.cell_keys(c["far"], eye, re_.FAR_RES)
    near, ok2 = rr.cell_keys(c["near"], eye, re_.FAR_RES)
    other, _ = rr.cell_keys(c["unrelated"], eye, re_.FAR_RES)
    assert ok.all() and ok2.all() and far == near and not set(other) & set(far)
    cells = np.floor(c["far"].astype(np.float64) * (1.0 / re_.FAR_RES)).astype(np.int64)
    g = cells + rr.OFFSET
    assert (g >= 1 << 24).any() and (cells < -(1 << 20)).any() and (np.abs(cells) < 2 ** 31 - 2 ** 20).all()
    assert (np.abs(c["far"]) > 1.69e7).all() and (np.abs(c["far"]) > 9.9e8).any() and (np.abs(c["near"]) < 4000).all()
    assert (g.astype(np.int32) == g).all() and ((g >> 3) & rr.MASK21 != g >> 3).all()  # inside the int, outside the 21 bits on every axis


# ---- feature matching --------------------------------------------------------------------------------------------------------------------------------------------------
def highest_at_ties(tf, sf, rows=None):
    """the flipped rule: the HIGHEST index at the minimum"""
    idx, sq, ties = rr.match_features(tf[::-1], sf, rows)
    return np.where(idx >= 0, len(tf) - 1 - idx, -1)


@pytest.mark.parametrize("d", re_.TIE_DIMS)
def test_planted_ties_are_the_only_ties(d):
    for pattern, offs in re_.TIE_PATTERNS:
        for a in re_.TIE_PLACES:
            tf, sf, group = re_.tie_case(d, pattern, a)
            idx, sq, ties = rr.match_features(tf, sf)
            planted = np.isin(np.arange(len(sf)), (0, 5, 16))
            assert (idx[planted] == a).all() and (ties[planted] == len(group)).all() and (sq[planted] > 0).all(), (pattern, a)
            assert (ties[~planted] == 1).all() or set(idx[~planted][ties[~planted] > 1].tolist()) <= {a}
            assert (highest_at_ties(tf, sf)[planted] == group[-1]).all()  # the flipped rule fails the comparison
    same = np.tile(np.float32(0.25), (130, d))
    idx, sq, ties = rr.match_features(same, np.zeros((3, d), np.float32))
    assert (idx == 0).all() and (ties == 130).all()


def test_shape_inputs_have_no_ties():
    for d in re_.SHAPE_DIMS:
        for nt in re_.SHAPE_NT:
            for nq in re_.SHAPE_NQ:
                for with_rows in (False, True):
                    tf, sf, rows, idx, sq, ties = re_.shape_case(d, nt, nq, with_rows)
                    assert (ties == 1).all() and len(idx) == nq and (sq > 0).all()


def test_value_inputs_and_the_nan_rule():
    tf, sf = re_.value_case("zero")
    idx, sq, ties = rr.match_features(tf, sf)
    assert idx[3] == 77 and idx[16] == 5 and sq[3] == 0.0 and sq[16] == 0.0 and (ties == 1).all()
    tf, sf = re_.value_case("huge")
    idx, sq, ties = rr.match_features(tf, sf)
    assert (ties == 1).all() and np.isfinite(sq).all() and sq.max() > 1e35 and idx[1] == 4 and 0 < sq[1] == float(np.float32(1e-30)) ** 2 < 1e-59
    tf, sf = re_.value_case("nan_target")
    idx, sq, ties = rr.match_features(tf, sf)
    assert not np.isin(idx, (9, 70)).any() and (ties == 1).all() and np.isfinite(sq).all()
    clean = tf.copy()
    clean[9, 3], clean[70, 6] = 0.0, 0.0
    assert rr.match_features(clean, sf)[0][2] == 9 and rr.match_features(clean, sf)[0][4] == 70  # without the NaN / inf these rows WOULD be returned
    tf, sf = re_.value_case("all_nan")
    idx, sq, ties = rr.match_features(tf, sf)
    assert np.isnan(tf).any(axis=1).all() and (idx == -1).all() and np.isposinf(sq).all()
    tf, sf = re_.value_case("nan_query")
    idx, sq, ties = rr.match_features(tf, sf)
    bad = np.isin(np.arange(17), (5, 16))
    assert (idx[bad] == -1).all() and np.isposinf(sq[bad]).all() and (idx[~bad] >= 0).all() and (ties[~bad] == 1).all()
    idx, sq, ties = rr.match_features(tf, sf, [0, -1, 17, 1])  # rows outside the source rows
    assert idx[1] == -1 and idx[2] == -1 and np.isposinf(sq[1:3]).all() and idx[0] >= 0 and idx[3] >= 0


# ---- RANSAC ------------------------------------------------------------------------------------------------------------------------------------------------------------
def conditions(c, hyp, thresholds=(0.5 * np.pi / 180.0, 0.25), poly_thresh=0.5, planted_ties=()):
    tried = np.isfinite(hyp["poly"])
    assert (np.abs(hyp["poly"][tried] - poly_thresh) > 1e-12).all()
    for it in np.flatnonzero(tried):
        assert hyp["match_ties"][it] <= 1 or it in planted_ties, it  # (0: a row without a match)
    for deltas in hyp["taboo"]:
        for a, t in deltas:
            assert abs(a - thresholds[0]) > 1e-9 * thresholds[0] and abs(t - thresholds[1]) > 1e-9 * thresholds[1]


def test_small_case_is_what_the_edge_tests_assume():
    for dof in (6, 4):
        for far in (0.0, 1e5):
            c = rr.make_small_case(dof, far)
            sf = c["source_features"]
            assert len(c["target"]) <= 512 and len(c["source"]) == 256 and sf.shape[1] == 8
            assert float(sf[rr.SMALL_ROW_1E3].astype(np.float64).max()) > 1e-3 and np.float32(1e-3) == sf[rr.SMALL_ROW_1E3, 5] and (sf[rr.SMALL_ROW_1E3] != 0).sum() == 1
            assert (sf[rr.SMALL_ROW_2M10] == 2.0 ** -10).all() and 2.0 ** -10 <= 1e-3 and np.isnan(sf[rr.SMALL_ROW_NAN]).all() and (sf[list(rr.SMALL_ZERO_ROWS)] == 0).all()
            if far:
                assert np.abs(c["target"][:, :2]).min() > 9e4 and np.abs(c["source"]).max() > 9e4
            rate, T, status, inl, hyp = re_.small_ref(dof, far, chunk_iterations=re_.EDGE_ITERATIONS, early_stop_inlier_rate=re_.NEVER_STOP)
            conditions(c, hyp)
            for s in (rr.SCORED, rr.INVALID_FEATURE, rr.POLY_REJECTED):
                assert (status == s).any(), (dof, far, s)
            alive = np.flatnonzero(status == rr.SCORED)
            assert sum(rr.rotation_bound(hyp["H"][it], dof)[0] for it in alive) >= 0.9 * len(alive)
            assert sum(rr.band_count(c["source"], hyp["poses"][it], 1.0) > 0 for it in alive) <= 1
            assert rr.taboo_delta(T, c["T_true"])[0] < (1e-3 if far else 1e-6)


def test_chunk_geometry_and_the_stop_rule_on_the_restatement():
    """what tests/test_ransac_edges_gpu.py expects of the chunks, established here; and the stop rule flipped to >=, which the equality case tells apart"""
    c = rr.make_small_case(6)
    ns = len(c["source"])
    runs = [re_.small_ref(6, chunk_iterations=ch, early_stop_inlier_rate=re_.NEVER_STOP) for ch in re_.CHUNKS]
    for r in runs:
        assert np.array_equal(r[2], runs[0][2]) and np.array_equal(r[3], runs[0][3]) and np.array_equal(r[1], runs[0][1]) and not (r[2] == rr.SKIPPED).any()
    status0, inl = runs[0][2], runs[0][3]
    best = int(inl.max())
    first = int(np.flatnonzero(status0 == rr.SCORED)[0])
    # a stop inside chunk 0: the first scored hypothesis already crosses 0.3 N_s
    assert first < 7 and inl[first] > 0.3 * ns
    status, _, _ = rr.select(status0, inl, 7, ns, 0.3)
    assert (status[7:] == rr.SKIPPED).all() and (status[:7] != rr.SKIPPED).all()
    # equality is not a stop: best / N_s is exactly representable, N_s x (best / N_s) == best
    rate = best / float(ns)
    assert ns == 256 and ns * rate == best and ns * np.nextafter(rate, 0.0) < best
    status, _, _ = rr.select(status0, inl, 7, ns, rate)
    assert not (status == rr.SKIPPED).any()
    status, _, _ = rr.select(status0, inl, 7, ns, float(np.nextafter(rate, 0.0)))
    at = int(np.flatnonzero(inl == best)[0])
    assert at < re_.EDGE_ITERATIONS - 7 and (status[(at // 7 + 1) * 7 :] == rr.SKIPPED).all() and (status[: (at // 7 + 1) * 7] != rr.SKIPPED).all()
    # `>=` instead of `>` in the stop rule: the equality run would skip the chunks behind the best hypothesis, and the comparison of the status arrays fails
    ge = rr.select(status0, np.where(inl == best, best + 1, inl), 7, ns, rate)[0]  # (inliers >= N_s rate  <=>  inliers + 1 > N_s rate at the crossing value)
    assert (ge == rr.SKIPPED).any() and not np.array_equal(ge, rr.select(status0, inl, 7, ns, rate)[0])


def test_nothing_scored_inputs():
    for dof in (6, 4):
        c = rr.make_small_case(dof)
        sf = np.full_like(c["source_features"], np.float32(2.0 ** -10))
        hyp = rr.hypotheses(c["target"], c["source"], c["target_features"], sf, re_.EDGE_ITERATIONS, dof=dof)
        assert (hyp["status"] == rr.INVALID_FEATURE).all()
        hyp = rr.hypotheses(c["target"], c["source"], c["target_features"], c["source_features"], re_.EDGE_ITERATIONS, dof=dof, poly_error_thresh=0.0)
        tried = np.isfinite(hyp["poly"])
        assert (hyp["status"][tried] == rr.POLY_REJECTED).all() and (hyp["poly"][tried] > 1e-12).all() and not (hyp["status"] == rr.SCORED).any()
        # every aligned hypothesis' own pose on the list: each is within the thresholds of itself (delta = identity up to rounding), none near a threshold
        first = rr.hypotheses(c["target"], c["source"], c["target_features"], c["source_features"], re_.EDGE_ITERATIONS, dof=dof)
        own = [first["poses"][it] for it in np.flatnonzero(first["status"] == rr.SCORED)]
        assert 1 <= len(own) <= 64
        hyp = rr.hypotheses(c["target"], c["source"], c["target_features"], c["source_features"], re_.EDGE_ITERATIONS, dof=dof, taboo_list=tuple(own))
        conditions(c, hyp)
        assert not (hyp["status"] == rr.SCORED).any() and (hyp["status"] == rr.TABOO).sum() == len(own)


def test_boundary_samples_hit_their_rows():
    for dof in (6, 4):
        c = rr.make_small_case(dof)
        given = re_.boundary_samples(dof)
        hyp = rr.hypotheses(c["target"], c["source"], c["target_features"], c["source_features"], len(given), dof=dof, sample_indices=given)
        conditions(c, hyp)
        s = hyp["status"]
        assert (s[0:4] != rr.INVALID_FEATURE).all() and (s[4:8] == rr.INVALID_FEATURE).all() and (s[8:12] != rr.INVALID_FEATURE).all() and (s[12:16] == rr.INVALID_FEATURE).all()
        assert (s[16:] == rr.SCORED).all() and len(s) == 20
        samples = 3 if dof == 6 else 2
        for it in range(8, 12):  # the NaN row: no match, target 0
            assert hyp["target_indices"][it, it % samples] == 0 and given[it, it % samples] == rr.SMALL_ROW_NAN
        # `<` for `<=` cannot be told apart (no f32 value widens to exactly 1e-3); the rule in f32 arithmetic (|f| <= 1e-3f) would call the float32(1e-3) row zero:
        assert np.float32(1e-3) <= np.float32(1e-3) and not float(np.float32(1e-3)) <= 1e-3


def test_taboo_inputs():
    c = rr.make_small_case(6)
    _, T, _, _, _ = re_.small_ref(6, chunk_iterations=re_.EDGE_ITERATIONS, early_stop_inlier_rate=re_.NEVER_STOP)
    decoys = re_.decoy_poses(63)
    hyp = rr.hypotheses(c["target"], c["source"], c["target_features"], c["source_features"], re_.EDGE_ITERATIONS, dof=6, taboo_list=tuple(decoys) + (T,))
    conditions(c, hyp)
    only_decoys = rr.hypotheses(c["target"], c["source"], c["target_features"], c["source_features"], re_.EDGE_ITERATIONS, dof=6, taboo_list=tuple(decoys))
    assert not (only_decoys["status"] == rr.TABOO).any() and (hyp["status"] == rr.TABOO).sum() >= 1 and (hyp["status"] == rr.SCORED).sum() >= 1
    for it in np.flatnonzero(hyp["status"] == rr.TABOO):  # only the last pose of the list matches: a loop that ends one pose early would miss every one
        hits = [a < 0.5 * np.pi / 180.0 and t < 0.25 for a, t in hyp["taboo"][it]]
        assert hits[-1] and not any(hits[:-1])


def test_degenerate_samples_are_degenerate():
    c = re_.degenerate_cloud()
    src, tgt = c["source"].astype(np.float64), c["target"].astype(np.float64)
    idx, _, ties = rr.match_features(c["target_features"], c["source_features"])
    assert np.array_equal(idx, np.arange(len(src))) and (ties == 1).all()
    assert np.array_equal(tgt[0], tgt[1]) and np.array_equal(tgt[0], tgt[2]) and np.array_equal(tgt[5, :2], tgt[0, :2]) and tgt[5, 2] != tgt[0, 2]
    for dof, sample, what in re_.DEGENERATE_SAMPLES:
        k = 3 if dof == 6 else 2
        s, t = src[list(sample[:k])], tgt[list(sample[:k])]
        assert rr.poly_error(t, s) < 1e-6, what  # far below the threshold 0.5
        H, mt, ms = rr.cross_covariance(t, s)
        assert not rr.rotation_bound(H, dof)[0], what
        if "H = 0" in what:
            assert (H == 0).all()
        if "columns" in what:
            assert (H[:, 1:] == 0).all() and (H[:, 0] != 0).any()
        if dof == 4 and "2x2" in what:
            assert (H[:2, :2] == 0).all() and H[2, 2] != 0
        T = rr.pose_from(H, mt, ms, dof)  # the restatement's pose is a minimiser: no rigid pose of the family does better than the sample allows
        assert rr.alignment_residual(T, s, t) < 1e-9


def test_alignment_inputs():
    for dof in (6, 4):
        for n in re_.ALIGN_SIZES:
            t, s, w = re_.align_case(dof, n)
            keep = w != 0
            assert 0.3 * n < (~keep).sum() < 0.4 * n
            H, _, _ = rr.cross_covariance(t[keep], s[keep], w[keep])
            assert rr.rotation_bound(H, dof)[0]
            full = (rr.align_points_se3 if dof == 6 else rr.align_points_4dof)(t, s, w)
            sub = (rr.align_points_se3 if dof == 6 else rr.align_points_4dof)(t[keep], s[keep], w[keep])
            assert np.abs(full - sub).max() < 1e-12  # zero weights do not count; a sum that ignored the weights would be off by metres
            unweighted = (rr.align_points_se3 if dof == 6 else rr.align_points_4dof)(t, s, np.ones(n))
            assert np.abs(unweighted - sub).max() > 1e-3

"""tests/ransac_ref.py held to what it restates (no device), and the inputs of tests/test_ransac_gpu.py held to the conditions its exact comparisons rest on.

The conditions are conditions, not measurements: an input that breaks one is changed (seed, pose), never the cap."""
import functools

import numpy as np

import ransac_ref as rr


def test_generator_matches_the_library_bit_for_bit():
    """gp_ransac_sample_index (host code) is the function the sampling kernel calls"""
    from gtsam_points_amd import _capi

    lib = _capi.load()
    for seed in (0, 1, 5489, 2**63 + 12345, 2**64 - 1):
        for it in (0, 1, 255, 4999, 2**31):
            for draw in (0, 1, 2, 66):
                for n in (1, 2, 3, 2048, 124668, 2**31 - 1):
                    assert lib.gp_ransac_sample_index(seed, it, draw, n) == rr.sample_index(seed, it, draw, n) < n
    assert len(set(rr.draw_samples(7, 3, 3, 3))) == 3 and sorted(rr.draw_samples(7, 3, 3, 3)) == [0, 1, 2]
    assert rr.draw_samples(7, 3, 2, 3) is None  # three distinct indices out of two: 64 redraws, then the failure
    counts = np.bincount([rr.sample_index(5489, it, 0, 10) for it in range(20000)], minlength=10)
    assert counts.min() > 1800 and counts.max() < 2200  # uniform to a few sigma (sigma = 42)


def test_alignment_recovers_a_known_transform():
    rng = np.random.default_rng(3)
    for dof in (6, 4):
        T = np.eye(4)
        T[:3, :3] = rr.rot([0.3, 0.5, -1.0], 0.8) if dof == 6 else rr.rot([0, 0, 1], -2.1)
        T[:3, 3] = [1.0, -4.0, 0.3]
        for n in (3 if dof == 6 else 2, 10, 200):
            s = rng.normal(size=(n, 3)) * 5
            t = s @ T[:3, :3].T + T[:3, 3]
            w = None if n <= 3 else rng.random(n) + 0.1
            got = (rr.align_points_se3 if dof == 6 else rr.align_points_4dof)(t, s, w)
            assert np.abs(got - T).max() < 1e-12, (dof, n)


def test_alignment_returns_a_proper_rotation_for_a_mirrored_triplet():
    """t = mirror image of s: the SVD's U V^T is a reflection, the det(U) det(V) < 0 branch (alignment.cpp:30-33) turns it into the nearest rotation"""
    s = np.array([[1.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, 3.0], [1.0, 1.0, 1.0]])
    t = s * np.array([1.0, 1.0, -1.0])
    H, _, _ = rr.cross_covariance(t, s)
    U, _, Vt = np.linalg.svd(H)
    assert np.linalg.det(U) * np.linalg.det(Vt) < 0
    R = rr.align_points_se3(t, s)[:3, :3]
    assert abs(np.linalg.det(R) - 1.0) < 1e-12 and np.abs(R @ R.T - np.eye(3)).max() < 1e-12
    R3 = rr.align_points_se3(t[:3], s[:3])[:3, :3]  # three points are always coplanar with their mirror image: a rotation maps them exactly
    assert abs(np.linalg.det(R3) - 1.0) < 1e-12


def test_occupancy_counts_equal_a_direct_cell_set_count():
    rng = np.random.default_rng(5)
    pts = (rng.random((3000, 3)) * 40 - 20).astype(np.float32)  # negative coordinates included
    T = np.eye(4)
    T[:3, :3] = rr.rot([1, 2, 3], 0.4)
    T[:3, 3] = [0.5, -7.0, 2.0]
    for res in (1.0, 0.37):
        g = rr.OccupancySet(res).insert(pts)
        direct = {tuple(c) for c in np.floor(pts.astype(np.float64) * (1.0 / res)).astype(np.int64).tolist()}
        assert g.num_occupied_cells() == len(direct)
        q = rr.transform(pts, T)
        want = sum(tuple(c) in direct for c in np.floor(q * (1.0 / res)).astype(np.int64).tolist())
        assert g.calc_overlap(pts, T) == want == int(g.get_overlaps(pts, T).sum())
        assert g.calc_overlap(pts) == len(pts)


def test_occupancy_negative_coordinates_and_the_block_boundary():
    g = rr.OccupancySet(1.0).insert(np.array([[7.5, 0.5, 0.5], [8.5, 0.5, 0.5], [-0.5, -0.5, -0.5], [-8.5, 0.5, 0.5]], np.float32))
    assert g.num_occupied_cells() == 4 and g.num_blocks() == 4  # cells 7 and 8 lie in different blocks, so do -1 and 0, -9 and -8
    keys, ok = rr.cell_keys(np.array([[7.5, 0.5, 0.5], [8.5, 0.5, 0.5]], np.float32), np.eye(4), 1.0)
    assert ok.all() and keys[0] >> 9 != keys[1] >> 9 and keys[0] & 511 == 7 and keys[1] & 511 == 0
    probe = np.array([[7.99, 0.0, 0.0], [8.0, 0.99, 0.99], [9.0, 0.5, 0.5], [-0.01, -1.0, -0.25], [-1.01, -0.5, -0.5], [0.0, 0.0, 0.0], [-8.01, 0.5, 0.5], [np.nan, 0, 0]], np.float32)
    assert g.get_overlaps(probe).tolist() == [1, 1, 0, 1, 0, 0, 1, 0]
    g.insert(np.array([[0.25, 0.25, 0.25]], np.float32))  # the union
    assert g.num_occupied_cells() == 5 and g.get_overlaps(probe).tolist() == [1, 1, 0, 1, 0, 1, 1, 0]


def test_selection_ties_and_the_chunk_after_the_crossing():
    S, P = rr.SCORED, rr.POLY_REJECTED
    status = [S, P, S, S, S, S, S, S]
    inl = [5, -1, 9, 9, 3, 50, 50, 1]
    got, it, best = rr.select(status, inl, 8, 100, 0.8)
    assert got.tolist() == status and (it, best) == (5, 50)  # the tie at 50 goes to iteration 5, nothing crosses 80
    got, it, best = rr.select(status, inl, 2, 100, 0.08)  # 9 > 8 in chunk 1 (iterations 2, 3): chunks 2 and 3 are skipped
    assert got.tolist() == [S, P, S, S] + [rr.SKIPPED] * 4 and (it, best) == (2, 9)
    got, it, best = rr.select(status, inl, 3, 100, 0.08)  # the crossing in chunk 0 (iteration 2): iterations 3 .. 5 would have held a better one
    assert got.tolist() == [S, P, S] + [rr.SKIPPED] * 5 and (it, best) == (2, 9)
    got, it, best = rr.select([P, P], [-1, -1], 1, 10, 0.5)
    assert (it, best) == (-1, 0)
    got, it, best = rr.select([S, S], [0, 0], 1, 10, 0.5)
    assert (it, best) == (0, 0)  # a scored hypothesis without inliers still is the result


@functools.lru_cache(maxsize=None)
def case_run(dof):
    c = rr.make_case(dof)
    return rr.estimate_pose_ransac(c["target"], c["source"], c["target_features"], c["source_features"], rr.CASE_ITERATIONS, dof=dof)


def _conditions(c, hyp, dof, taboo_thresholds=(0.5 * np.pi / 180.0, 0.25), poly_thresh=0.5):
    tried = np.isfinite(hyp["poly"])
    assert tried.sum() > 100
    assert (np.abs(hyp["poly"][tried] - poly_thresh) > 1e-12).all()
    assert (hyp["match_ties"][tried] == 1).all()
    for deltas in hyp["taboo"]:
        for a, t in deltas:
            assert abs(a - taboo_thresholds[0]) > 1e-9 * taboo_thresholds[0] and abs(t - taboo_thresholds[1]) > 1e-9 * taboo_thresholds[1]
    alive = np.flatnonzero((hyp["status"] == rr.SCORED) | (hyp["status"] == rr.TABOO))
    assert len(alive) >= 20
    conditioned = sum(rr.rotation_bound(hyp["H"][it], dof)[0] for it in alive)
    assert conditioned >= 0.9 * len(alive)
    in_band = sum(rr.band_count(c["source"], hyp["poses"][it], 1.0) > 0 for it in alive)
    assert in_band <= 0.01 * len(alive)


def test_inputs_of_the_gpu_tests_meet_their_conditions():
    for dof in (6, 4):
        c = rr.make_case(dof)
        rate, T, status, inl, hyp = case_run(dof)
        _conditions(c, hyp, dof)
        assert (hyp["status"] == rr.INVALID_FEATURE).sum() >= 1 and (hyp["status"] == rr.POLY_REJECTED).sum() >= 10
        # the restatement finds the pose the source was moved by
        d = rr.pose_inverse(c["T_true"]) @ T
        assert rr.taboo_delta(T, c["T_true"])[0] < 0.5 * np.pi / 180.0 and np.linalg.norm(d[:3, 3]) < 0.25
        assert rate == inl.max() / float(len(c["target"])) and len(c["target"]) <= 4096


def test_taboo_input_meets_its_conditions():
    """the GPU test puts the device's first result on the taboo list; it differs from this restatement's by rounding only, far inside the 1e-9 margins"""
    c = rr.make_case(6)
    _, T, _, _, _ = case_run(6)
    hyp = rr.hypotheses(c["target"], c["source"], c["target_features"], c["source_features"], rr.CASE_ITERATIONS, dof=6, taboo_list=(T,))
    _conditions(c, hyp, 6)
    assert (hyp["status"] == rr.TABOO).sum() >= 1 and (hyp["status"] == rr.SCORED).sum() >= 1

"""Fast global registration on the device against tests/gnc_ref.py, the f64 restatement of the reference (tests/test_gnc_ref_cpu.py holds the restatement and the
conditions the exact comparisons here rest on).  Correspondences and tuple-test survivors are compared as integer arrays; every traced alignment is held to the rounding
of ONE alignment (the restatement starts from the device's own previous pose); counts, the schedule of mu and the inlier counts are exact."""
import numpy as np
import pytest

import gnc_ref as G
import ransac_ref as R

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def gpa():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import gtsam_points_amd

    return gtsam_points_amd


def _gp(gpa, p):
    return gpa.GNCParams(**p)


def _clouds(gpa, target, source):
    return gpa.PointCloudGPU(np.ascontiguousarray(target)), gpa.PointCloudGPU(np.ascontiguousarray(source))


def _pairs(gpa, target, source, tf, sf, p, query_indices=None):
    t, s = _clouds(gpa, target, source)
    return gpa.find_feature_correspondences_gpu(t, s, tf, sf, _gp(gpa, p), query_indices=query_indices).cpu().numpy().astype(np.int64)


def _trace(tr):
    return dict(mu=tr.mu.cpu().numpy(), sum_weights=tr.sum_weights.cpu().numpy(), sum_errors=tr.sum_errors.cpu().numpy(), num_inliers=tr.num_inliers.cpu().numpy(),
                poses=tr.poses.cpu().numpy().reshape(-1, 4, 4).transpose(0, 2, 1))


def _check_steps(target, source, pairs, p, res, tr):
    """every traced alignment against the restatement's alignment from the DEVICE's previous pose"""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    n = len(pairs)
    t = np.asarray(target, np.float32).astype(np.float64)[pairs[:, 0]]
    s = np.asarray(source, np.float32).astype(np.float64)[pairs[:, 1]]
    sched, final_mu = G.schedule(G.diameter(target), p)
    d = _trace(tr)
    assert res.num_alignments == len(sched) == len(d["mu"]) and res.final_mu == final_mu and res.num_correspondences == n
    T = np.eye(4)
    worst = 0.0
    for k, (outer, mu) in enumerate(sched):
        st = G.align_step(t, s, T, mu, outer, p)
        assert d["mu"][k] == mu, k
        assert d["num_inliers"][k] == st["num_inliers"], k
        assert abs(d["sum_weights"][k] - st["sum_weights"]) <= n * EPS * st["sum_weights"], k
        assert abs(d["sum_errors"][k] - st["sum_errors"]) <= n * EPS * st["sum_errors"], k
        ok, bound = R.rotation_bound(st["H"], p["dof"])
        assert ok, k
        bound += n * EPS
        dR = np.linalg.norm(d["poses"][k][:3, :3] - st["T"][:3, :3])
        dt = np.linalg.norm(d["poses"][k][:3, 3] - st["T"][:3, 3])
        assert dR <= bound, (k, dR, bound)
        assert dt <= bound * (20.0 + np.linalg.norm(st["mean_s"])), (k, dt, bound)
        assert (d["poses"][k][3] == [0, 0, 0, 1]).all()
        worst = max(worst, dR / bound)
        T = d["poses"][k]
    assert (res.T_target_source == T).all()
    assert res.inlier_rate == d["num_inliers"][-1] / float(n)
    return worst


# ---- correspondences -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("recip", [True, False])
def test_correspondences_equal_the_restatement(gpa, recip):
    c = R.make_small_case(6)
    tf, sf = c["target_features"], c["source_features"]
    p = G.params(reciprocal_check=recip)
    # the source is the smaller cloud: it queries.  The NaN row has no pair; the all-zero rows match like any other (GNC has no invalid-feature rule)
    ref = G.find_correspondences(tf, sf, p)
    got = _pairs(gpa, c["target"], c["source"], tf, sf, p)
    assert not ref["swapped"] and (got == ref["pairs"]).all() and len(got) == (205 if recip else 255)
    assert R.SMALL_ROW_NAN not in got[:, 1]
    if not recip:
        assert set(R.SMALL_ZERO_ROWS) <= set(got[:, 1].tolist())
    # the clouds the other way round: the swap branch (:78-79), pairs still (target, source)
    ref = G.find_correspondences(sf, tf, p)
    got = _pairs(gpa, c["source"], c["target"], sf, tf, p)
    assert ref["swapped"] and (got == ref["pairs"]).all() and len(got) == (205 if recip else 255) and (np.diff(got[:, 0]) > 0).all()
    # equal sizes are the swap branch too: the target rows query
    ref = G.find_correspondences(tf[:256], sf, p)
    got = _pairs(gpa, c["target"][:256], c["source"], tf[:256], sf, p)
    assert ref["swapped"] and (got == ref["pairs"]).all() and len(got) > 50 and (np.diff(got[:, 0]) > 0).all()


@pytest.mark.parametrize("k", [100, 255])
def test_subsampled_queries_equal_the_restatement(gpa, k):
    c = R.make_small_case(6)
    tf, sf = c["target_features"], c["source_features"]
    for recip in (True, False):
        p = G.params(reciprocal_check=recip, max_init_samples=k)
        ref = G.find_correspondences(tf, sf, p)
        assert len(ref["rows"]) == k and (np.diff(ref["rows"]) > 0).all()
        got = _pairs(gpa, c["target"], c["source"], tf, sf, p)
        assert (got == ref["pairs"]).all() and len(got) > k // 2
    other = _pairs(gpa, c["target"], c["source"], tf, sf, G.params(reciprocal_check=False, max_init_samples=100, seed=7))
    if k == 100:
        assert other.shape != got.shape or (other != got).any()  # another seed, another sample
    rows = np.array([0, 5, 29, 30, 31, 200, 255])  # the caller's queries, the NaN row among them
    ref = G.find_correspondences(tf, sf, G.params(reciprocal_check=False), query_indices=rows)
    got = _pairs(gpa, c["target"], c["source"], tf, sf, G.params(reciprocal_check=False), query_indices=rows)
    assert (got == ref["pairs"]).all() and got[:, 1].tolist() == [0, 5, 29, 31, 200, 255]
    t, s = _clouds(gpa, c["target"], c["source"])
    with pytest.raises(IndexError):
        gpa.find_feature_correspondences_gpu(t, s, tf, sf, gpa.GNCParams(), query_indices=[0, 256])
    with pytest.raises(gpa.GPError):
        gpa.find_feature_correspondences_gpu(t, s, tf, sf, gpa.GNCParams(), query_indices=[3, 3])


@pytest.mark.parametrize("small,tuples", [(True, 50), (False, 300)])
def test_tuple_test_survivors_equal_the_restatement(gpa, small, tuples):
    c, _, out = G.case_result(small, 6, True)
    tf, sf = c["target_features"], c["source_features"]
    p = G.params(tuple_check=True, max_num_tuples=tuples)
    assert len(out["pairs"]) > 3 * tuples
    ref = G.tuple_test(c["target"], c["source"], out["pairs"], p)
    got = _pairs(gpa, c["target"], c["source"], tf, sf, p)
    assert (got == ref).all() and 3 <= len(got) < len(out["pairs"]) and (np.diff(got[:, 1]) > 0).all()
    # count <= 3 max_num_tuples: the stage is skipped (:91)
    p = G.params(tuple_check=True, max_num_tuples=(len(out["pairs"]) + 2) // 3)
    assert (_pairs(gpa, c["target"], c["source"], tf, sf, p) == out["pairs"]).all()


def test_tuple_test_keeps_the_lowest_target_of_a_source(gpa):
    """the swapped direction without the reciprocal check: several target rows (the queries) share one source row.  Planted: 60 query rows repeat another's features."""
    c = R.make_small_case(6)
    target, source, sf = c["source"], c["target"], c["target_features"]  # (the clouds the other way round: the 256 rows are the target and query)
    tf = c["source_features"].copy()
    good = np.flatnonzero(c["good"] & ~np.isin(np.arange(256), list(R.SMALL_ZERO_ROWS) + [R.SMALL_ROW_1E3, R.SMALL_ROW_2M10, R.SMALL_ROW_NAN]))
    tf[good[1:121:2]] = tf[good[0:120:2]]
    p = G.params(reciprocal_check=False, tuple_check=True, max_num_tuples=80, tuple_thresh=0.125)
    before = G.find_correspondences(tf, sf, p)
    assert before["swapped"] and len(before["pairs"]) > 240
    idx, ratios = G.tuple_ratios(target, source, before["pairs"], 80, p["seed"])
    r = ratios[np.isfinite(ratios)]
    assert (np.abs(r - 0.125) > 1e-9).all() and (np.abs(r - 8.0) > 1e-9).all()
    with np.errstate(invalid="ignore"):
        valid = ~((ratios < 0.125) | (ratios > 8.0)).any(axis=1)
    chosen = np.unique(before["pairs"][idx[valid].reshape(-1)], axis=0)
    contested = [s for s in np.unique(chosen[:, 1]) if (chosen[:, 1] == s).sum() > 1]
    assert contested, "no source is held by two chosen pairs with different targets: the example shows nothing"
    ref = G.tuple_test(target, source, before["pairs"], p)
    got = _pairs(gpa, target, source, tf, sf, p)
    assert (got == ref).all() and (np.diff(got[:, 1]) > 0).all()
    for s in contested:
        assert got[got[:, 1] == s, 0][0] == chosen[chosen[:, 1] == s, 0].min()


# ---- the loop ----------------------------------------------------------------------------------------------------------------------------------------------------------
ROWS = [(small, dof, recip) for small in (True, False) for dof in (6, 4) for recip in (True, False)]


@pytest.mark.parametrize("small,dof,recip", ROWS)
def test_end_to_end_and_every_step(gpa, small, dof, recip):
    c, p, ref = G.case_result(small, dof, recip)
    t, s = _clouds(gpa, c["target"], c["source"])
    res, tr, pairs = gpa.estimate_pose_gnc_gpu(t, s, c["target_features"], c["source_features"], _gp(gpa, p), return_trace=True, return_pairs=True)
    pairs = pairs.cpu().numpy().astype(np.int64)
    assert (pairs == ref["pairs"]).all() and res.num_initial == len(c["source"]) and not res.swapped
    assert res.num_alignments == ref["num_alignments"] == (57 if small else 60) and res.final_mu == ref["final_mu"]
    worst = _check_steps(c["target"], c["source"], pairs, p, res, tr)
    dR, dt = G.pose_error(res.T_target_source, c["T_true"])
    print(f"small={small} dof={dof} reciprocal={recip}: pairs {len(pairs)} alignments {res.num_alignments} dR {dR:.1e} dt {dt:.1e} worst step dR / bound {worst:.2e}")
    assert dR < 1e-4 and dt < 1e-3
    assert abs(res.inlier_rate - ref["inlier_rate"]) <= 1.0 / len(pairs)
    if dof == 4:
        assert (res.T_target_source[2, :3] == [0, 0, 1]).all() and (res.T_target_source[:2, 2] == 0).all()
    plain = gpa.estimate_pose_gnc_gpu(t, s, c["target_features"], c["source_features"], _gp(gpa, p))  # without trace and pairs: the same bits
    assert (plain.T_target_source == res.T_target_source).all() and plain.inlier_rate == res.inlier_rate and plain.num_correspondences == len(pairs)


@pytest.mark.parametrize("kw", [dict(max_iterations=1), dict(max_corr_dist=None), dict(inner_iterations=1), dict(inner_iterations=5, div_factor=3.0, max_iterations=4)])
def test_alignment_count_and_final_mu_follow_the_schedule(gpa, kw):
    c, _, ref = G.case_result(True, 6, True)
    mu0 = G.diameter(c["target"])
    if "max_corr_dist" in kw:
        kw = dict(max_corr_dist=0.8 * mu0)  # above mu0 / div_factor: exactly one outer iteration
    p = G.params(**kw)
    sched, _ = G.schedule(mu0, p)
    if "max_corr_dist" in kw:
        assert mu0 / p["div_factor"] < kw["max_corr_dist"] < mu0 and len(sched) == 3
    if kw == dict(max_iterations=1):
        assert len(sched) == 3
    t, s = _clouds(gpa, c["target"], c["source"])
    res, tr = gpa.gnc_align_correspondences_gpu(t, s, ref["pairs"], _gp(gpa, p), return_trace=True)
    _check_steps(c["target"], c["source"], ref["pairs"], p, res, tr)


def test_same_seed_same_bits(gpa):
    c = R.make_small_case(6)
    t, s = _clouds(gpa, c["target"], c["source"])
    p = gpa.GNCParams(max_init_samples=100, tuple_check=True, max_num_tuples=20)
    runs = [gpa.estimate_pose_gnc_gpu(t, s, c["target_features"], c["source_features"], p, return_trace=True, return_pairs=True) for _ in range(2)]
    (a, ta, pa), (b, tb, pb) = runs
    assert a.T_target_source.tobytes() == b.T_target_source.tobytes() and a.inlier_rate == b.inlier_rate and a.num_alignments == b.num_alignments > 0
    assert (pa == pb).all() and 3 <= len(pa) <= 60
    for x, y in zip((ta.mu, ta.sum_weights, ta.sum_errors, ta.num_inliers, ta.poses), (tb.mu, tb.sum_weights, tb.sum_errors, tb.num_inliers, tb.poses)):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    p.seed = 6
    _, pc = gpa.estimate_pose_gnc_gpu(t, s, c["target_features"], c["source_features"], p, return_pairs=True)
    assert pc.shape != pa.shape or bool((pc != pa).any())


# ---- edges of gnc_align_correspondences_gpu ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2])
def test_one_and_two_pairs_give_a_rigid_pose(gpa, n):
    c, _, ref = G.case_result(True, 6, True)
    pairs = ref["pairs"][[3, 40][:n]]
    t, s = _clouds(gpa, c["target"], c["source"])
    for dof in (6, 4):
        res, tr = gpa.gnc_align_correspondences_gpu(t, s, pairs, gpa.GNCParams(dof=dof), return_trace=True)
        T = res.T_target_source
        assert res.num_alignments == 57 and np.isfinite(T).all()
        assert np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(T[:3, :3]) - 1.0) < 1e-14
        tp, sp = c["target"].astype(np.float64)[pairs[:, 0]], c["source"].astype(np.float64)[pairs[:, 1]]
        st = G.align_step(tp, sp, _trace(tr)["poses"][-2], _trace(tr)["mu"][-1], 18, G.params(dof=dof))
        assert np.abs(T[:3, 3] - (st["mean_t"] - T[:3, :3] @ st["mean_s"])).max() <= 1e-12 * (20.0 + np.linalg.norm(st["mean_s"]))


@pytest.mark.parametrize("n", [255, 256, 257])
def test_stride_and_tree_boundaries(gpa, n):
    c, _, ref = G.case_result(False, 6, True)
    pairs = ref["pairs"][:n]
    p = G.params(max_iterations=6)
    t, s = _clouds(gpa, c["target"], c["source"])
    res, tr = gpa.gnc_align_correspondences_gpu(t, s, pairs, _gp(gpa, p), return_trace=True)
    _check_steps(c["target"], c["source"], pairs, p, res, tr)


def test_identical_points_empty_pairs_and_bad_indices(gpa):
    c, _, ref = G.case_result(True, 6, True)
    t, s = _clouds(gpa, c["target"], c["source"])
    res, tr = gpa.gnc_align_correspondences_gpu(t, s, np.tile(ref["pairs"][7], (40, 1)), gpa.GNCParams(), return_trace=True)  # H = 0 up to rounding: any rotation, about the one point
    T, d = res.T_target_source, _trace(tr)
    assert res.num_alignments == 57 and np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(T[:3, :3]) - 1.0) < 1e-14
    assert np.abs(T[:3, :3] @ c["source"][ref["pairs"][7, 1]].astype(np.float64) + T[:3, 3] - c["target"][ref["pairs"][7, 0]].astype(np.float64)).max() < 1e-10
    assert d["num_inliers"][0] == 0 and d["num_inliers"][-1] == 40 and res.inlier_rate == 1.0
    with pytest.raises(IndexError):
        gpa.gnc_align_correspondences_gpu(t, s, [[0, 256]], gpa.GNCParams())
    with pytest.raises(IndexError):
        gpa.gnc_align_correspondences_gpu(t, s, [[512, 0]], gpa.GNCParams())
    res, tr = gpa.gnc_align_correspondences_gpu(t, s, np.zeros((0, 2), np.int32), gpa.GNCParams(), return_trace=True)
    assert (res.T_target_source == np.eye(4)).all() and res.inlier_rate == 0.0 and res.num_alignments == 0 and res.num_correspondences == 0 and len(tr.mu) == 0
    # ... and features none of which matches (every query row NaN): no correspondences, no fault, and the device goes on working
    nan = np.full_like(c["source_features"], np.nan)
    res = gpa.estimate_pose_gnc_gpu(t, s, c["target_features"], nan, gpa.GNCParams())
    assert (res.T_target_source == np.eye(4)).all() and res.inlier_rate == 0.0 and res.num_correspondences == 0 and res.num_initial == 256 and res.num_alignments == 0
    again = gpa.gnc_align_correspondences_gpu(t, s, ref["pairs"], gpa.GNCParams())
    assert again.num_alignments == 57 and G.pose_error(again.T_target_source, c["T_true"])[0] < 1e-4


def test_far_from_the_origin(gpa):
    c, p, ref = G.case_result(True, 6, True, far=1e4)
    t, s = _clouds(gpa, c["target"], c["source"])
    res, tr = gpa.gnc_align_correspondences_gpu(t, s, ref["pairs"], _gp(gpa, p), return_trace=True)
    _check_steps(c["target"], c["source"], ref["pairs"], p, res, tr)


def test_refusals_raise(gpa):
    c = R.make_small_case(6)
    t, s = _clouds(gpa, c["target"], c["source"])
    tf, sf = c["target_features"], c["source_features"]
    with pytest.raises(gpa.GPError, match="dof"):
        gpa.estimate_pose_gnc_gpu(t, s, tf, sf, gpa.GNCParams(dof=5))
    with pytest.raises(gpa.GPError, match="129"):
        gpa.estimate_pose_gnc_gpu(t, s, np.zeros((512, 129), np.float32), np.zeros((256, 129), np.float32))
    with pytest.raises(gpa.GPError, match="one feature row per point"):
        gpa.estimate_pose_gnc_gpu(t, s, tf[:500], sf)
    with pytest.raises(gpa.GPError, match="div_factor"):
        gpa.gnc_align_correspondences_gpu(t, s, [[0, 0]], gpa.GNCParams(div_factor=1.0))

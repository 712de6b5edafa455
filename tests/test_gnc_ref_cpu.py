"""CPU checks of tests/gnc_ref.py, the f64 restatement that tests/test_gnc_gpu.py compares the device with: the subsampling rule, the reference's shadowed-variable
weight rule on an example worked by hand, convergence to the true pose on the inputs of the GPU tests, and the conditions the exact GPU comparisons rest on."""
import numpy as np
import pytest

import gnc_ref as G
import ransac_ref as R

ROWS = [(small, dof, recip) for small in (False, True) for dof in (6, 4) for recip in (True, False)]


@pytest.mark.parametrize("n,k", [(101, 100), (199, 100), (124668, 5000), (7, 7), (5001, 5000)])
def test_stratified_sample_is_k_distinct_ascending_indices(n, k):
    for seed in (5489, 1):
        idx = G.stratified_sample(seed, n, k)
        assert len(idx) == k and idx[0] >= 0 and idx[-1] < n and (np.diff(idx) > 0).all()
    if n > k + 1:
        assert (G.stratified_sample(5489, n, k) != G.stratified_sample(1, n, k)).any()
    else:
        assert k < n or (G.stratified_sample(5489, n, k) == np.arange(n)).all()


def test_shadowed_variable_forces_the_weight_of_pair_zero_in_outer_iteration_zero_only():
    """impl :150 / :158 / :165.  Three pairs, T = identity, mu = 1: e = (1, 1, 0), so (mu / (mu + e))^2 = (1/4, 1/4, 1).  With the correspondence index shadowing the
    inner iteration, pair 0's weight is 1 during outer iteration 0 -- in BOTH of its inner iterations -- and 1/4 afterwards: sum_weights = 1 + 1/4 + 1 = 9/4, the
    weighted means (1 t0 + 1/4 t1 + 1 t2) / (9/4).  (Read without the shadowing, the rule would force every weight of the first alignment: sum 3; without the rule: 3/2.)"""
    t = np.array([[1, 0, 0], [0, 2, 0], [0, 0, 0]], np.float64)
    s = np.array([[0, 0, 0], [0, 1, 0], [0, 0, 0]], np.float32)
    e, w = G.errors_and_weights(t, s, np.eye(4), 1.0, outer=0)
    assert e.tolist() == [1.0, 1.0, 0.0] and w.tolist() == [1.0, 0.25, 1.0]
    e, w = G.errors_and_weights(t, s, np.eye(4), 1.0, outer=1)
    assert w.tolist() == [0.25, 0.25, 1.0]
    p = G.params(max_iterations=2, inner_iterations=2, max_corr_dist=0.01, div_factor=2.0)
    st = G.align_step(t, s.astype(np.float64), np.eye(4), 1.0, 0, p)
    assert st["sum_weights"] == 2.25 and st["sum_errors"] == 2.0 and st["num_inliers"] == 1  # (2 x 0.01)^2 = 4e-4: only e = 0 is below
    assert np.allclose(st["mean_t"], [1 / 2.25, 0.5 / 2.25, 0.0], rtol=0, atol=1e-16) and np.allclose(st["mean_s"], [0.0, 0.25 / 2.25, 0.0], rtol=0, atol=1e-16)
    out = G.gnc_loop(t.astype(np.float32), s, [[0, 0], [1, 1], [2, 2]], p, mu0=1.0)
    assert out["num_alignments"] == 4 and [x["outer"] for x in out["steps"]] == [0, 0, 1, 1] and [x["mu"] for x in out["steps"]] == [1.0, 1.0, 0.5, 0.5]
    assert [x["w"][0] == 1.0 for x in out["steps"]] == [True, True, False, False]
    assert out["steps"][0]["sum_weights"] == 2.25 and out["final_mu"] == 0.25


def test_schedule_follows_the_reference_loop():
    p = G.params()
    sched, final = G.schedule(100.0, p)
    mu, n = 100.0, 0
    while True:
        n += 1
        mu /= 1.4
        if mu < 0.25 or n == 64:
            break
    assert len(sched) == 3 * n and final == mu and sched[0] == (0, 100.0) and sched[3] == (1, 100.0 / 1.4)
    assert len(G.schedule(100.0, G.params(max_iterations=1))[0]) == 3
    assert len(G.schedule(100.0, G.params(max_corr_dist=100.0 / 1.4 + 1.0))[0]) == 3  # above mu0 / div_factor: one outer iteration
    assert len(G.schedule(1e30, G.params())[0]) == 192


def test_numpy_sums_agree_with_the_serial_cross_covariance():
    c, p, out = G.case_result(True, 6, True)
    st = out["steps"][5]
    t, s = c["target"].astype(np.float64)[out["pairs"][:, 0]], c["source"].astype(np.float64)[out["pairs"][:, 1]]
    H, mt, ms = R.cross_covariance(t, s, st["w"])
    n = len(t)
    assert np.abs(mt - st["mean_t"]).max() <= n * 2.0 ** -52 * np.abs(t).max() and np.abs(ms - st["mean_s"]).max() <= n * 2.0 ** -52 * np.abs(s).max()
    assert np.abs(H - st["H"]).max() <= 4 * n * 2.0 ** -52 * np.abs(H).max()


@pytest.mark.parametrize("small,dof,recip", ROWS)
def test_restatement_recovers_the_true_pose(small, dof, recip):
    """the reference's GNC on the inputs of the GPU tests; measured: dR 3e-7 .. 1e-5, dt 3e-5 .. 2e-4, 60 alignments on make_case, 57 on make_small_case"""
    c, p, out = G.case_result(small, dof, recip)
    share = float((c["pick"][out["pairs"][:, 1]] == out["pairs"][:, 0]).mean())
    dR, dt = G.pose_error(out["T"], c["T_true"])
    print(f"small={small} dof={dof} reciprocal={recip}: pairs {len(out['pairs'])} true share {share:.2f} alignments {out['num_alignments']} dR {dR:.1e} dt {dt:.1e}")
    assert not out["swapped"] and out["num_initial"] == len(c["source"])
    assert out["num_alignments"] == (57 if small else 60)
    assert share > 0.55 and dR < 2e-5 and dt < 3e-4
    if dof == 4:
        assert (out["T"][2, :3] == [0, 0, 1]).all() and (out["T"][:2, 2] == 0).all()


@pytest.mark.parametrize("small,dof", [(True, 6), (True, 4), (False, 6), (False, 4)])
def test_no_match_is_decided_by_a_tie_or_a_narrow_gap(small, dof):
    c, p, out = G.case_result(small, dof, True)
    corr = out["corr"]
    tf, sf = c["target_features"], c["source_features"]
    ok = corr["forward"] >= 0
    idx, gap = G.match_margins(tf, sf, corr["rows"][ok])
    assert (idx == corr["forward"][ok]).all() and gap.min() > 1e-9
    idx, gap = G.match_margins(sf, tf, corr["forward"][ok])
    assert (idx == corr["back"][ok]).all() and gap.min() > 1e-9
    if small:
        assert not ok[R.SMALL_ROW_NAN] and ok[list(R.SMALL_ZERO_ROWS)].all()  # GNC has no invalid-feature rule: zero rows match, the NaN row drops out
        # the clouds passed the other way round (as the GPU test does): the smaller cloud still queries, so the searches are the same two and the pairs the same, swapped
        sw = G.find_correspondences(sf, tf, p)
        assert sw["swapped"] and (sw["forward"] == corr["forward"]).all() and (sw["pairs"] == corr["pairs"][:, ::-1]).all()


@pytest.mark.parametrize("small,dof,tuples", [(True, 6, 50), (True, 4, 50), (False, 6, 300), (False, 4, 300)])
def test_no_tuple_ratio_lies_on_a_threshold(small, dof, tuples):
    c, p, out = G.case_result(small, dof, True)
    assert len(out["pairs"]) > 3 * tuples
    _, ratios = G.tuple_ratios(c["target"], c["source"], out["pairs"], tuples, p["seed"])
    r = ratios[np.isfinite(ratios)]
    assert (np.abs(r - 0.9) > 1e-9).all() and (np.abs(r - 1.0 / 0.9) > 1e-9).all()
    kept = G.tuple_test(c["target"], c["source"], out["pairs"], G.params(dof=dof, tuple_check=True, max_num_tuples=tuples))
    assert 3 <= len(kept) <= 3 * tuples and (np.diff(kept[:, 1]) > 0).all()


@pytest.mark.parametrize("small,dof,recip", ROWS)
def test_traced_steps_are_conditioned_and_no_error_lies_on_the_inlier_threshold(small, dof, recip):
    c, p, out = G.case_result(small, dof, recip)
    thresh = (2.0 * p["max_corr_dist"]) ** 2
    for st in out["steps"]:
        assert R.rotation_bound(st["H"], dof)[0]
        assert (np.abs(st["e"] - thresh) > 1e-9 * thresh).all()

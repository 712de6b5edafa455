"""tests/icp_ref.py held to the reference's own definitions (impl/integrated_icp_factor_impl.hpp), without a device: the derivatives against differences of the
error and of the residuals, the correspondence cut-off, and the three branches of the update tolerance.

Bounds of the differencing (h = 1e-5, central): truncation h^2 / 6 x (third / first derivative, of order one for a rotation) = 2e-11 relative; rounding
eps x |f| / (h |f'|) = 1e-11 x |f| / |f'|, with |error| / |b| and |r| / |J| of order one or below on a scan.  1e-7 on b and 1e-8 on H leave three orders."""
import numpy as np
import pytest

import icp_ref
import normals_ref
from helpers import expmap, rel_err

H_STEP = 1e-5
XI = np.array([0.01, -0.02, 0.015, 0.10, -0.05, 0.03])


@pytest.fixture(scope="module")
def small(kitti00):
    """a few hundred source points against the whole target, with the target's normals"""
    tp = kitti00["target_points"]
    normals = normals_ref.reference_normals(tp, kitti00["target_covs"]).astype(np.float32)
    return tp, kitti00["source_points"][::40].copy(), normals


def _perturbed(delta, xi_t, xi_s):
    """delta of the poses (T_t Expmap(xi_t), T_s Expmap(xi_s)) with T_t^-1 T_s = delta"""
    return np.linalg.inv(expmap(xi_t)) @ delta @ expmap(xi_s)


@pytest.mark.parametrize("plane", [False, True])
def test_derivatives_match_differences(small, plane):
    tp, sp, normals = small
    f = icp_ref.ICPFactorRef(tp, sp, normals, use_point_to_plane=plane)
    delta = expmap(XI)
    L = f.linearize(delta)
    assert 300 < L["num_inliers"] <= len(sp)
    zero = np.zeros(6)
    gt, gs = np.zeros(6), np.zeros(6)
    Jt, Js = np.zeros((L["num_inliers"], 3, 6)), np.zeros((L["num_inliers"], 3, 6))
    for k in range(6):
        e = np.zeros(6)
        e[k] = H_STEP
        # correspondences frozen: error() and residuals() never search once some are stored
        gt[k] = (f.error(_perturbed(delta, e, zero)) - f.error(_perturbed(delta, -e, zero))) / (2 * H_STEP)
        gs[k] = (f.error(_perturbed(delta, zero, e)) - f.error(_perturbed(delta, zero, -e))) / (2 * H_STEP)
        Jt[:, :, k] = (f.residuals(_perturbed(delta, e, zero)) - f.residuals(_perturbed(delta, -e, zero))) / (2 * H_STEP)
        Js[:, :, k] = (f.residuals(_perturbed(delta, zero, e)) - f.residuals(_perturbed(delta, zero, -e))) / (2 * H_STEP)
    assert f.searches == 1
    # r(xi) = mu - T(xi) p has the Jacobians J_t = [-[q]x, I] and J_s = [R [p]x, -R] (:220-226), so the gradient of sum r^T r is 2 sum J^T r = 2 b
    assert rel_err(gt, 2 * L["b_target"]) < 1e-7
    assert rel_err(gs, 2 * L["b_source"]) < 1e-7
    assert rel_err(np.einsum("nki,nkj->ij", Jt, Jt), L["H_target"]) < 1e-8
    assert rel_err(np.einsum("nki,nkj->ij", Js, Js), L["H_source"]) < 1e-8
    assert rel_err(np.einsum("nki,nkj->ij", Jt, Js), L["H_target_source"]) < 1e-8
    assert abs((f.residuals(delta) ** 2).sum() - L["error"]) <= 1e-12 * L["error"]  # error = sum r^T r, no 1/2


def test_cut_off_is_strict_and_point_to_plane_is_element_wise():
    tp = np.array([[0.0, 0.0, 0.0], [10.0, 0.0, 0.0]], np.float32)
    sp = np.array([[0.5, 0.0, 0.0], [1.0, 0.0, 0.0], [9.75, 0.25, 0.0], [5.0, 0.0, 0.0]], np.float32)
    n = np.array([[0.6, 0.0, 0.8], [0.0, 1.0, 0.0]], np.float32)
    f = icp_ref.ICPFactorRef(tp, sp, n, use_point_to_plane=False)
    L = f.linearize(np.eye(4))
    assert f.correspondences.tolist() == [0, -1, 1, -1]  # sq_dist 1.0 is not < 1.0
    assert L["num_inliers"] == 2 and L["error"] == 0.25 + 0.125
    g = icp_ref.ICPFactorRef(tp, sp, n, use_point_to_plane=True)
    Lp = g.linearize(np.eye(4))
    n64 = n.astype(np.float64)
    # r = n o d, not n . d: point 0 has d = (-0.5, 0, 0), r = (-0.3, 0, 0); point 2 has d = (0.25, -0.25, 0), r = (0, -0.25, 0)
    assert abs(Lp["error"] - ((n64[0, 0] * 0.5) ** 2 + 0.0625)) < 1e-15
    tie, cut = f.margins(np.eye(4))
    assert cut[1] == 0.0 and tie[3] == 0.0 and tie[0] > 0.9  # the point on the cut-off and the point half way between the two targets are flagged
    with pytest.raises(ValueError, match="target frame doesn't have required attributes for icp"):
        icp_ref.ICPFactorRef(tp, sp, None, use_point_to_plane=True)
    one = icp_ref.ICPFactorRef(tp[:1], sp)
    assert np.isinf(one.margins(np.eye(4))[0]).all()  # a target of one point has no second neighbour


def test_update_tolerance_walks_its_three_branches(small):
    tp, sp, _ = small
    f = icp_ref.ICPFactorRef(tp, sp)
    d1 = expmap(XI)
    d2 = d1 @ expmap([0.01, 0.0, -0.01, 0.05, 0.0, 0.02])   # 0.014 rad, 0.054 m from d1
    d3 = d1 @ expmap([0.06, 0.0, 0.0, 0.0, 0.0, 0.0])        # 0.06 rad from d1
    rot, trans = icp_ref.pose_difference(d2, d1)
    assert abs(rot - np.hypot(0.01, 0.01)) < 1e-12 and 0.05 < trans < 0.06
    # (1) zero tolerances (the default): every linearise searches and moves the correspondence point
    f.linearize(d1)
    f.linearize(d2)
    assert f.searches == 2 and np.array_equal(f.last_correspondence_point, d2)
    # (2) both tolerances set: nothing stored -> searches; inside both -> kept; outside one -> searched
    g = icp_ref.ICPFactorRef(tp, sp)
    g.set_correspondence_update_tolerance(0.05, 0.5)
    g.linearize(d1)                       # nothing stored: searches whatever the tolerances
    c1 = g.correspondences.copy()
    L2 = g.linearize(d2)                  # inside: kept
    assert g.searches == 1 and np.array_equal(g.correspondences, c1) and np.array_equal(g.last_correspondence_point, d1)
    fresh = icp_ref.ICPFactorRef(tp, sp).linearize(d2)
    assert L2["num_inliers"] == (c1 >= 0).sum() and (L2["error"] != fresh["error"])
    g.linearize(d3)                       # 0.06 rad >= 0.05: searched, and the correspondence point moves
    assert g.searches == 2 and np.array_equal(g.last_correspondence_point, d3)
    # (3) only one tolerance set: the other's strict '<' against zero always fails -> searches
    for tol in [(0.05, 0.0), (0.0, 0.5)]:
        k = icp_ref.ICPFactorRef(tp, sp)
        k.set_correspondence_update_tolerance(*tol)
        k.linearize(d1)
        k.linearize(d2)
        k.linearize(d2)
        assert k.searches == 3, tol

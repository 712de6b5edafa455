"""CPU checks of tests/loam_ref.py, the numpy restatement the LOAM GPU tests compare against: its Jacobians against central differences of its residual rows, the
residuals against their geometric meaning and against the M-forms the kernels sum."""
import numpy as np
import pytest

import icp_ref
import loam_ref
from helpers import expmap

XI = np.array([0.01, -0.02, 0.015, 0.10, -0.05, 0.03])


@pytest.fixture(scope="module")
def parts(kitti00):
    tp, sp = kitti00["target_points"], kitti00["source_points"][:1500]
    e, p = loam_ref.EdgeFactorRef(tp[0::2], sp), loam_ref.PlaneFactorRef(tp[1::2], sp)
    for f in (e, p):
        f.update_correspondences(expmap(XI))
        assert (f.correspondences[:, 0] >= 0).sum() > 500  # (enough rows for the checks below to mean something)
    return e, p


def test_jacobians_match_central_differences(parts):
    """step 1e-6, agreement to 1e-6 relative: the truncation bound of the central difference of these smooth rows, not a kernel tolerance"""
    delta, h = expmap(XI), 1e-6
    for f in parts:
        Jt, Js = f.jacobians(delta)
        for k in range(6):
            xi = np.zeros(6)
            xi[k] = h
            # source side: delta -> delta Exp(xi); target side: T_t -> T_t Exp(xi), i.e. delta -> Exp(-xi) delta
            ds = (f.residuals(delta @ expmap(xi)) - f.residuals(delta @ expmap(-xi))) / (2 * h)
            dt = (f.residuals(expmap(-xi) @ delta) - f.residuals(expmap(xi) @ delta)) / (2 * h)
            for num, J, side in [(ds, Js[:, :, k], "source"), (dt, Jt[:, :, k], "target")]:
                # (r = A (x_j - q) and dq = -J_s xi on the source side, -J_t xi on the target side: the rows' derivatives are the Jacobians themselves)
                assert np.linalg.norm(num - J) <= 1e-6 * np.linalg.norm(J), (f.K, side, k)


def test_edge_residual_is_the_distance_to_the_line(parts):
    e, _ = parts
    delta = expmap(XI)
    sel, p, q, r, _ = e._rows(delta)
    c = e.correspondences[sel]
    xj, xl = e.target[c[:, 0]], e.target[c[:, 1]]
    u = (xl - xj) / np.linalg.norm(xl - xj, axis=1)[:, None]
    w = q - xj
    dist = np.linalg.norm(w - (w * u).sum(1)[:, None] * u, axis=1)
    assert np.allclose(np.linalg.norm(r, axis=1), dist, rtol=1e-9, atol=1e-12)


def test_edge_cross_product_form_equals_the_m_form(parts):
    e, _ = parts
    delta = expmap(XI)
    sel, p, q, r, A = e._rows(delta)
    xj = e.target[e.correspondences[sel][:, 0]]
    m_form = np.einsum("nij,nj->ni", A, xj - q)  # c [v]x (x_j - q)
    assert np.abs(r - m_form).max() <= 1e-12 * max(1.0, np.abs(r).max())
    M = np.einsum("nki,nkj->nij", A, A)
    assert np.allclose(np.einsum("ni,nij,nj->n", xj - q, M, xj - q), (r * r).sum(1), rtol=1e-10, atol=1e-14)


def test_plane_residual_is_the_icp_reference_given_the_same_normal(parts, kitti00):
    _, p = parts
    delta = expmap(XI)
    sel, src, q, r, A = p._rows(delta)
    c = p.correspondences[sel]
    n = np.cross(p.target[c[:, 0]] - p.target[c[:, 1]], p.target[c[:, 0]] - p.target[c[:, 2]])
    n /= np.linalg.norm(n, axis=1)[:, None]
    normals = np.zeros_like(p.target)
    normals[c[:, 0]] = n  # (anchors repeat; the comparison below is per anchor with the last normal written)
    keep = np.all(normals[c[:, 0]] == n, axis=1)
    icp = icp_ref.ICPFactorRef(p.target, p.source, normals, use_point_to_plane=True)
    icp.normals = normals  # exact f64 normals
    icp.correspondences = np.where(p.correspondences[:, 0] >= 0, p.correspondences[:, 0], -1)
    assert keep.sum() > 500 and np.array_equal(icp.residuals(delta)[keep], r[keep])


def test_combined_is_edge_plus_plane(kitti00):
    tp, sp = kitti00["target_points"], kitti00["source_points"][:1500]
    delta = expmap(XI)
    f = loam_ref.LOAMFactorRef(tp[0::2], tp[1::2], sp, sp)
    L = f.linearize(delta)
    e, p = loam_ref.EdgeFactorRef(tp[0::2], sp).linearize(delta), loam_ref.PlaneFactorRef(tp[1::2], sp).linearize(delta)
    for k in loam_ref.BLOCKS + ["error", "num_inliers"]:
        assert np.array_equal(L[k], e[k] + p[k]), k
    # validation rejects some edge pairs, is idempotent, and leaves the plane part to the second bound as written (always true: it rejects with the first alone)
    f.set_enable_correspondence_validation(True)
    f.update_correspondences(delta)
    first = f.rejected
    assert first[0] > 0 and f.edge.validate() == 0 and f.plane.validate() == 0
    assert loam_ref.THETA_PLANE_2 > np.pi

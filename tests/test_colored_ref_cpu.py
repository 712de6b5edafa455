"""CPU checks of the colored GICP restatement (tests/colored_ref.py) the GPU tests compare against, of the constants those tests are held to, and of what the
library decides on the host: the exports and the argument refusals made before any device work."""
import ctypes as C

import numpy as np

import colored_ref
import icp_ref
from helpers import BLOCKS, expmap, rel_err

from gtsam_points_amd.features import IntegratedColoredGICPFactorGPU, estimate_intensity_gradients_gpu  # noqa: F401  (what the restatement stands beside: no device code, no tests of it)

XI = np.array([0.01, -0.02, 0.015, 0.10, -0.05, 0.03])


def _brute_neighbours(p, k):
    d = ((p[:, None, :] - p[None, :, :]) ** 2).sum(axis=2)
    return np.argsort(d, axis=1, kind="stable")[:, :k]


def test_gradient_of_a_linear_field_on_a_tilted_plane():
    """I = a . p + c on a plane with unit normal n: every neighbour row reads (p_j - p) . g = a . (p_j - p) and the normal row n . g = 0, so g = P a"""
    rng = np.random.default_rng(2)
    n = np.array([0.3, -0.2, 0.9])
    n /= np.linalg.norm(n)
    t1 = np.cross(n, [1.0, 0.0, 0.0])
    t1 /= np.linalg.norm(t1)
    t2 = np.cross(n, t1)
    st = rng.uniform(-1.0, 1.0, (200, 2))
    p = np.array([0.5, -1.0, 2.0]) + st[:, :1] * t1 + st[:, 1:] * t2
    a = np.array([0.7, -0.4, 0.25])
    I = p @ a + 0.3
    want = a - (a @ n) * n
    for k, k_photo in [(10, None), (10, 4), (32, None)]:
        g, cond = colored_ref.intensity_gradients(p, np.tile(n, (len(p), 1)), I, _brute_neighbours(p, k), k_photo, as_given=True)
        assert np.isfinite(cond).all() and cond.max() < 1e6
        assert np.abs(g - want).max() <= 1e-10, (k, k_photo, np.abs(g - want).max())
    nb = _brute_neighbours(p, 10)
    assert colored_ref.grad_H_cond(p, np.tile(n, (len(p), 1)), I, nb, 7) == np.linalg.cond(colored_ref.gradient_systems(p, np.tile(n, (len(p), 1)), I, nb)[1][7])


def test_short_neighbour_lists_give_zero_gradients():
    p, I = colored_ref.two_plane_cloud(50)
    nb, normals = colored_ref.host_neighbours_and_normals(p, 10)
    nb = nb.copy()
    nb[3, 9] = -1
    nb[5, 2] = -1
    g, cond = colored_ref.intensity_gradients(p, normals, I, nb)
    assert not g[3].any() and not g[5].any() and np.isinf(cond[[3, 5]]).all() and g[4].any()
    g6, _ = colored_ref.intensity_gradients(p, normals, I, nb, 6)  # slot 9 is not among the first 6
    assert g6[3].any() and not g6[5].any()


def test_gradient_constants_on_the_test_cloud():
    """GRADIENT_C is 4x (at most 6x) the reference's own reorder difference on the GPU tests' cloud, and no point of that cloud comes near the cond(H) cap"""
    p, I = colored_ref.two_plane_cloud()
    worst = 0.0
    for k in (10, 32):
        nb, normals = colored_ref.host_neighbours_and_normals(p, k)
        assert (nb[:, 0] == np.arange(len(p))).all()
        for k_photo in (k, 6):
            _, cond = colored_ref.intensity_gradients(p, normals, I, nb, k_photo)
            assert (cond > colored_ref.COND_CAP).sum() <= 0.01 * len(p)
            ratio = colored_ref.reorder_ratio(p, normals, I, nb, k_photo).max()
            print(f"[colored] k = {k}, k_photo = {k_photo}: reorder ratio {ratio:.3f}, cond(H) up to {cond.max():.3g}")
            worst = max(worst, ratio)
    assert 4.0 * worst <= colored_ref.GRADIENT_C <= 6.0 * worst, worst


def _random_factor(seed, weight, n_target=300, n_source=120):
    rng = np.random.default_rng(seed)
    tp = rng.uniform(-2.0, 2.0, (n_target, 3)).astype(np.float32)
    T = expmap(XI)
    sp = ((tp[:n_source].astype(np.float64) + rng.normal(0.0, 0.02, (n_source, 3)) - T[:3, 3]) @ T[:3, :3]).astype(np.float32)

    def spd(count):
        A = rng.normal(size=(count, 3, 3))
        return (A @ A.transpose(0, 2, 1) * 0.01 + 1e-3 * np.eye(3)).astype(np.float32)

    normals = rng.normal(size=(n_target, 3))
    normals = (normals / np.linalg.norm(normals, axis=1, keepdims=True)).astype(np.float32)
    return colored_ref.ColoredGICPFactorRef(tp, spd(n_target), normals, rng.uniform(0, 1, n_target), rng.normal(size=(n_target, 3)), sp, spd(n_source), rng.uniform(0, 1, n_source),
                                            max_correspondence_distance=0.5, photometric_term_weight=weight)


def _general(delta):
    out = delta.copy()
    out[:3, :3] = out[:3, :3] @ (np.eye(3) + 1e-3 * np.random.default_rng(11).normal(size=(3, 3)))
    return out


def test_record_matches_finite_differences_and_gauss_newton_products():
    """with rho(delta) the stacked residuals on the stored correspondences and M_g (error = |rho|^2): for a source perturbation delta Expmap(xi) and a target
    perturbation Expmap(-xi) delta, b = J_rho^T rho = grad(error) / 2 and H = J_rho^T J_rho, J_rho by central differences -- at a rigid pose and at one whose 3x3
    block is not orthonormal (the Jacobians use the block as given, so the identities hold there too)"""
    h = 1e-6
    for weight in (0.25, 0.0, 1.0):
        for delta in (expmap(XI), _general(expmap(XI))):
            ref = _random_factor(4, weight)
            L = ref.linearize(delta)
            assert L["num_inliers"] > 60
            source = lambda xi: delta @ expmap(xi)  # noqa: E731
            target = lambda xi: expmap(-np.asarray(xi)) @ delta  # noqa: E731
            J, grad = {}, {}
            for name, move in (("source", source), ("target", target)):
                cols = [(ref.residuals(move(h * e)) - ref.residuals(move(-h * e))) / (2 * h) for e in np.eye(6)]
                J[name] = np.stack(cols, axis=2)  # (N, 4, 6)
                grad[name] = np.array([(ref.error(move(h * e)) - ref.error(move(-h * e))) / (2 * h) for e in np.eye(6)])
            rho = ref.residuals(delta)
            assert abs((rho * rho).sum() - L["error"]) <= 1e-12 * L["error"]
            for name in ("source", "target"):
                assert rel_err(np.einsum("nki,nk->i", J[name], rho), L["b_" + name]) < 1e-6, (weight, name)
                assert rel_err(0.5 * grad[name], L["b_" + name]) < 1e-6, (weight, name)
                assert rel_err(np.einsum("nki,nkj->ij", J[name], J[name]), L["H_" + name]) < 1e-6, (weight, name)
            assert rel_err(np.einsum("nki,nkj->ij", J["target"], J["source"]), L["H_target_source"]) < 1e-6, weight
            assert ref.searches == 1  # error() and residuals() never search


def test_weight_zero_with_unit_mahalanobis_is_point_to_point_icp():
    rng = np.random.default_rng(8)
    tp = rng.uniform(-2.0, 2.0, (300, 3)).astype(np.float32)
    sp = (tp[:150] + rng.normal(0.0, 0.05, (150, 3))).astype(np.float32)
    eye, zero = np.tile(np.eye(3), (300, 1, 1)), np.zeros((150, 3, 3))
    delta = _general(expmap(0.2 * XI))
    col = colored_ref.ColoredGICPFactorRef(tp, eye, rng.normal(size=(300, 3)), rng.uniform(0, 1, 300), rng.normal(size=(300, 3)), sp, zero, rng.uniform(0, 1, 150), 0.5, 0.0)
    icp = icp_ref.ICPFactorRef(tp, sp, max_correspondence_distance=0.5)
    A, B = col.linearize(delta), icp.linearize(delta)
    assert A["num_inliers"] == B["num_inliers"] > 100 and abs(A["error"] - B["error"]) <= 1e-13 * B["error"]
    for k in BLOCKS:
        assert rel_err(A[k], B[k]) <= 1e-13, k
    near = delta @ expmap(0.1 * XI)
    assert abs(col.error(near) - icp.error(near)) <= 1e-13 * icp.error(near)
    assert np.array_equal(col.margins(delta)[0], icp.margins(delta)[0])


def test_update_tolerance_keeps_correspondences_but_not_the_mahalanobis():
    ref = _random_factor(4, 0.25)
    ref.set_correspondence_update_tolerance(0.05, 0.5)
    d1 = expmap(XI)
    d2 = d1 @ expmap([0.01, 0.0, -0.01, 0.05, 0.0, 0.02])
    ref.linearize(d1)
    c1, m1 = ref.correspondences.copy(), ref.mahalanobis.copy()
    ref.linearize(d2)
    assert ref.searches == 1 and np.array_equal(ref.correspondences, c1) and not np.array_equal(ref.mahalanobis, m1)  # :131-139 run at every call
    ref.linearize(d1 @ expmap([0.06, 0.0, 0.0, 0.0, 0.0, 0.0]))
    assert ref.searches == 2


NEW_SYMBOLS = [
    "gp_estimate_intensity_gradients", "gp_estimate_intensity_gradients_from_neighbors", "gp_colored_gicp_factor_create", "gp_colored_gicp_factor_destroy",
    "gp_colored_gicp_factor_linearize", "gp_colored_gicp_factor_compute_error", "gp_colored_gicp_factor_set_photometric_term_weight",
    "gp_colored_gicp_factor_set_max_correspondence_distance", "gp_colored_gicp_factor_set_correspondence_update_tolerance", "gp_colored_gicp_factor_num_correspondences",
]


def test_new_names_are_exported():
    import gtsam_points_amd as gpa
    from gtsam_points_amd import _capi

    lib = _capi.load()
    for s in NEW_SYMBOLS:
        assert s in _capi.EXPORTED_SYMBOLS and hasattr(lib, s), s
    for name in ("IntegratedColoredGICPFactorGPU", "IntensityGradientsGPU", "estimate_intensity_gradients_gpu"):
        assert name in gpa.__all__ and hasattr(gpa, name), name


def test_entry_points_refuse_bad_arguments_without_a_device():
    from gtsam_points_amd import _capi

    lib = _capi.load()
    INVALID = 1  # GP_ERROR_INVALID_ARGUMENT
    fake = C.c_void_p(64)  # never dereferenced: every call below is refused first
    # the gradients on a given table: (points, normals, intensities, n, neighbors, k, k_photo, gradients, stream)
    good = [fake, fake, fake, 1, fake, 10, 10, fake, None]
    for at in (0, 1, 2, 4, 7):
        args = list(good)
        args[at] = None
        assert lib.gp_estimate_intensity_gradients_from_neighbors(*args) == INVALID, at
    assert b"gp_estimate_intensity_gradients_from_neighbors" in lib.gp_last_error()
    for k, k_photo in [(10, 11), (10, 0), (0, 0), (33, 34)]:
        assert lib.gp_estimate_intensity_gradients_from_neighbors(fake, fake, fake, 1, fake, k, k_photo, fake, None) == INVALID, (k, k_photo)
    assert lib.gp_estimate_intensity_gradients_from_neighbors(fake, fake, fake, -1, fake, 10, 10, fake, None) == INVALID
    # ... with the search: (points, normals, intensities, n, k, cell_size, gradients, num_short, stream)
    good = [fake, fake, fake, 1, 10, 0.0, fake, None, None]
    for at in (0, 1, 2, 6):
        args = list(good)
        args[at] = None
        assert lib.gp_estimate_intensity_gradients(*args) == INVALID, at
    for k in (33, 0, -1):
        assert lib.gp_estimate_intensity_gradients(fake, fake, fake, 1, k, 0.0, fake, None, None) == INVALID, k
    assert b"gp_estimate_intensity_gradients" in lib.gp_last_error()
    # the factor: (grid, 5 target arrays, num_target, 3 source arrays, num_points, max_sq, weight, stream, out)
    h = C.c_void_p()
    good = [fake, fake, fake, fake, fake, fake, 1, fake, fake, fake, 1, 1.0, 0.25, None, C.byref(h)]
    for at in (0, 1, 2, 3, 4, 5, 7, 8, 9, 14):
        args = list(good)
        args[at] = None
        assert lib.gp_colored_gicp_factor_create(*args) == INVALID and not h.value, at
    for weight in (-0.1, 1.1, float("nan")):
        args = list(good)
        args[12] = weight
        assert lib.gp_colored_gicp_factor_create(*args) == INVALID and not h.value, weight
        assert b"photometric_term_weight" in lib.gp_last_error()
    args = list(good)
    args[11] = 0.0
    assert lib.gp_colored_gicp_factor_create(*args) == INVALID and not h.value
    # NULL handles
    assert lib.gp_colored_gicp_factor_destroy(None) == 0 and lib.gp_colored_gicp_factor_num_correspondences(None) == 0
    assert lib.gp_colored_gicp_factor_linearize(None, None, None) == INVALID and lib.gp_colored_gicp_factor_compute_error(None, None, None, None) == INVALID
    assert lib.gp_colored_gicp_factor_set_photometric_term_weight(None, 0.5) == INVALID
    assert lib.gp_colored_gicp_factor_set_max_correspondence_distance(None, 1.0) == INVALID
    assert lib.gp_colored_gicp_factor_set_correspondence_update_tolerance(None, 0.1, 0.1) == INVALID

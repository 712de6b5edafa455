"""IntensityGradients::estimate (factors/intensity_gradients.cpp) and IntegratedColoredGICPFactor_ (factors/impl/integrated_colored_gicp_factor_impl.hpp) restated in
numpy, f64 on the f32 inputs.  A helper, not a test.

  intensity_gradients(points, normals, intensities, neighbors, k_photo)   :40-66   per point: row 0 of A is the normal (b = 0), row j = 1 .. k_photo - 1 is the
                                            neighbour projected onto the tangent plane minus the point, b_j = I_j - I; H = A^T A, e = A^T b, g = H^-1 e with the
                                            closed-form cofactor inverse (Eigen's 3x3 inverse).  The rows are summed one after the other in slot order
                                            (reverse=True: from the last slot down -- what two correct f64 implementations may differ by).  A point with a -1
                                            among its first k_photo slots gets (0, 0, 0).  Returns (g (N,3), cond(H) (N,); inf where there is no H)
                                            dtype: the float type every operation and every sum runs in (f64; np.longdouble for precision checks)
  gradient_systems(...)                     the same up to the solve: (rows with a full list, H, e, rho = the largest |a_j| of each row)
  grad_H_cond(..., i)                       cond(H) of one point
  ColoredGICPFactorRef
    update_correspondences(delta) :101-140  the tolerance rule, a brute-force 1-NN of T p among the target points (icp_ref.nearest_two: sq_dist < max), and
                                            M_g = (C_B + R C_A R^T)^-1 at delta for every matched point -- recomputed at every call, searched or kept (:131-139)
    evaluate(delta)               :162-253  q = T p_A, d = mu_B - q, P = I - n_B n_B^T, u = P g_B, r_p = I_B - I_A - u . d, w_p the photometric weight,
                                            w_g = 1 - w_p: error = sum w_g d^T M_g d + w_p r_p^2, H = sum J^T (w_g M_g + w_p u u^T) J,
                                            b = sum J^T (w_g M_g d - w_p r_p u), J_t = [-[q]x, I], J_s = [R [p]x, -R], R = delta's 3x3 block AS GIVEN
                                            (the reference has q - mu_B and -J_t: the products are the same)
    residuals(delta)                        (N_matched, 4) rows [sqrt(w_g) L^T d, sqrt(w_p) r_p] with M_g = L L^T on the stored correspondences and M_g: their
                                            squares sum to error(delta), for differencing
    margins(delta)                          as icp_ref's

  two_plane_cloud(n, seed)                  the test cloud: jittered points on two intersecting planes with a smooth non-linear intensity field
  moved_copy(points, intensities, T, ...)   a source for it: a jittered subset, every 20th point pushed off the surface, in the frame T maps onto the cloud's
"""
import numpy as np

from icp_ref import hat, nearest_two, pose_difference, transform


def _f32_as_f64(a, shape):
    return np.asarray(a, dtype=np.float32).reshape(shape).astype(np.float64)


def inverse_sym3(H):
    """the cofactor inverse of symmetric 3x3 matrices (N,3,3), from the upper triangle, in H's own float type"""
    c00, c01, c02, c11, c12, c22 = H[:, 0, 0], H[:, 0, 1], H[:, 0, 2], H[:, 1, 1], H[:, 1, 2], H[:, 2, 2]
    i00 = c11 * c22 - c12 * c12
    i01 = c02 * c12 - c01 * c22
    i02 = c01 * c12 - c02 * c11
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = H.dtype.type(1.0) / (c00 * i00 + c01 * i01 + c02 * i02)
        m = np.stack([i00 * inv, i01 * inv, i02 * inv, (c00 * c22 - c02 * c02) * inv, (c01 * c02 - c00 * c12) * inv, (c00 * c11 - c01 * c01) * inv], axis=1)
    return m[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)


def gradient_systems(points, normals, intensities, neighbors, k_photo=None, reverse=False, as_given=False, dtype=np.float64):
    """(rows with a full neighbour list, H (M,3,3), e (M,3), rho (M,) f64: the largest |a_j|_2 among a row's neighbour rows) of those rows.  as_given: the inputs
    are f64 and are not rounded to f32 first (exact test inputs).  dtype: the float type every operation and every sum runs in (np.longdouble for the precision
    check of tests/test_colored_domain_ref_cpu.py)"""
    read = (lambda a, shape: np.asarray(a, dtype=np.float64).reshape(shape)) if as_given else _f32_as_f64
    p, n, I = (read(a, shape).astype(dtype) for a, shape in ((points, (-1, 3)), (normals, (-1, 3)), (intensities, (-1,))))
    nb = np.asarray(neighbors, dtype=np.int64).reshape(len(p), -1)
    k_photo = nb.shape[1] if k_photo is None else int(k_photo)
    assert 1 <= k_photo <= nb.shape[1]  # :32-35
    rows = np.flatnonzero((nb[:, :k_photo] >= 0).all(axis=1))
    p0, n0, I0 = p[rows], n[rows], I[rows]
    H = n0[:, :, None] * n0[:, None, :]  # :50-51
    e = np.zeros((len(rows), 3), dtype=dtype)
    rho = np.zeros(len(rows))
    slots = range(1, k_photo)
    for j in reversed(slots) if reverse else slots:  # :54-61
        t = nb[rows, j]
        along = ((p[t] - p0) * n0).sum(axis=1)
        a = (p[t] - along[:, None] * n0) - p0
        H = H + a[:, :, None] * a[:, None, :]
        e = e + a * (I[t] - I0)[:, None]
        rho = np.maximum(rho, np.sqrt((a * a).sum(axis=1)).astype(np.float64))
    return rows, H, e, rho


def intensity_gradients(points, normals, intensities, neighbors, k_photo=None, reverse=False, as_given=False, dtype=np.float64):
    """(g (N,3) in `dtype`, cond(H) (N,) f64 of the f64 rounding of H; inf where there is no H)"""
    rows, H, e, _ = gradient_systems(points, normals, intensities, neighbors, k_photo, reverse, as_given, dtype)
    count = len(np.asarray(points).reshape(-1, 3))
    g, cond = np.zeros((count, 3), dtype=dtype), np.full(count, np.inf)
    if len(rows):
        with np.errstate(all="ignore"):
            g[rows] = np.einsum("nij,nj->ni", inverse_sym3(H), e)  # :63-65
            cond[rows] = _cond(H.astype(np.float64))
    return g, cond


def _cond(H):
    """2-norm condition numbers of (M,3,3) matrices; inf for those with a non-finite entry (numpy.linalg refuses them)"""
    out = np.full(len(H), np.inf)
    ok = np.isfinite(H).all(axis=(1, 2))
    if ok.any():
        out[ok] = np.linalg.cond(H[ok])
    return out


def grad_H_cond(points, normals, intensities, neighbors, i, k_photo=None):
    rows, H, _, _ = gradient_systems(points, normals, intensities, neighbors, k_photo)
    at = np.flatnonzero(rows == i)
    return float(np.linalg.cond(H[at[0]])) if len(at) else float("inf")


# How far two correct f64 implementations of the gradient may differ: C cond(H) 2^-52 |g|.  C is 4x what intensity_gradients differs from itself when the
# neighbours are summed in reversed order, measured on two_plane_cloud() with host k-NN tables and host normals at k = 10 and k = 32 (the largest ratio
# |g - g_reversed|_inf / (cond(H) 2^-52 |g|_inf) over all points was 3.88, at k = 32 where cond(H) is about 2 and the
# length of the sums counts; tests/test_colored_ref_cpu.py measures it again and holds C to 4x .. 6x of it).
GRADIENT_C = 16.0
COND_CAP = 1e8  # points with cond(H) beyond it are not compared (at most 1 % of a cloud)


def gradient_bound(g_ref, cond):
    """per point: 2^-23 |g_ref|_inf (the store's rounding to f32, with a factor 2 to spare) + GRADIENT_C cond(H) 2^-52 |g_ref|_inf"""
    a = np.abs(g_ref).max(axis=1)
    return 2.0**-23 * a + GRADIENT_C * cond * 2.0**-52 * a


def reorder_ratio(points, normals, intensities, neighbors, k_photo=None):
    """per point with cond(H) <= COND_CAP: |g - g_reversed|_inf / (cond(H) 2^-52 |g|_inf)"""
    g, cond = intensity_gradients(points, normals, intensities, neighbors, k_photo)
    gr, _ = intensity_gradients(points, normals, intensities, neighbors, k_photo, reverse=True)
    keep = cond <= COND_CAP
    return np.abs(g - gr).max(axis=1)[keep] / (cond[keep] * 2.0**-52 * np.maximum(np.abs(g).max(axis=1)[keep], 1e-300))


def host_neighbours_and_normals(points, k):
    """(neighbour table (N,k) int with the point itself in slot 0, unit normals (N,3) f32 by eigh of the neighbourhood's covariance): what the CPU tests feed the
    restatement with where the GPU tests use the device's search and estimator"""
    import knn_ref

    _, idx = knn_ref.neighbours(points, points, k - 1)
    _, _, V = knn_ref.reference_covariance(knn_ref._f64(points)[idx])
    return idx, np.ascontiguousarray(V[:, :, 0], dtype=np.float32)


def two_plane_cloud(n=4000, seed=3):
    """(points (n,3) f32, intensities (n,) f32): a floor tilted about y and a wall leaning onto it, meeting in a line, each point jittered by 5 mm across and along
    its plane; I = 0.5 + 0.3 sin(1.3 x + 0.4 z) cos(0.9 y) + 0.05 z^2"""
    rng = np.random.default_rng(seed)
    a = n // 2
    uv = rng.uniform(0.0, 4.0, (n, 2))
    p = np.empty((n, 3))
    p[:a] = np.stack([uv[:a, 0], uv[:a, 1], 0.1 * uv[:a, 0]], axis=1)                 # z = 0.1 x
    p[a:] = np.stack([4.0 - 0.2 * uv[a:, 0], uv[a:, 1], 0.4 + uv[a:, 0]], axis=1)      # x = 4 - 0.2 (z - 0.4), from the floor's edge at x = 4 upwards
    p += rng.normal(0.0, 0.005, (n, 3))
    I = 0.5 + 0.3 * np.sin(1.3 * p[:, 0] + 0.4 * p[:, 2]) * np.cos(0.9 * p[:, 1]) + 0.05 * p[:, 2] ** 2
    return np.ascontiguousarray(p, dtype=np.float32), np.ascontiguousarray(I, dtype=np.float32)


def moved_copy(points, intensities, T, count=2500, seed=21):
    """(points (count,3) f32, intensities (count,) f32): `count` of the points with 1 cm of jitter (intensities: 0.01), every 20th pushed 0.15 .. 0.8 m off in a
    random direction (so that a 0.3 m cut-off drops points a 1 m cut-off keeps), transformed by T^-1"""
    rng = np.random.default_rng(seed)
    pick = rng.choice(len(points), count, replace=False)
    moved = points[pick].astype(np.float64) + rng.normal(0.0, 0.01, (count, 3))
    off = rng.normal(size=(len(moved[::20]), 3))
    moved[::20] += off / np.linalg.norm(off, axis=1, keepdims=True) * rng.uniform(0.15, 0.8, (len(off), 1))
    T = np.asarray(T, dtype=np.float64)
    sp = np.ascontiguousarray((moved - T[:3, 3]) @ T[:3, :3], dtype=np.float32)
    return sp, np.ascontiguousarray(intensities[pick] + rng.normal(0.0, 0.01, count), dtype=np.float32)


class ColoredGICPFactorRef:
    def __init__(self, target_points, target_covs, target_normals, target_intensities, target_gradients, source_points, source_covs, source_intensities,
                 max_correspondence_distance=1.0, photometric_term_weight=0.25):
        """covariances as (N,3,3) matrices; like the device, the restatement reads their symmetric part"""
        sym = lambda c: 0.5 * (c + c.transpose(0, 2, 1))  # noqa: E731
        self.target = _f32_as_f64(target_points, (-1, 3))
        self.target_covs = sym(_f32_as_f64(target_covs, (-1, 3, 3)))
        self.normals = _f32_as_f64(target_normals, (-1, 3))
        self.target_intensities = _f32_as_f64(target_intensities, (-1,))
        self.gradients = _f32_as_f64(target_gradients, (-1, 3))
        self.source = _f32_as_f64(source_points, (-1, 3))
        self.source_covs = sym(_f32_as_f64(source_covs, (-1, 3, 3)))
        self.source_intensities = _f32_as_f64(source_intensities, (-1,))
        self.max_sq = float(max_correspondence_distance) ** 2  # :28
        self.photometric_term_weight = float(photometric_term_weight)  # :29
        self.tol_rot = self.tol_trans = 0.0  # :30-31
        self.correspondences = None
        self.mahalanobis = None
        self.last_correspondence_point = None
        self.searches = 0

    def set_correspondence_update_tolerance(self, angle, trans):
        self.tol_rot, self.tol_trans = float(angle), float(trans)

    def update_correspondences(self, delta):
        delta = np.asarray(delta, dtype=np.float64)
        keep = self.correspondences is not None and (self.tol_trans > 0.0 or self.tol_rot > 0.0)  # :103
        if keep:
            diff_rot, diff_trans = pose_difference(delta, self.last_correspondence_point)
            keep = diff_rot < self.tol_rot and diff_trans < self.tol_trans
        if not keep:
            self.last_correspondence_point = np.array(delta)
            idx, d1, _ = nearest_two(self.target, transform(delta, self.source))
            self.correspondences = np.where(d1 < self.max_sq, idx, -1)  # :127-128
            self.searches += 1
        sel = np.flatnonzero(self.correspondences >= 0)
        R = delta[:3, :3]
        self.mahalanobis = np.linalg.inv(self.target_covs[self.correspondences[sel]] + R[None] @ self.source_covs[sel] @ R.T[None])  # :134-138, matched points only

    def margins(self, delta):
        _, d1, d2 = nearest_two(self.target, transform(delta, self.source))
        with np.errstate(invalid="ignore", divide="ignore"):
            tie = np.where(np.isfinite(d2), (d2 - d1) / np.maximum(d2, 1e-300), np.inf)
        return tie, np.abs(d1 - self.max_sq) / self.max_sq

    def _terms(self, delta):
        delta = np.asarray(delta, dtype=np.float64)
        if self.correspondences is None:
            self.update_correspondences(delta)  # :170-172
        sel = np.flatnonzero(self.correspondences >= 0)
        c = self.correspondences[sel]
        p = self.source[sel]
        q = transform(delta, p)
        d = self.target[c] - q
        n, g = self.normals[c], self.gradients[c]
        u = g - (n * g).sum(axis=1)[:, None] * n  # :236-241
        rp = self.target_intensities[c] - self.source_intensities[sel] - (u * d).sum(axis=1)  # :207-209
        return sel, p, q, d, u, rp, self.mahalanobis

    def evaluate(self, delta, derivatives=True):
        delta = np.asarray(delta, dtype=np.float64)
        sel, p, q, d, u, rp, Mg = self._terms(delta)
        wp = self.photometric_term_weight
        wg = 1.0 - wp  # :174
        Md = np.einsum("nij,nj->ni", Mg, d)
        out = dict(error=float((wg * (d * Md).sum(axis=1) + wp * rp * rp).sum()), num_inliers=int(len(sel)))  # :204, :211
        if not derivatives:
            return out
        R = delta[:3, :3]
        Jt = np.concatenate([-hat(q), np.broadcast_to(np.eye(3), (len(sel), 3, 3))], axis=2)
        Js = np.concatenate([R[None] @ hat(p), np.broadcast_to(-R, (len(sel), 3, 3))], axis=2)
        M = wg * Mg + wp * u[:, :, None] * u[:, None, :]  # :229, :246
        w = wg * Md - (wp * rp)[:, None] * u              # :232, :249
        out["H_target"] = np.einsum("nki,nkl,nlj->ij", Jt, M, Jt)
        out["H_source"] = np.einsum("nki,nkl,nlj->ij", Js, M, Js)
        out["H_target_source"] = np.einsum("nki,nkl,nlj->ij", Jt, M, Js)
        out["b_target"] = np.einsum("nki,nk->i", Jt, w)
        out["b_source"] = np.einsum("nki,nk->i", Js, w)
        return out

    def linearize(self, delta):
        self.update_correspondences(delta)
        return self.evaluate(delta)

    def error(self, delta):
        return self.evaluate(delta, derivatives=False)["error"]

    def residuals(self, delta):
        _, _, _, d, _, rp, Mg = self._terms(delta)
        wp = self.photometric_term_weight
        L = np.linalg.cholesky(Mg)
        return np.concatenate([np.sqrt(1.0 - wp) * np.einsum("nji,nj->ni", L, d), np.sqrt(wp) * rp[:, None]], axis=1)

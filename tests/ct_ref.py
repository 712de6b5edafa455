"""numpy statement of the continuous-time ICP / GICP factors (factors/impl/integrated_ct_icp_factor_impl.hpp, integrated_ct_gicp_factor_impl.hpp), written out
independently of the kernels: the time table, the pose table with its two derivative blocks, the brute-force search with one pose per point, both per-point terms,
the records, error() on stored correspondences (and, for GICP, the stored M) and the deskewed points.  f64 on the f32 inputs; the pose table also evaluates in
np.longdouble, which is what the device's bound on it is measured against.

Conventions are GTSAM's Pose3: tangent (omega, v), full SE(3) exponential, right-trivialised derivatives.  Coefficients that cancel at a small angle are summed as
series below theta = 1/2, like the device's (csrc/gp_pose3_ct.hpp)."""
import math

import numpy as np

from pose3_ref import skew, so3_logmap

TIME_EPS = 1e-3
SERIES_THETA2 = 0.25


# ---- time table ------------------------------------------------------------------------------------------------------------------------------------------------


def time_table(times):
    """(:41-55) greedy and sequential, in index order, f64 on the f32 times: a new entry when t - table[-1] > 1e-3 (strict); then every entry over
    max(1e-9, table[-1]).  No sort, no offset."""
    table, indices = [], []
    for t in np.asarray(times, dtype=np.float32).astype(np.float64).ravel():
        if not table or t - table[-1] > TIME_EPS:
            table.append(t)
        indices.append(len(table) - 1)
    table = np.array(table, dtype=np.float64)
    if len(table):
        table = table / max(1e-9, table[-1])
    return table, np.array(indices, dtype=np.int32)


# ---- Pose3 pieces, any float dtype ------------------------------------------------------------------------------------------------------------------------------


def _alt_series(x, m, terms=9):
    """sum over k of (-x)^k / (2k + m)!"""
    dt = type(x)
    s = dt(0)
    for k in range(terms - 1, -1, -1):
        s = dt(1) / dt(math.factorial(2 * k + m)) - x * s
    return s


def so3_coeffs(th2):
    """A = sin/th, B = (1 - cos)/th^2, C = (th - sin)/th^3, D = (1 - th^2/2 - cos)/th^4, E = (th - sin - th^3/6)/th^5"""
    dt = type(th2)
    if th2 < SERIES_THETA2:
        return _alt_series(th2, 1), _alt_series(th2, 2), _alt_series(th2, 3), -_alt_series(th2, 4), -_alt_series(th2, 5)
    th = np.sqrt(th2)
    s, c = np.sin(th), np.cos(th)
    return s / th, (1 - c) / th2, (th - s) / (th2 * th), (1 - th2 / dt(2) - c) / (th2 * th2), (th - s - th2 * th / dt(6)) / (th2 * th2 * th)


_BERNOULLI = [(1, 12), (1, 720), (1, 30240), (1, 1209600), (1, 47900160), (691, 1307674368000), (1, 74724249600), (3617, 10670622842880000), (43867, 5109094217170944000)]


def so3_log_coeff(th2):
    """F = 1/th^2 - (1 + cos)/(2 th sin) = sum |B_2k| th^(2k-2) / (2k)!"""
    dt = type(th2)
    if th2 < SERIES_THETA2:
        s = dt(0)
        for num, den in reversed(_BERNOULLI):
            s = dt(num) / dt(den) + th2 * s
        return s
    th = np.sqrt(th2)
    return dt(1) / th2 - (1 + np.cos(th)) / (2 * th * np.sin(th))


def _eye(n, dt):
    return np.eye(n).astype(dt)


def inverse(T):
    out = _eye(4, T.dtype.type)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
    return out


def expmap(xi):
    """Pose3::Expmap"""
    dt = xi.dtype.type
    w, v = xi[:3], xi[3:]
    A, B, C, _, _ = so3_coeffs(w @ w)
    W = skew(w).astype(dt)
    T = _eye(4, dt)
    T[:3, :3] = _eye(3, dt) + A * W + B * (W @ W)
    T[:3, 3] = (_eye(3, dt) + B * W + C * (W @ W)) @ v
    return T


def logmap(T):
    """Pose3::Logmap: omega from SO3::Logmap, v = (I - W/2 + F W^2) t"""
    dt = T.dtype.type
    w = np.asarray(so3_logmap(T[:3, :3]), dtype=dt)
    W = skew(w).astype(dt)
    F = so3_log_coeff(w @ w)
    return np.concatenate([w, (_eye(3, dt) - W / dt(2) + F * (W @ W)) @ T[:3, 3]])


def adjoint(T):
    dt = T.dtype.type
    A = np.zeros((6, 6), dtype=dt)
    A[:3, :3] = T[:3, :3]
    A[3:, :3] = skew(T[:3, 3]).astype(dt) @ T[:3, :3]
    A[3:, 3:] = T[:3, :3]
    return A


def _q(xi):
    """Pose3::ComputeQforExpmapDerivative"""
    dt = xi.dtype.type
    W, V = skew(xi[:3]).astype(dt), skew(xi[3:]).astype(dt)
    _, _, C, D, E = so3_coeffs(xi[:3] @ xi[:3])
    WVW = W @ V @ W
    return (-V / dt(2) + C * (W @ V + V @ W - WVW) + D * (W @ W @ V + V @ W @ W - dt(3) * WVW) - (D - dt(3) * E) / dt(2) * (WVW @ W + W @ WVW))


def expmap_derivative(xi):
    """Pose3::ExpmapDerivative = [[Jw, 0], [Q, Jw]], Jw = I - B W + C W^2"""
    dt = xi.dtype.type
    W = skew(xi[:3]).astype(dt)
    _, B, C, _, _ = so3_coeffs(xi[:3] @ xi[:3])
    Jw = _eye(3, dt) - B * W + C * (W @ W)
    J = np.zeros((6, 6), dtype=dt)
    J[:3, :3], J[3:, 3:], J[3:, :3] = Jw, Jw, _q(xi)
    return J


def logmap_derivative(xi):
    """Pose3::LogmapDerivative at Exp(xi) = [[Ji, 0], [-Ji Q Ji, Ji]], Ji = I + W/2 + F W^2"""
    dt = xi.dtype.type
    W = skew(xi[:3]).astype(dt)
    Ji = _eye(3, dt) + W / dt(2) + so3_log_coeff(xi[:3] @ xi[:3]) * (W @ W)
    J = np.zeros((6, 6), dtype=dt)
    J[:3, :3], J[3:, 3:], J[3:, :3] = Ji, Ji, -(Ji @ _q(xi) @ Ji)
    return J


def pose_table(T0, T1, table, dtype=np.float64):
    """update_poses (:202-248): T [B, 4, 4], D0 [B, 6, 6], D1 [B, 6, 6] with T(t) = T0 Exp(t Log(T0^-1 T1))"""
    T0, T1 = np.asarray(T0).astype(dtype), np.asarray(T1).astype(dtype)
    delta = inverse(T0) @ T1
    vel = logmap(delta)
    H_vel_delta = logmap_derivative(vel)
    H_delta_0 = -adjoint(inverse(delta))
    Ts, D0s, D1s = [], [], []
    for t in np.asarray(table).astype(dtype):
        inc = expmap(t * vel)
        H_pose_delta = expmap_derivative(t * vel) @ H_vel_delta * t  # (H_pose_inc = I)
        Ts.append(T0 @ inc)
        D0s.append(adjoint(inverse(inc)) + H_pose_delta @ H_delta_0)
        D1s.append(H_pose_delta)  # (H_delta_1 = I)
    B = len(Ts)
    return np.array(Ts, dtype=dtype).reshape(B, 4, 4), np.array(D0s, dtype=dtype).reshape(B, 6, 6), np.array(D1s, dtype=dtype).reshape(B, 6, 6)


def pose_table_rows(T0, T1, table, dtype=np.float64):
    """the device's layout: [B][12 + 36 + 36], T(t) 3x4 | D0 | D1, all row-major"""
    T, D0, D1 = pose_table(T0, T1, table, dtype)
    return np.concatenate([T[:, :3, :].reshape(len(T), 12), D0.reshape(len(T), 36), D1.reshape(len(T), 36)], axis=1)


# ---- correspondences --------------------------------------------------------------------------------------------------------------------------------------------


def transform(T_tab, indices, points):
    p = np.asarray(points, dtype=np.float64)
    Ti = T_tab[indices]
    return np.einsum("nij,nj->ni", Ti[:, :3, :3], p) + Ti[:, :3, 3]


def nearest(queries, target_points, chunk=512):
    """brute force: (index of the nearest target point, its squared distance, the second-nearest squared distance), f64 on the f32 targets"""
    tp = np.asarray(target_points, dtype=np.float64)
    idx, d1, d2 = np.zeros(len(queries), np.int64), np.zeros(len(queries)), np.full(len(queries), np.inf)
    for a in range(0, len(queries), chunk):
        d = ((queries[a : a + chunk, None, :] - tp[None]) ** 2).sum(axis=2)
        rows, first = np.arange(len(d)), d.argmin(axis=1)  # (argmin: the lowest index among equals)
        idx[a : a + chunk], d1[a : a + chunk] = first, d[rows, first]
        if tp.shape[0] > 1:
            d[rows, first] = np.inf
            d2[a : a + chunk] = d.min(axis=1)
    return idx, d1, d2


def correspondences(T_tab, indices, points, target_points, max_sq_dist):
    """(:251-288) the nearest target point of T(t_i) p_i within the cut-off (strict, as the ICP factor's search), or -1"""
    if len(points) == 0:
        return np.zeros(0, np.int32)
    idx, d1, _ = nearest(transform(T_tab, indices, points), target_points)
    return np.where(d1 < max_sq_dist, idx, -1).astype(np.int32)


def margins(T_tab, indices, points, target_points, max_sq_dist):
    """what the exact-equality tests need of a fixture: (smallest gap between a query's nearest and second-nearest squared distance, smallest |nearest - cut-off|)"""
    _, d1, d2 = nearest(transform(T_tab, indices, points), target_points)
    return float((d2 - d1).min()), float(np.abs(d1 - max_sq_dist).min())


# ---- the factors -------------------------------------------------------------------------------------------------------------------------------------------------


def _sym(c):
    """the symmetric part of (N, 3, 3) covariances, as the device takes them"""
    c = np.asarray(c, dtype=np.float64).reshape(-1, 3, 3)
    return 0.5 * (c + c.transpose(0, 2, 1))


class CTFactorRef:
    """kind 0: CT-ICP (scalar point-to-plane residual e = n_B . (T p - x_B)); kind 1: CT-GICP (r = T p - x_B under M = (C_B + R C_A R^T)^-1 of the linearisation poses)"""

    def __init__(self, kind, target_points, target_normals, target_covs, points, covs, times, max_correspondence_distance=1.0):
        self.kind = kind
        self.tp = np.asarray(target_points, dtype=np.float32).astype(np.float64)
        self.tn = None if target_normals is None else np.asarray(target_normals, dtype=np.float32).astype(np.float64)
        self.tc = None if target_covs is None else _sym(np.asarray(target_covs, dtype=np.float32))
        self.p = np.asarray(points, dtype=np.float32).astype(np.float64).reshape(-1, 3)
        self.c = None if covs is None else _sym(np.asarray(covs, dtype=np.float32))
        self.table, self.indices = time_table(times)
        self.max_sq = float(max_correspondence_distance) ** 2
        self.corr = None
        self.M = None
        self.searches = 0

    # -- state --
    def update_correspondences(self, T0, T1, corr=None):
        """search at (T0, T1) -- or take `corr` as given (the device's own) -- and, for GICP, store M at those poses"""
        T, _, _ = pose_table(T0, T1, self.table)
        if corr is None:
            corr = correspondences(T, self.indices, self.p, self.tp, self.max_sq)
            self.searches += 1
        self.corr = np.asarray(corr, dtype=np.int32)
        if self.kind == 1:
            R = T[self.indices][:, :3, :3]
            j = np.maximum(self.corr, 0)
            self.M = np.linalg.inv(self.tc[j] + R @ self.c @ R.transpose(0, 2, 1))
        return self.corr

    # -- per-point pieces on the stored correspondences --
    def _matched(self, T0, T1):
        T, D0, D1 = pose_table(T0, T1, self.table)
        m = self.corr >= 0
        b, j = self.indices[m], self.corr[m]
        q = transform(T, b, self.p[m])
        return m, b, j, q, T, D0, D1

    def residuals(self, T0, T1):
        """stacked residuals whose squared norm is error(): e (N) for ICP, L r (N, 3) with M = L L^T for GICP"""
        m, _, j, q, _, _, _ = self._matched(T0, T1)
        r = q - self.tp[j]
        if self.kind == 0:
            return (r * self.tn[j]).sum(axis=1)
        L = np.linalg.cholesky(self.M[m])
        return np.einsum("nji,nj->ni", L, r)

    def error(self, T0, T1):
        if self.corr is None:
            self.update_correspondences(T0, T1)
        rho = self.residuals(T0, T1)
        return float((rho * rho).sum())

    def linearize(self, T0, T1, corr=None):
        self.update_correspondences(T0, T1, corr)
        return self.record(T0, T1)

    def record(self, T0, T1):
        m, b, j, q, T, D0, D1 = self._matched(T0, T1)
        R = T[b][:, :3, :3]
        p = self.p[m]
        S = np.zeros((len(p), 3, 3))
        S[:, 0, 1], S[:, 0, 2], S[:, 1, 0], S[:, 1, 2], S[:, 2, 0], S[:, 2, 1] = -p[:, 2], p[:, 1], p[:, 2], -p[:, 0], -p[:, 1], p[:, 0]
        J = np.concatenate([-(R @ S), R], axis=2)  # (N, 3, 6): d(T p) / d(local tangent of T)
        r = q - self.tp[j]
        if self.kind == 0:
            n = self.tn[j]
            e = (r * n).sum(axis=1)
            h = np.einsum("nk,nkj->nj", n, J)
            H0, H1 = np.einsum("ni,nij->nj", h, D0[b])[:, None, :], np.einsum("ni,nij->nj", h, D1[b])[:, None, :]
            M = np.ones((len(p), 1, 1))
            w = e[:, None]
            error = float((e * e).sum())
        else:
            H0, H1 = J @ D0[b], J @ D1[b]
            M = self.M[m]
            w = r
            error = float(np.einsum("ni,nij,nj->", r, M, r))
        MH0, MH1 = M @ H0, M @ H1
        Mw = np.einsum("nij,nj->ni", M, w)
        return {
            "H_target": np.einsum("nki,nkj->ij", H0, MH0),
            "H_source": np.einsum("nki,nkj->ij", H1, MH1),
            "H_target_source": np.einsum("nki,nkj->ij", H0, MH1),
            "b_target": np.einsum("nki,nk->i", H0, Mw),
            "b_source": np.einsum("nki,nk->i", H1, Mw),
            "error": error,
            "num_inliers": int(m.sum()),
        }

    def deskewed(self, T0, T1, local=False):
        T, _, _ = pose_table(T0, T1, self.table)
        if local:
            T = inverse(np.asarray(T0, dtype=np.float64))[None] @ T
        out = np.ones((len(self.p), 4))
        out[:, :3] = transform(T, self.indices, self.p)
        return out


def system12(L):
    """the 12x12 Gauss-Newton system of a record: (H, b) with H [[H_00, H_01], [H_01^T, H_11]] and b = [b_0, b_1] (the HessianFactor's g = -b)"""
    H = np.block([[L["H_target"], L["H_target_source"]], [L["H_target_source"].T, L["H_source"]]])
    return H, np.concatenate([L["b_target"], L["b_source"]])


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------------------------------------


def bins_to_times(bin_of_point):
    """f32 times whose table has one entry per distinct bin: bin b at b * 0.01 (gaps of ten time_eps)"""
    return (np.asarray(bin_of_point, dtype=np.float64) * 0.01).astype(np.float32)


def skewed_scan(n, T0, T1, bin_of_point, seed=7, target_points=6000, noise=0.0):
    """the synthetic walls seen from the origin twice: once as the target (with its normals and covariances), once -- another seed, so no point is shared -- as the
    world points w_i a sensor moving from T0 to T1 sees at its times t_i; the source holds p_i = T(t_i)^-1 w_i, so deskewing with (T0, T1) puts it back on the
    walls.  Returns a dict of f32 arrays."""
    from gtsam_points_amd import synthetic

    walls = synthetic.make_walls(42)
    tp, tn = synthetic.cast_scan(target_points, seed=seed, walls=walls, rings=32, noise=noise)
    wp, wn = synthetic.cast_scan(n, seed=seed + 1, walls=walls, rings=32, noise=noise)
    times = bins_to_times(bin_of_point)
    table, indices = time_table(times)
    T, _, _ = pose_table(T0, T1, table)
    Ti = T[indices]
    R, t = Ti[:, :3, :3], Ti[:, :3, 3]
    sp = np.einsum("nji,nj->ni", R, wp.astype(np.float64) - t).astype(np.float32)
    sn = np.einsum("nji,nj->ni", R, wn.astype(np.float64)).astype(np.float32)
    return dict(target_points=tp, target_normals=tn, target_covs=synthetic.covs_from_normals(tn), points=sp, covs=synthetic.covs_from_normals(sn), times=times)

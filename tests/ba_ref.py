"""numpy restatement of the BALM eigenvalue-minimisation factors (PlaneEVMFactor / EdgeEVMFactor, Liu & Zhang, RA-L 2021) in a chosen dtype (float64 / longdouble).

  literal    BALMFeature, Ji, Hij (t1 + t2 + t3 with Fmn), every (i, j) block of the 3N x 3N point Hessian, its upper triangle mirrored (selfadjointView<Upper>),
             D^T H D and -J D.  The (i, j) loop is carried out by broadcasting; the formulas are term for term the reference's.  One deviation: the covariance is
             formed from centred points (the raw-moment formula loses the digits that a yardstick must keep far from the origin).
  collapsed  the O(N) form the device computes: per-pose sums s_a, g_{m,a}, B_a, r_a and outer products of 6-vectors; in the edge factor the (k, m) = (0, 1) and
             (1, 0) terms, which cancel identically, are omitted.
A factor is (G [6K, 6K], g [6K], f) over its poses in ascending pose order.
"""
import numpy as np

PLANE, EDGE = 0, 1

# The largest deviation of the collapsed float64 restatement from the literal longdouble one over all fixture cases (deviation() below: per 6 x 6 block of G, per
# 6-block of g, and f, each relative to the block's own max-norm), as tests/test_ba_ref_cpu.py::test_measured_tolerance computes it: MEASURED_F64_DEVIATION is that
# figure rounded up; the test holds the computed value to at most this constant and at least a quarter of it.  The device is held to 4 x: it orders its
# sums as the collapsed form does, the factor covers its tree reductions and its Jacobi eigen-solver.
# What sets the figure: features whose points all lie on ONE pose.  lambda does not change when the whole feature moves rigidly, so their G_aa is what is left when
# c B_a and c s_a s_a^T / N (entries ~20 near the origin) cancel: entries ~1e-5, which float64 holds to ~1e-9 of themselves.  Features on two or more poses stay
# below 1e-11.
MEASURED_F64_DEVIATION = 1.0e-8  # measured 7.99e-9, at a 23-point single-pose feature of the 300-feature batch
GPU_BOUND = 4.0 * MEASURED_F64_DEVIATION
# The same cancellation 1e3 from the origin: c B_a has entries ~3e5 there (q x u grows with |q|), the G_aa left over still ~1e-5, and float64 -- in this restatement
# as on the device -- holds it to ~1e-5 of itself.  That one fixture (single_pose_far_case: 64 points, one pose) has a constant of its own, measured the same way
# and held by test_measured_tolerance_single_pose_far; the batch far from the origin has no single-pose feature.  Its g is zero, its f an ordinary eigenvalue.
SINGLE_POSE_FAR_DEVIATION = 1.5e-5  # measured 1.07e-5
# Blocks that are ZERO in exact arithmetic have no max-norm to be relative to; they alone are measured against RESIDUAL_FLOOR x the size of their terms:
#   every block (G, g, f) of a plane factor with N = 3 points -- three points always lie in a plane, lambda_0 is identically zero;
#   g of a feature on one pose -- lambda does not change under a rigid motion of the whole feature.
# The term sizes: for G_ab the block-diagonal term c B_a (geometric mean over a and b), for g_a and f the sums with residuals as large as the points' distances to
# the mean.  No other block is given a floor: collapsed_factor(with_scales=True) names the zero blocks, denominators() applies the floor to them only.
RESIDUAL_FLOOR = 1e-6


def skew(v, dtype):
    z = dtype(0)
    return np.array([[z, -v[2], v[1]], [v[2], z, -v[0]], [-v[1], v[0], z]], dtype=dtype)


def expmap(xi, dtype=np.float64):
    """SE(3) exponential, tangent (omega, v), in dtype"""
    xi = np.asarray(xi, dtype=dtype)
    w, v = xi[:3], xi[3:]
    th = np.sqrt(w @ w)
    W = skew(w, dtype)
    I = np.eye(3, dtype=dtype)
    if th < 1e-6:
        A, B, Cc = dtype(1) - th * th / 6, dtype(0.5) - th * th / 24, dtype(1) / 6 - th * th / 120
    else:
        A, B, Cc = np.sin(th) / th, (1 - np.cos(th)) / (th * th), (th - np.sin(th)) / (th * th * th)
    T = np.eye(4, dtype=dtype)
    T[:3, :3] = I + A * W + B * (W @ W)
    T[:3, 3] = (I + B * W + Cc * (W @ W)) @ v
    return T


def eigh3(A):
    """eigenpairs of a symmetric 3 x 3 in A's dtype, ascending: cyclic Jacobi to convergence"""
    dtype = A.dtype.type
    a = A.copy()
    V = np.eye(3, dtype=dtype)
    with np.errstate(over="ignore"):
        return _jacobi(a, V, dtype)


def _jacobi(a, V, dtype):
    for _ in range(30):
        off = abs(a[0, 1]) + abs(a[0, 2]) + abs(a[1, 2])
        if off == 0:
            break
        for p, q in ((0, 1), (0, 2), (1, 2)):
            if a[p, q] == 0:
                continue
            theta = (a[q, q] - a[p, p]) / (2 * a[p, q])
            t = np.sign(theta) / (abs(theta) + np.sqrt(theta * theta + 1)) if theta != 0 else dtype(1)
            c = 1 / np.sqrt(t * t + 1)
            s = t * c
            J = np.eye(3, dtype=dtype)
            J[p, p] = c
            J[q, q] = c
            J[p, q] = s
            J[q, p] = -s
            a = J.T @ a @ J
            a[p, q] = a[q, p] = 0
            V = V @ J
    order = np.argsort(np.diag(a), kind="stable")
    return np.diag(a)[order].copy(), V[:, order].copy()


def transform(points, poses_of_points, values, dtype):
    """q_i = T_pose(i) p_i in dtype"""
    T = np.asarray(values, dtype=dtype)[np.asarray(poses_of_points)]
    p = np.asarray(points, dtype=dtype)
    return np.einsum("nij,nj->ni", T[:, :3, :3], p) + T[:, :3, 3]


class BALMFeature:
    """balm_feature.hpp: mean, cov, eigenpairs; Ji, Fmn, Hij"""

    def __init__(self, q):
        self.dtype = q.dtype.type
        self.N = len(q)
        self.mean = q.sum(0) / self.N
        d = q - self.mean
        self.cov = d.T @ d / self.N
        self.eigenvalues, self.eigenvectors = eigh3(self.cov)

    def Ji(self, k, q):
        """[N, 3]: row i = 2/N (q_i - mean)^T u_k u_k^T"""
        u = self.eigenvectors[:, k]
        return (2 / self.dtype(self.N)) * ((q - self.mean) @ u)[:, None] * u[None, :]

    def Fmn(self, m, n, q):
        """[N, 3]: row j = (q_j - mean)^T / (N (l_n - l_m)) (u_m u_n^T + u_n u_m^T); zero for m = n"""
        if m == n:
            return np.zeros((len(q), 3), dtype=self.dtype)
        l, U = self.eigenvalues, self.eigenvectors
        rhs = np.outer(U[:, m], U[:, n]) + np.outer(U[:, n], U[:, m])
        return ((q - self.mean) / (self.N * (l[n] - l[m]))) @ rhs

    def H(self, k, q):
        """the 3N x 3N point Hessian of lambda_k: block (i, j) = 2/N (t1 + t2 + t3), computed for j >= i and mirrored"""
        N, U = self.N, self.eigenvectors
        u = U[:, k]
        d = q - self.mean
        Fk = np.stack([self.Fmn(0, k, q), self.Fmn(1, k, q), self.Fmn(2, k, q)], axis=1)  # [j, m, :]
        UF = np.einsum("rm,jmc->jrc", U, Fk)  # U F_k of p_j
        t2 = np.einsum("r,ijc->ijrc", u, np.einsum("is,jsc->ijc", d, UF))  # u_k (p_i - mean)^T U F_k
        t3 = np.einsum("jrc,i->ijrc", UF, d @ u)  # U F_k (u_k^T (p_i - mean))
        uu = np.outer(u, u)
        H = t2
        H += t3
        H -= uu / self.dtype(N)  # t1: -1/N off the diagonal ...
        H[np.arange(N), np.arange(N)] += uu  # ... and (N - 1)/N on it
        H *= 2 / self.dtype(N)
        H = H.transpose(0, 2, 1, 3).reshape(3 * N, 3 * N)
        upper = np.triu(H)
        return upper + np.triu(H, 1).T


def _segments(poses_of_points):
    poses = sorted(set(int(p) for p in poses_of_points))
    return poses, {p: i for i, p in enumerate(poses)}


def literal_factor(kind, points, poses_of_points, values, scale=1.0, dtype=np.longdouble):
    """the reference's linearize(): (G, g, f) over the factor's poses in ascending order"""
    q = transform(points, poses_of_points, values, dtype)
    N = len(q)
    poses, index = _segments(poses_of_points)
    feat = BALMFeature(q)
    ks = (0,) if kind == PLANE else (0, 1)
    H = sum(feat.H(k, q) for k in ks)
    J = sum(feat.Ji(k, q) for k in ks).reshape(1, 3 * N)
    f = sum(feat.eigenvalues[k] for k in ks)
    D = np.zeros((3 * N, 6 * len(poses)), dtype=dtype)
    for i in range(N):
        a = index[int(poses_of_points[i])]
        D[3 * i:3 * i + 3, 6 * a:6 * a + 3] = -skew(q[i], dtype)
        D[3 * i:3 * i + 3, 6 * a + 3:6 * a + 6] = np.eye(3, dtype=dtype)
    s = dtype(scale) if kind == PLANE else dtype(1)  # (EdgeEVMFactor does not apply error_scale)
    return s * (D.T @ H @ D), s * (-(J @ D)).reshape(-1), s * f


def factor_error(kind, points, poses_of_points, values, scale=1.0, dtype=np.longdouble):
    l = BALMFeature(transform(points, poses_of_points, values, dtype)).eigenvalues
    return dtype(scale) * l[0] if kind == PLANE else l[0] + l[1]


def collapsed_factor(kind, points, poses_of_points, values, scale=1.0, dtype=np.float64, with_scales=False):
    """the O(N) form: (G, g, f); with_scales also returns the rounding scales of g's blocks and of f (see RESIDUAL_FLOOR)"""
    q = transform(points, poses_of_points, values, dtype)
    N = dtype(len(q))
    poses, index = _segments(poses_of_points)
    K = len(poses)
    seg = np.array([index[int(p)] for p in poses_of_points])
    feat = BALMFeature(q)
    l, U = feat.eigenvalues, feat.eigenvectors
    d = q - feat.mean
    a = d @ U  # a[:, m] = d_i . u_m

    def Dt(w):  # rows D_i^T w_i = (q_i x w_i ; w_i)
        return np.concatenate([np.cross(q, w), w], axis=1)

    def per_pose(rows):
        out = np.zeros((K,) + rows.shape[1:], dtype=dtype)
        for i in range(len(rows)):  # in point order, as the device folds a segment
            out[seg[i]] += rows[i]
        return out

    s = dtype(scale) if kind == PLANE else dtype(1)
    c = s * 2 / N
    G = np.zeros((6 * K, 6 * K), dtype=dtype)
    r = np.zeros((K, 6), dtype=dtype)
    B = np.zeros((K, 6, 6), dtype=dtype)
    terms = []  # (coefficient, per-pose 6-vectors)
    for k in ((0,) if kind == PLANE else (0, 1)):
        x = Dt(np.broadcast_to(U[:, k], q.shape))
        terms.append((-1 / N, per_pose(x)))
        for m in range(3):
            if m == k or (kind == EDGE and m < 2):  # (edge: the (0, 1) and (1, 0) terms cancel)
                continue
            w = a[:, m:m + 1] * U[:, k] + a[:, k:k + 1] * U[:, m]
            terms.append((1 / (N * (l[k] - l[m])), per_pose(Dt(w))))
        B += per_pose(x[:, :, None] * x[:, None, :])
        r += per_pose(a[:, k:k + 1] * x)
    for A_ in range(K):
        for B_ in range(K):
            blk = B[A_].copy() if A_ == B_ else np.zeros((6, 6), dtype=dtype)
            for coef, V in terms:
                blk += coef * np.outer(V[A_], V[B_])
            G[6 * A_:6 * A_ + 6, 6 * B_:6 * B_ + 6] = c * blk
    g = (-c * r).reshape(-1)
    f = s * l[0] if kind == PLANE else l[0] + l[1]
    if not with_scales:
        return G, g, f
    dn = np.sqrt((d * d).sum(1))
    xs = sum(np.abs(Dt(np.broadcast_to(U[:, k], q.shape))).max(1) for k in ((0,) if kind == PLANE else (0, 1)))
    g_scale = np.array([float(abs(c) * (dn * xs)[seg == A_].sum()) for A_ in range(K)])
    b_scale = np.array([float(abs(c) * (xs * xs)[seg == A_].sum()) for A_ in range(K)])  # the size of the block-diagonal term c B_a
    zero = "all" if kind == PLANE and len(q) == 3 else ("g" if K == 1 else "")  # what is zero in exact arithmetic (see RESIDUAL_FLOOR)
    return G, g, f, (np.sqrt(np.outer(b_scale, b_scale)), g_scale, float(abs(s) * np.trace(feat.cov)), zero)


def denominators(ref, scales):
    """what deviation() divides by: per 6 x 6 block of G (-> [K, K]), per 6-block of g (-> [K]) and for f the block's own max-norm, except where the block is zero
    in exact arithmetic (RESIDUAL_FLOOR x the size of its terms)"""
    G_scale, g_scale, f_scale, zero = scales
    Gr, gr, fr = ref
    K = len(gr) // 6
    dG = np.array([[float(np.abs(Gr[6 * a:6 * a + 6, 6 * b:6 * b + 6]).max()) for b in range(K)] for a in range(K)])
    dg = np.array([float(np.abs(gr[6 * a:6 * a + 6]).max()) for a in range(K)])
    df = float(abs(fr))
    if zero == "all":
        dG, df = RESIDUAL_FLOOR * G_scale, RESIDUAL_FLOOR * f_scale
    if zero in ("all", "g"):
        dg = RESIDUAL_FLOOR * g_scale
    return dG, dg, df


def deviation(got, ref, scales):
    """the largest of: per 6 x 6 block of G and per 6-block of g, max|got - ref| / max|ref|; |f - f_ref| / |f_ref| (denominators())"""
    G, g, f = (np.asarray(x, dtype=np.longdouble) for x in got)
    Gr, gr, fr = (np.asarray(x, dtype=np.longdouble) for x in ref)
    dG, dg, df = denominators((Gr, gr, fr), scales)
    K = len(gr) // 6
    worst = float(abs(f - fr)) / df
    for a in range(K):
        for b in range(K):
            sl = (slice(6 * a, 6 * a + 6), slice(6 * b, 6 * b + 6))
            worst = max(worst, float(np.abs(G[sl] - Gr[sl]).max()) / dG[a, b])
        worst = max(worst, float(np.abs(g[6 * a:6 * a + 6] - gr[6 * a:6 * a + 6]).max()) / dg[a])
    return worst


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------------------------------------

def trajectory(K, rng, far=0.0):
    """K poses along a gently turning path; far: the norm of a common offset of every translation"""
    poses = []
    for k in range(K):
        xi = np.concatenate([0.05 * rng.standard_normal(3) + [0, 0, 0.02 * k], [0.5 * k, 0.1 * np.sin(k), 0.0] + 0.05 * rng.standard_normal(3)])
        T = expmap(xi)
        T[:3, 3] += far * np.array([0.6, -0.64, 0.48])
        poses.append(T)
    return np.stack(poses)


def perturbed(values, rng, rot=2e-3, trans=5e-3):
    """the linearisation point: every pose moved a little, so that the residuals are not the noise alone"""
    return np.stack([expmap(np.concatenate([rot * rng.standard_normal(3), trans * rng.standard_normal(3)])) @ T for T in values])


def _frame(rng):
    Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return Q


def make_feature(kind, N, pose_list, truth, rng, centre=None, order="sorted"):
    """one feature of N points dealt to the poses of pose_list (every pose at least once when N allows): world points on a 2 : 1 (or longer) rectangle with noise
    along the normal (plane), or on a segment with 2 : 1 anisotropic noise across it (edge), carried into each observing pose's frame.  -> (points [N, 3], poses [N])"""
    Q = _frame(rng)
    c = np.asarray(centre if centre is not None else truth[pose_list[0]][:3, 3] + rng.uniform(-2, 2, 3) + [0, 0, 3.0])
    if kind == PLANE:
        w = c + np.outer(rng.uniform(-1.0, 1.0, N), Q[:, 0]) + np.outer(rng.uniform(-0.45, 0.45, N), Q[:, 1]) + np.outer(2e-3 * rng.standard_normal(N), Q[:, 2])
    else:
        w = c + np.outer(rng.uniform(-1.0, 1.0, N), Q[:, 0]) + np.outer(4e-3 * rng.standard_normal(N), Q[:, 1]) + np.outer(2e-3 * rng.standard_normal(N), Q[:, 2])
    K = len(pose_list)
    if order == "sorted":
        pose = np.sort(np.array([pose_list[i % K] for i in range(N)]))
    else:  # dealt round robin: the keys arrive out of order
        pose = np.array([pose_list[(N - 1 - i) % K] for i in range(N)])
    p = np.stack([np.linalg.inv(truth[pose[i]]) @ np.append(w[i], 1.0) for i in range(N)])[:, :3]
    return p, pose


def eigen_gaps(kind, points, pose, values):
    """the pairwise gaps (l1 - l0) / l1, (l2 - l1) / l2, (l2 - l0) / l2 at `values`"""
    l = BALMFeature(transform(points, pose, values, np.longdouble)).eigenvalues
    return float((l[1] - l[0]) / l[1]), float((l[2] - l[1]) / l[2]), float((l[2] - l[0]) / l[2])


SINGLE_N = (3, 4, 63, 64, 65, 129, 1025)
SINGLE_K = (1, 2, 3, 8, 33)


def single_cases():
    """(name, kind, N, K, order, scale, far): every N and every K of the lists, for both kinds; segments of one point (N = K), all points on one pose (K = 1), keys out
    of order, a scale"""
    cases = []
    for kind in (PLANE, EDGE):
        for N, K in ((3, 1), (3, 3), (4, 2), (63, 8), (64, 33), (65, 3), (129, 33), (1025, 2), (33, 33), (200, 1)):
            cases.append((f"{'plane' if kind == PLANE else 'edge'}-N{N}-K{K}", kind, N, K, "sorted", 1.0, 0.0))
        cases.append((f"{'plane' if kind == PLANE else 'edge'}-unordered", kind, 65, 8, "dealt", 1.0, 0.0))
        cases.append((f"{'plane' if kind == PLANE else 'edge'}-scaled", kind, 64, 3, "dealt", 2.5, 0.0))
        cases.append((f"{'plane' if kind == PLANE else 'edge'}-far", kind, 63, 3, "sorted", 1.0, 1e3))
    return cases


def build_single(case, seed=0):
    """-> (kind, points, pose, values, scale) of a single-factor case; the gaps are the fixture's own (the generator is deterministic)"""
    name, kind, N, K, order, scale, far = case
    rng = np.random.default_rng(1000 + seed + 7 * N + 131 * K + kind)
    for _ in range(200):  # (a draw whose eigenvalue gaps fall below 0.25 is drawn again: N = 3 or 4 points have no shape to speak of)
        truth = trajectory(K, rng, far)
        pose_list = list(rng.permutation(K)) if order == "dealt" else list(range(K))
        p, pose = make_feature(kind, N, pose_list, truth, rng, order=order)
        values = perturbed(truth, rng)
        if min(eigen_gaps(kind, p, pose, values)) >= 0.25:
            return kind, p, pose, values, scale
    raise AssertionError(name)


def build_batch(F, num_poses, seed=0, far=0.0, unseen=None):
    """F features of mixed kinds and lengths over num_poses poses (none touches pose `unseen`): -> (features [(kind, points, pose, scale)], truth, values)"""
    rng = np.random.default_rng(5000 + seed + F)
    truth = trajectory(num_poses, rng, far)
    values = perturbed(truth, rng)
    seen = [k for k in range(num_poses) if k != unseen]
    feats = []
    while len(feats) < F:
        kind = PLANE if len(feats) % 3 != 2 else EDGE
        K = int(rng.integers(2 if far else 1, min(len(seen), 6) + 1))  # (no single-pose feature far from the origin: single_pose_far_case)
        pose_list = sorted(rng.choice(seen, size=K, replace=False).tolist())
        N = int(rng.integers(max(6, K), 90 if F <= 100 else 40))
        p, pose = make_feature(kind, N, pose_list, truth, rng, order="dealt" if len(feats) % 2 else "sorted")
        if min(eigen_gaps(kind, p, pose, values)) >= 0.25:
            feats.append((kind, p, pose, 1.0 + 0.5 * (len(feats) % 4) if kind == PLANE else 1.0))
    return feats, truth, values


def dense_system(feats, factors, slot, num_slots, dtype=np.longdouble):
    """A, b, c of the factors (G, g, f) scattered by slot (a negative slot drops out; every f stays in c)"""
    A, b, c = np.zeros((6 * num_slots, 6 * num_slots), dtype=dtype), np.zeros(6 * num_slots, dtype=dtype), dtype(0)
    for (kind, p, pose, scale), (G, g, f) in zip(feats, factors):
        poses, _ = _segments(pose)
        c += f
        for i, pa in enumerate(poses):
            if slot[pa] < 0:
                continue
            b[6 * slot[pa]:6 * slot[pa] + 6] += g[6 * i:6 * i + 6]
            for j, pb in enumerate(poses):
                if slot[pb] >= 0:
                    A[6 * slot[pa]:6 * slot[pa] + 6, 6 * slot[pb]:6 * slot[pb] + 6] += G[6 * i:6 * i + 6, 6 * j:6 * j + 6]
    return A, b, c


def gauss_newton(system_at, values, slot, iterations, lam, dtype):
    """damped Gauss-Newton with the left update T <- Exp(xi) T: system_at(values) -> (A, b, c); -> the iterates' values and costs"""
    values = np.asarray(values, dtype=dtype).copy()
    out, costs = [], []
    for _ in range(iterations):
        A, b, c = system_at(values)
        x = solve_spd(A + lam * np.eye(len(b), dtype=dtype), b)
        for k in range(len(values)):
            if slot[k] >= 0:
                values[k] = expmap(x[6 * slot[k]:6 * slot[k] + 6], dtype) @ values[k]
        out.append(values.copy())
        costs.append(c)
    return out, costs


def solve_spd(A, b):
    """A x = b by Cholesky in A's dtype (numpy's solvers stop at float64)"""
    n = len(b)
    L = np.zeros_like(A)
    for j in range(n):
        L[j, j] = np.sqrt(A[j, j] - L[j, :j] @ L[j, :j])
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    y = np.zeros_like(b)
    for i in range(n):
        y[i] = (b[i] - L[i, :i] @ y[:i]) / L[i, i]
    x = np.zeros_like(b)
    for i in reversed(range(n)):
        x[i] = (y[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


_REFERENCES = {}


def reference_single(case):
    """(kind, points, pose, values, scale, literal longdouble factor, collapsed float64 factor, scales) of a single case, computed once per process"""
    if case[0] not in _REFERENCES:
        kind, p, pose, values, scale = build_single(case)
        G, g, f, scales = collapsed_factor(kind, p, pose, values, scale, np.float64, True)
        _REFERENCES[case[0]] = (kind, p, pose, values, scale, literal_factor(kind, p, pose, values, scale), (G, g, f), scales)
    return _REFERENCES[case[0]]


BATCHES = ((1, 3, 0.0, None), (2, 4, 0.0, None), (65, 8, 0.0, 5), (300, 12, 0.0, None), (65, 8, 1e3, None))  # (F, poses, far, a pose that no feature sees)


def reference_batch(cfg):
    """(features, values, literal longdouble factors, collapsed float64 factors, scales) of a batch, computed once per process"""
    if cfg not in _REFERENCES:
        F, P, far, unseen = cfg
        feats, _, values = build_batch(F, P, far=far, unseen=unseen)
        col = [collapsed_factor(k, p, pose, values, sc, np.float64, True) for k, p, pose, sc in feats]
        _REFERENCES[cfg] = (feats, values, [literal_factor(k, p, pose, values, sc) for k, p, pose, sc in feats], [c[:3] for c in col], [c[3] for c in col])
    return _REFERENCES[cfg]


def dense_denominators(feats, factors, scales, slot, num_slots):
    """what a deviation of the assembled A, b, c is relative to: per entry the SUM over the features of the denominators deviation() gives their blocks"""
    dA, db, dc = np.zeros((6 * num_slots, 6 * num_slots)), np.zeros(6 * num_slots), 0.0
    for (kind, p, pose, scale), factor, sc in zip(feats, factors, scales):
        poses, _ = _segments(pose)
        dG, dg, df = denominators(factor, sc)
        dc += df
        for i, pa in enumerate(poses):
            if slot[pa] < 0:
                continue
            db[6 * slot[pa]:6 * slot[pa] + 6] += dg[i]
            for j, pb in enumerate(poses):
                if slot[pb] >= 0:
                    dA[6 * slot[pa]:6 * slot[pa] + 6, 6 * slot[pb]:6 * slot[pb] + 6] += dG[i, j]
    return dA, db, dc


def single_pose_far_case():
    """a plane feature whose points all lie on ONE pose 1e3 from the origin (see SINGLE_POSE_FAR_DEVIATION): -> as reference_single"""
    return reference_single(("plane-far-K1", PLANE, 64, 1, "sorted", 1.0, 1e3))


def near_degenerate_edge(gap=5e-7, seed=11):
    """an edge feature of 40 points over three poses whose lambda_0 and lambda_1 lie `gap` apart (relative) at the values returned: a generic edge fixture, its cross
    section stretched along u_0 in the world frame until lambda_0 = (1 - gap) lambda_1, then carried back into the poses' frames.  -> (points, pose, values)"""
    rng = np.random.default_rng(seed)
    truth = trajectory(3, rng)
    p, pose = make_feature(EDGE, 40, [0, 1, 2], truth, rng)
    values = perturbed(truth, rng)
    q = transform(p, pose, values, np.longdouble)
    feat = BALMFeature(q)
    l, U = feat.eigenvalues, feat.eigenvectors
    alpha = np.sqrt(l[1] * (1 - np.longdouble(gap)) / l[0])
    d = q - feat.mean
    w = feat.mean + d + (alpha - 1) * np.outer(d @ U[:, 0], U[:, 0])
    inv = np.linalg.inv(values)
    return np.stack([inv[pose[i], :3, :3] @ np.asarray(w[i], dtype=np.float64) + inv[pose[i], :3, 3] for i in range(len(w))]), pose, values

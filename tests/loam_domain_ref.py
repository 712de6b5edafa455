"""Inputs and statements of the LOAM factor-domain sweep (tests/test_loam_domain_gpu.py, tests/test_loam_domain_ref_cpu.py).  A helper, not a test.

The scene, the placements and the poses are tests/factor_domain_ref.py's (scan_to_map / both_far / scaled, with its face-margin filter and DROP_CAP); the f64
statement is tests/loam_ref.py's (the reference's CROSS-PRODUCT form).  The target cloud serves as edge target and as plane target, the source as both sources.

mform() restates both terms the way the kernel sums them, in any numpy float type (np.longdouble for the precision check): d = x_j - q, q = T p,
  edge   v = x_j - x_l, M = (|v|^2 I - v v^T) / |v|^2          (full, rank 2)
  plane  n = normalize((x_j - x_l) x (x_j - x_m)), M = diag(n o n)
  error = sum d^T M d, H = sum J^T M J, b = sum J^T M d, J_t = [-[q]x, I], J_s = [R [p]x, -R]
on the correspondences a PartRef has stored.

cluster_scene(): the near-degenerate neighbours of section 3 -- 257 isolated clusters 5 m apart along x, each of exactly K + 1 target points with a prescribed
edge length (K = 2) or sine of the triple (K = 3), one source point beside each.  Every coordinate that carries the prescribed geometry lies on a grid f32 holds
exactly at |x| < 8192 (2^-10 m), except the small offset itself, which lies in the y-z plane where the origin placement resolves 6e-8 m; translated by 10 km along
factor_domain_ref.DIRECTION (6000, -6400, 4800: integers) that offset meets the 0.5 mm f32 grid, which is what realised() reports."""
import numpy as np

import factor_domain_ref as fd
import loam_ref

PARITY_TOL = 1e-7  # tests/test_loam_gpu.py
GATE = 1e-5        # the north-star gate
MARGIN = 1e-9      # tests/test_loam_gpu.py's input condition
SINE = 1e-6
NEARBY = np.array([0.002, -0.001, 0.003, 0.01, 0.02, -0.01])
KINDS = ["edge", "plane", "loam"]
CUTOFFS = [1.0, 0.5]
CASES_A = [(t, r) for t in fd.DISTANCES for r in fd.ROTATIONS]


def tolerance(far):
    """what the GPU tests assert: the project's own tolerance at |t| = 0, in the controls and in other units; the gate further out"""
    return GATE if far else PARITY_TOL


def sweep():
    """every case of the sweep: (name, maker in factor_domain_ref, its arguments, cut-off in the case's units, far)"""
    for t, r in CASES_A:
        for c in CUTOFFS:
            yield f"a {t:g} m {r} cutoff {c:g}", "scan_to_map", (t, r), c, t > 0
    for c in CUTOFFS:
        yield f"b both far cutoff {c:g}", "both_far", (), c, False
    for s in fd.SCALES:
        yield f"c scale {s:g}", "scaled", (s,), s, False


_CASES = {}


def case(maker, args):
    """(inputs, delta, nearby pose, dropped share, unit of length) of one placement, made once and shared (never written to)"""
    key = (maker,) + tuple(args)
    if key not in _CASES:
        d, delta, _, dropped = getattr(fd, maker)(*args)
        assert dropped <= fd.DROP_CAP
        unit = args[0] if maker == "scaled" else 1.0
        step = fd.expmap(NEARBY)
        step[:3, 3] *= unit
        _CASES[key] = (d, delta, delta @ step, dropped, unit)
    return _CASES[key]


def non_orthonormal(delta):
    """test_loam_gpu.py::test_non_orthonormal_pose_uses_the_block_as_given's perturbation: the 3x3 block orthonormal to 1e-6 only (the general kernels)"""
    out = np.array(delta, dtype=np.float64)
    out[:3, :3] = out[:3, :3] @ (np.eye(3) + 1e-6 * np.random.default_rng(11).normal(size=(3, 3)))
    return out


def make_ref(kind, target, source, cutoff):
    if kind == "edge":
        return loam_ref.EdgeFactorRef(target, source, cutoff)
    if kind == "plane":
        return loam_ref.PlaneFactorRef(target, source, cutoff)
    return loam_ref.LOAMFactorRef(target, target, source, source, cutoff)


def conditioned(ref, delta, what, validation=False):
    """test_loam_gpu._conditioned: tie, cut-off and length margins > 1e-9, sine > 1e-6, the validation margin > 1e-9 rad -> the smallest margins per part"""
    lows = {}
    for part in ref.parts:
        m = part.margins(delta, validation)
        low = {k: (float(v.min()) if len(v) else np.inf) for k, v in m.items()}
        print(f"[loam domain] {what} K={part.K}: smallest margins {low}")
        assert low["tie"] > MARGIN and low["cut"] > MARGIN and low["length"] > MARGIN, f"{what}: a correspondence two f64 implementations could decide differently {low}"
        assert low.get("sine", 1.0) > SINE and low.get("theta", 1.0) > MARGIN, f"{what}: {low}"
        lows[part.K] = low
    return lows


def _mform_part(part, delta, dt):
    sel = np.flatnonzero(part.correspondences[:, 0] >= 0)
    c = part.correspondences[sel]
    T = np.asarray(delta).astype(dt)
    R, t = T[:3, :3], T[:3, 3]
    p = part.source[sel].astype(dt)
    x = part.target.astype(dt)
    q = p @ R.T + t
    xj = x[c[:, 0]]
    d = xj - q
    eye = np.broadcast_to(np.eye(3, dtype=dt), (len(sel), 3, 3))
    with np.errstate(invalid="ignore", divide="ignore"):
        if part.K == 2:
            v = xj - x[c[:, 1]]
            vv = (v * v).sum(1)
            M = (vv[:, None, None] * eye - v[:, :, None] * v[:, None, :]) / vv[:, None, None]
        else:
            n = np.cross(xj - x[c[:, 1]], xj - x[c[:, 2]])
            n = n / np.sqrt((n * n).sum(1))[:, None]
            M = (n * n)[:, :, None] * eye
    Jt = np.concatenate([-fd._hat(q, dt), eye], axis=2)
    Js = np.concatenate([np.einsum("ij,njk->nik", R, fd._hat(p, dt)), np.broadcast_to(-R, (len(sel), 3, 3))], axis=2)
    Md = np.einsum("nij,nj->ni", M, d)
    return dict(
        num_inliers=int(len(sel)),
        error=(d * Md).sum(),
        H_target=np.einsum("nki,nkl,nlj->ij", Jt, M, Jt),
        H_source=np.einsum("nki,nkl,nlj->ij", Js, M, Js),
        H_target_source=np.einsum("nki,nkl,nlj->ij", Jt, M, Js),
        b_target=np.einsum("nki,nk->i", Jt, Md),
        b_source=np.einsum("nki,nk->i", Js, Md),
    )


def mform(ref, delta, dtype=np.longdouble):
    """the M-form record at `delta` on the correspondences `ref` (a PartRef or a LOAMFactorRef) has stored, every operation and every sum in `dtype`"""
    parts = [_mform_part(p, delta, dtype) for p in ref.parts]
    return {k: sum(p[k] for p in parts[1:]) + parts[0][k] if len(parts) > 1 else parts[0][k] for k in parts[0]}


def agreement(L, X):
    """(worst block, error) of an f64 record L against a record X in a wider type, norm-wise relative, the differences formed in X's type"""
    dt = X["error"].dtype
    worst = max(float(np.linalg.norm((np.asarray(L[k]).astype(dt) - X[k]).astype(np.float64)) / np.linalg.norm(X[k].astype(np.float64))) for k in loam_ref.BLOCKS)
    e = float(abs(dt.type(L["error"]) - X["error"]) / X["error"]) if X["error"] != 0 else float(abs(L["error"]))
    return worst, e


# ---- near-degenerate neighbours -------------------------------------------------------------------------------------------------------------------------------------
CLUSTERS = 257  # a workgroup plus one lane
SPACING = 5.0
GRID = 2.0**-10
LENGTHS = [1.0, 1e-2, 1e-4]
SINES = [1e-1, 1e-2, 1e-3, 1e-4, 1e-5]
FAR = 10000.0


def _snap(a):
    return np.rint(np.asarray(a) / GRID) * GRID


def cluster_scene(K, value, far, seed=77):
    """-> (target f32 (257 (K + 1), 3), source f32 (257, 3), delta): K = 2 with |x_j - x_l| = value, K = 3 with the sine between x_j - x_l and x_j - x_m = value;
    far: the target translated by 10 km along fd.DIRECTION.  delta = [translation] expmap(fd.SMALL); the source is delta^-1 applied to the points beside the
    clusters, rounded to f32 (it need not be anywhere exactly)."""
    rng = np.random.default_rng(seed + 1000 * K)
    n = CLUSTERS
    base = np.stack([SPACING * np.arange(n), _snap(rng.uniform(-0.3, 0.3, n)), _snap(rng.uniform(-0.3, 0.3, n))], 1)  # x_j, on the grid
    phi = rng.uniform(0.0, 2.0 * np.pi, n)
    ex = np.broadcast_to([1.0, 0.0, 0.0], (n, 3))
    if K == 2:
        e1 = np.stack([np.zeros(n), np.cos(phi), np.sin(phi)], 1)  # the edge direction, in the y-z plane: a length of 1e-4 m is resolved at the origin
        xl = base + value * e1
        u = np.cross(e1, ex)
        third = base + 0.5 * value * e1 - 1.5 * ex + 0.3 * u  # further from the source point than x_l, whichever side it stands on
        pts = [base, xl, third]
        frac, arm = rng.uniform(0.3, 0.42, n), value * e1
    else:
        e1 = rng.normal(size=(n, 3))
        e1[:, 0] = np.abs(e1[:, 0]) + 0.5  # never in the y-z plane: the normal a x w has every component
        a = 2.0 * _snap(0.15 * e1 / np.linalg.norm(e1, axis=1)[:, None])  # x_l - x_j, 0.3 m, on a grid that holds 1.5 a exactly
        w = np.cross(a, ex)
        w /= np.linalg.norm(w, axis=1)[:, None]  # perpendicular to a, in the y-z plane
        la = np.linalg.norm(a, axis=1)[:, None]
        xm = base + 1.5 * a + (value / np.sqrt(1.0 - value * value)) * 1.5 * la * w  # the sine between a and x_m - x_j is `value`
        fourth = base - 2.5 * a
        pts = [base, base + a, xm, fourth]
        u = np.cross(a, w) / la
        frac, arm = rng.uniform(0.05, 0.12, n), a
    lateral = rng.uniform(0.15, 0.25, n)[:, None] * (u * np.cos(phi)[:, None] + (ex if K == 2 else w) * np.sin(phi)[:, None])
    beside = base + frac[:, None] * arm + lateral
    order = rng.permutation(n * (K + 1))  # (a cluster's points are not consecutive in the cloud)
    target = np.stack(pts, 1).reshape(-1, 3)[order]
    shift = FAR * fd.DIRECTION if far else np.zeros(3)
    delta = fd.expmap(fd.SMALL)
    delta[:3, 3] += shift
    target = (target + shift).astype(np.float32)
    world = beside + shift
    source = ((world - delta[:3, 3]) @ delta[:3, :3]).astype(np.float32)
    return target, source, delta


def realised(part, delta):
    """what the f32 inputs realise, over the points that get a correspondence: (smallest, largest) |x_j - x_l| and, for K = 3, sine"""
    m = part.margins(delta)
    out = {"length": (float(m["length"].min()), float(m["length"].max()))} if len(m["length"]) else {"length": (np.inf, 0.0)}
    if part.K == 3 and len(m["sine"]):
        with np.errstate(invalid="ignore"):
            out["sine"] = (float(np.nanmin(m["sine"])), float(np.nanmax(m["sine"])))
    return out


def cluster_figure(K, value, far):
    """one prescribed case measured on the CPU -> dict(ok: the input condition holds on the realised values and every cluster has its correspondence, margins,
    realised, worst / error: the f64 cross-product reference against the long-double M-form) -- what decides whether the case is in CLUSTER_CASES"""
    target, source, delta = cluster_scene(K, value, far)
    ref = loam_ref.PartRef(K, target, source, 1.0)
    ref.update_correspondences(delta)
    m = ref.margins(delta)
    with np.errstate(invalid="ignore"):
        low = {k: (float(np.nan_to_num(v, nan=0.0).min()) if len(v) else 0.0) for k, v in m.items()}
    ok = low["tie"] > MARGIN and low["cut"] > MARGIN and low["length"] > MARGIN and low.get("sine", 1.0) > SINE and len(m["length"]) == CLUSTERS
    out = dict(ok=bool(ok), margins=low, realised=realised(ref, delta), worst=np.inf, error=np.inf)
    if ok:
        out["worst"], out["error"] = agreement(ref.evaluate(delta), mform(ref, delta))
    return out


# The prescribed cases that stay (K, value, far), by the rule of section 3: the input condition holds on the REALISED values and the f64 cross-product reference is
# within 1e-8 of the long-double M-form.  tests/test_loam_domain_ref_cpu.py::test_cluster_case_list recomputes the rule for every prescribed case and holds this
# list to it; the measured figures stand in its docstring.
CLUSTER_CASES = [
    (2, 1.0, False), (2, 1e-2, False), (2, 1e-4, False),
    (3, 1e-1, False), (3, 1e-2, False), (3, 1e-3, False), (3, 1e-4, False), (3, 1e-5, False),
    (2, 1.0, True), (2, 1e-2, True),
    (3, 1e-1, True), (3, 1e-2, True), (3, 1e-3, True),
]

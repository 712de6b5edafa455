"""The per-point check of estimate_normals, built on tests/knn_ref.py (imported, not edited).  A helper, not a test.

The reference (features/normal_estimation.cpp:18-62): n_i = the eigenvector of the smallest eigenvalue of the covariance of point i, turned round when
p_i . n_i > 1.  With the default regularisation the covariance is I - 0.999 v v^T, v the eigenvector of the smallest eigenvalue of the sample covariance, so
the normal IS +-v (knn_ref.classify's V[:, :, 0]).

Direction.  ||(I - 0.999 v v^T) - (I - 0.999 w w^T)||_F = 0.999 sqrt(2) sin(angle(v, w)) for unit v, w, and ||I - 0.999 v v^T||_F = sqrt(2) to 3e-4: the
per-point rule on the covariance, rel. Frobenius error <= knn_ref.covariance_bound(relgap), IS

    sin(angle(got, +-v)) <= knn_ref.covariance_bound(relgap) / (0.999 sqrt(2))

on the normal.  Derived, not measured: a device normal may be exactly as wrong as the device covariance is already allowed to be.  The bound's first term
(1.5e-7 / (0.999 sqrt 2) = 1.08e-7) also covers the f32 store of a unit vector (worst case sqrt(3) 2^-25 = 5.2e-8).
Unit length.  | ||got|| - 1 | <= 2e-7 (three f32 roundings).
Sign.  s = p . v in f64, m = ||p|| x bound.  Where |s| > 1 + m the rule decides: p . got < 0 (s > 1: turned round, p . got = -s; s < -1: kept).  Within
|s| <= 1 + m either sign passes: inside |s| <= 1 the reference's sign is whatever its cross products give, and within m of the threshold the allowed error of
the direction decides.  The share of a cloud inside the band is printed; it is information, not a condition.
Exemptions: knn_ref's, with its cap (EXEMPT_CAP of the cloud; beyond it the helper fails).  A tie at rank k must match the normal of one of the candidate
neighbour sets; below relgap 1e-6 the normal must be unit and lie in the plane of the two smallest eigenvectors to 1e-6 when the third is separated.
Fewer than k neighbours, or a non-finite point: the covariance is the identity, computeDirect returns the identity basis, so got == (+-1, 0, 0) exactly; for a
finite point the sign follows the rule on p.x; for a non-finite one either passes.

From given covariances (assert_normals_from_covs): the reference is numpy.linalg.eigh of THE SAME f32 covariances the device was given, widened to f64 (lower
triangle, as computeDirect reads it).  The spectral gap is 0.999, so the bound is the first term alone; a reference built from f64 covariances would charge
the device for the caller's rounding (up to 9e-8 / 0.999).
"""
import numpy as np

import knn_ref

SCALE = 0.999 * np.sqrt(2.0)
UNIT_TOL = 2e-7
PLANE_TOL = 1e-6


def direction_bound(relgap):
    return knn_ref.covariance_bound(relgap) / SCALE


def sin_angle(a, b):
    """sine of the angle between the lines of a and b (rows), sign aside"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    c = np.cross(a, b)
    return np.linalg.norm(c, axis=-1) / np.maximum(np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1), 1e-300)


def reference_normals(points_f32, covs):
    """the numpy restatement: covs (N,3,3) f64 as matrices -> (N,3) f64 normals by eigh + the sign rule (normal_estimation.cpp:18-50)"""
    p = knn_ref._f64(points_f32)
    _, V = np.linalg.eigh(np.asarray(covs, dtype=np.float64).reshape(-1, 3, 3))
    n = V[:, :, 0].copy()
    with np.errstate(invalid="ignore"):
        flip = np.einsum("ni,ni->n", p, n) > 1.0
    n[flip] *= -1.0
    return n


def _identity_rule(p, got, rows, problems, label):
    """rows whose covariance is the identity: (+-1, 0, 0) exactly; the sign by p.x where the point is finite"""
    for r in rows:
        g = got[r]
        ok = g[1] == 0.0 and g[2] == 0.0 and abs(g[0]) == 1.0
        if ok and np.isfinite(p[r]).all():
            ok = g[0] == (-1.0 if p[r, 0] > 1.0 else 1.0)
        if not ok:
            problems.append(f"  {label(r)}: identity covariance but normal {g.tolist()} (p = {p[r].tolist()})")


def _sign_rule(p, v, got, bound, rows, problems, label):
    """rows (boolean): where |p . v| > 1 + ||p|| bound the normal points to the sensor's side of the tangent plane; -> boolean array, inside the band"""
    with np.errstate(invalid="ignore"):  # (non-finite points are not among `rows`)
        s = np.einsum("ni,ni->n", p, v)
        m = np.linalg.norm(p, axis=1) * bound
        decided = rows & (np.abs(s) > 1.0 + m)
        bad = decided & ~(np.einsum("ni,ni->n", p, got) < 0.0)
    for r in np.flatnonzero(bad)[:12]:
        problems.append(f"  {label(r)}: p . v = {s[r]:.9g} (band {1.0 + m[r]:.9g}) but p . got = {float(p[r] @ got[r]):.9g}")
    if bad.sum() > 12:
        problems.append(f"  ... and {int(bad.sum()) - 12} more (sign)")
    return rows & ~decided


def assert_normals(points_f32, k, got, *, what, subset=None, cls=None, cap_is_condition=True, quiet=False):
    """`got`: (N,3) (or (len(subset),3)) normals as estimate_normals(points, n, k) wrote them.  Every point is held to the rules of the module header; returns
    the figures (worst sin / bound, band share, exempt share) and prints them in one line.  cap_is_condition=False: as knn_ref.assert_covariances."""
    p32 = np.asarray(points_f32, dtype=np.float32).reshape(-1, 3)
    pall = knn_ref._f64(p32)
    cls = knn_ref.classify(p32, k, subset) if cls is None else cls
    sel = cls["sel"]
    p = pall[sel]
    got = np.asarray(got, dtype=np.float64).reshape(-1, 3)
    assert len(got) == len(sel), f"{what}: {len(got)} normals for {len(sel)} points"
    problems = []
    label = lambda r: f"point {sel[r]}"
    short = cls["short"]
    finite = np.isfinite(got).all(1)
    for r in np.flatnonzero(~finite)[:12]:
        problems.append(f"  {label(r)}: not finite")
    _identity_rule(p, got, np.flatnonzero(short & finite), problems, label)
    normal = finite & ~short
    norm = np.linalg.norm(np.where(finite[:, None], got, 0.0), axis=1)
    bad_unit = normal & (np.abs(norm - 1.0) > UNIT_TOL)
    for r in np.flatnonzero(bad_unit)[:12]:
        problems.append(f"  {label(r)}: length {norm[r]:.9g}")
    v = cls["V"][:, :, 0]
    bound = direction_bound(cls["relgap"])
    exempt = (cls["tie"] | (cls["relgap"] < knn_ref.RELGAP_EXEMPT)) & ~short
    checked = normal & ~exempt
    sin = sin_angle(np.where(finite[:, None], got, 0.0), v)
    ratio = np.where(checked, sin / bound, 0.0)
    over = np.flatnonzero(checked & (sin > bound))
    for r in over[np.argsort(-ratio[over])][:12]:
        problems.append(f"  {label(r)}: beyond the per-point bound: sin {sin[r]:.3e} relgap {cls['relgap'][r]:.3e} bound {bound[r]:.3e} got {got[r].tolist()} v {v[r].tolist()}")
    if len(over) > 12:
        problems.append(f"  ... and {len(over) - 12} more (beyond the per-point bound)")
    in_band = _sign_rule(p, v, got, np.where(np.isfinite(bound), bound, 0.0), checked, problems, label)
    for r in np.flatnonzero(exempt & finite):
        if cls["tie"][r]:
            idx = cls["idx"][r]
            inside = [j for j in range(k) if cls["in_grp"][r, j]]
            outside = [j for j in range(k, len(idx)) if cls["out_grp"][r, j]]
            sets = [list(idx[:k])]
            for a in inside:
                for b in outside:
                    s_ = list(idx[:k])
                    s_[a] = idx[b]
                    sets.append(s_)
            Vc = knn_ref.reference_covariance(pall[np.array(sets)])[2][:, :, 0]
            ok = False
            for c in Vc:
                if sin_angle(got[r], c) <= bound[r]:
                    sc, mc = float(p[r] @ c), float(np.linalg.norm(p[r]) * bound[r])
                    ok = ok or abs(sc) <= 1.0 + mc or float(p[r] @ got[r]) < 0.0
            if not ok:
                problems.append(f"  {label(r)}: tie: matches the normal of none of the {len(sets)} candidate neighbour sets")
        elif cls["topgap"][r] >= 1e-3:
            out_of_plane = abs(float(got[r] @ cls["V"][r][:, 2]))
            if out_of_plane > PLANE_TOL:
                problems.append(f"  {label(r)}: degenerate pair: the normal leaves the plane of the two smallest eigenvectors by {out_of_plane:.2e}")
    share = exempt.sum() / max(len(sel), 1)
    if cap_is_condition and exempt.sum() > knn_ref.EXEMPT_CAP * len(sel):
        problems.append(f"  exempt share {exempt.sum()} of {len(sel)} = {share:.4%} is above the cap of {knn_ref.EXEMPT_CAP:.1%}: the wrong cloud for this helper")
    figs = dict(what=what, k=k, n=len(sel), exempt=int(exempt.sum()), ties=int(cls["tie"].sum()), short=int(short.sum()),
                worst_ratio=float(ratio.max()) if checked.any() else 0.0, worst_sin=float(sin[checked].max()) if checked.any() else 0.0,
                band_share=float(in_band.sum() / max(int(checked.sum()), 1)))
    if not quiet:
        print(f"[normals_ref] {what}: k={k} n={figs['n']} exempt={figs['exempt']} ({share:.4%}; ties {figs['ties']}) short={figs['short']} "
              f"worst sin/bound={figs['worst_ratio']:.3e} worst sin={figs['worst_sin']:.3e} sign band (either sign passes): {figs['band_share']:.2%}")
    assert not problems, f"{what} (k = {k}): {len(problems)} report lines\n" + "\n".join(problems)
    return figs


def stored_covs_as_matrices(covs_f32):
    """float [N][9] column-major (the device layout) -> (N,3,3) f64 matrices C[i][r][c]"""
    return np.asarray(covs_f32, dtype=np.float32).reshape(-1, 3, 3).astype(np.float64).transpose(0, 2, 1)


def assert_normals_from_covs(points_f32, covs_f32, got, *, what="from covariances", quiet=False):
    """`covs_f32`: float [N][9] exactly as the device was given them (column-major); `got`: (N,3) normals of estimate_normals(points, covs, n)"""
    p = knn_ref._f64(points_f32)
    C = stored_covs_as_matrices(covs_f32)
    got = np.asarray(got, dtype=np.float64).reshape(-1, 3)
    assert len(got) == len(p) == len(C), f"{what}: {len(got)} normals, {len(p)} points, {len(C)} covariances"
    problems = []
    label = lambda r: f"point {r}"
    finite = np.isfinite(got).all(1)
    for r in np.flatnonzero(~finite)[:12]:
        problems.append(f"  {label(r)}: not finite")
    low = np.tril(C)
    identity = (low == np.eye(3)).all((1, 2))  # (the lower triangle is all the solver reads)
    _identity_rule(p, got, np.flatnonzero(identity & finite), problems, label)
    rows = finite & ~identity
    w, V = np.linalg.eigh(C)  # UPLO = 'L'
    v = V[:, :, 0]
    norm = np.linalg.norm(np.where(finite[:, None], got, 0.0), axis=1)
    for r in np.flatnonzero(rows & (np.abs(norm - 1.0) > UNIT_TOL))[:12]:
        problems.append(f"  {label(r)}: length {norm[r]:.9g}")
    bound = np.full(len(p), knn_ref.TAU_OUT / SCALE)
    sin = sin_angle(np.where(finite[:, None], got, 0.0), v)
    over = np.flatnonzero(rows & (sin > bound))
    for r in over[np.argsort(-sin[over])][:12]:
        problems.append(f"  {label(r)}: beyond the bound: sin {sin[r]:.3e} bound {bound[r]:.3e} eigenvalues {w[r].tolist()} got {got[r].tolist()} v {v[r].tolist()}")
    if len(over) > 12:
        problems.append(f"  ... and {len(over) - 12} more (beyond the bound)")
    in_band = _sign_rule(p, v, got, bound, rows, problems, label)
    figs = dict(what=what, n=len(p), identity=int(identity.sum()), worst_sin=float(sin[rows].max()) if rows.any() else 0.0,
                band_share=float(in_band.sum() / max(int(rows.sum()), 1)))
    if not quiet:
        print(f"[normals_ref] {what}: n={figs['n']} identity={figs['identity']} worst sin={figs['worst_sin']:.3e} (bound {bound[0]:.3e}) "
              f"sign band (either sign passes): {figs['band_share']:.2%}")
    assert not problems, f"{what}: {len(problems)} report lines\n" + "\n".join(problems)
    return figs

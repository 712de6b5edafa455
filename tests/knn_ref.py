"""A plain reference for the k-NN search and for estimate_covariances, and the per-point check built on it.

No GPU and no oracle here: scipy's cKDTree finds candidate neighbours, every squared distance is recomputed in f64 from the f64 values of the f32
coordinates, the sample covariance is the centred f64 one, and the eigenvectors come from numpy.linalg.eigh.  The output of estimate_covariances
(features/covariance_estimation.cpp:18-77) is V diag(1e-3, 1, 1) V^-1 = I - 0.999 v v^T with v the eigenvector of the smallest eigenvalue.

How well that output is determined is decided by  relgap = (l2 - l1) / l3  of the sample covariance (l1 <= l2 <= l3): the eigenvector v turns by
(error of the covariance) / (l2 - l1).  The per-point tolerance on the relative Frobenius error is therefore

    covariance_bound(relgap) = TAU_OUT + ETA / relgap

  TAU_OUT = 4 x 3.81e-8.  3.81e-8 is the worst relative Frobenius distance between the oracle's f64 covariances and their f32 roundings over the clouds
            of tests/test_knn_ref_cpu.py (the output is stored as f32); the factor 4 leaves room for the three f64 products behind every entry.
  ETA     = 100 x 5.6e-9.  5.6e-9 is the worst  rel x relgap  of the ORACLE (the closed-form solver of the reference, restated in C) against this
            module over the same clouds -- on the cloud with duplicated points; <= 5e-12 on every other one.  The factor for the device's different f64
            contraction (fused multiply-adds) and summation order is 100, the largest the issue behind this module allows: the measured figure has a heavy
            tail (three orders of magnitude between one cloud and the next: it is the worst case of the closed form's trigonometric root finder near a
            double root), and another rounding of the same arithmetic draws another sample from that tail.  It is still four orders of magnitude below what
            a lost neighbour costs (rel x relgap ~ 1e-2).
  Neither number comes from the kernels.  tests/test_knn_ref_cpu.py measures both again in every CPU run and fails if the oracle exceeds the bases.
  Measured on the MI355X (tests/test_knn_edges_gpu.py prints them per structure and per k; GPU_FIGURES there): worst rel x relgap 3.2e-8 on every cloud,
  structure and k -- the oracle's own figure once its output is rounded to f32, to the digits shown.

Exempt from the bound are (i) near-ties at rank k BETWEEN DIFFERENT COORDINATES: d2[k+1] - d2[k] <= 1e-6 d2[k+1] (ranks from 1) where exchanging the tied
points changes the set of coordinates -- a tie between copies of one coordinate does not change the covariance and is no tie here; the output must then
match the reference built from one of the candidate sets; and (ii) relgap < 1e-6, where v is arbitrary within the plane of the two smallest eigenvectors:
it must lie in that plane to 1e-6 when the third eigenvalue is separated ((l3 - l2) / l3 >= 1e-3).  At most 0.1 % of a cloud may be exempt; a cloud with
more is the wrong cloud for assert_covariances, which fails on it.
"""
import numpy as np

TAU_OUT_BASE = 3.81e-8
TAU_OUT = 4.0 * TAU_OUT_BASE
ETA_BASE = 5.6e-9
ETA_FACTOR = 100.0
ETA = ETA_FACTOR * ETA_BASE
TIE_REL = 1e-6
RELGAP_EXEMPT = 1e-6
EXEMPT_CAP = 1e-3
EIGENVALUE_TOL = 1e-5
WORKERS = 16
_EXTRA = 4  # candidates past rank k + 1: the tree selects by ITS rounding of the distance; the recomputed d2 re-sorts them, and ties are seen as groups
_LAMBDA = np.array([1e-3, 1.0, 1.0])


def _f64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1, 3), dtype=np.float64)


def _candidates(points_f32, queries_f32, m):
    """the m nearest finite points of every query: (d2 (Q,m) ascending, ties by index; idx (Q,m) into `points_f32`).  Missing ones: d2 = inf, idx = -1
    (fewer than m finite points; a query that is not finite has none)."""
    from scipy.spatial import cKDTree

    p, q = _f64(points_f32), _f64(queries_f32)
    keep = np.flatnonzero(np.isfinite(p).all(1))
    qok = np.isfinite(q).all(1)
    d2 = np.full((len(q), m), np.inf)
    idx = np.full((len(q), m), -1, dtype=np.int64)
    mm = min(m + _EXTRA, len(keep))
    if mm == 0 or not qok.any():
        return d2, idx
    pk = p[keep]
    _, cand = cKDTree(pk).query(q[qok], k=mm, workers=WORKERS)
    cand = cand.reshape(-1, mm)
    diff = pk[cand] - q[qok][:, None, :]
    dd = diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1] + diff[..., 2] * diff[..., 2]
    gi = keep[cand]
    order = np.lexsort((gi, dd), axis=1)  # by recomputed d2, then by index
    dd, gi = np.take_along_axis(dd, order, 1), np.take_along_axis(gi, order, 1)
    w = min(m, mm)
    rows = np.flatnonzero(qok)
    d2[rows, :w] = dd[:, :w]
    idx[rows, :w] = gi[:, :w]
    return d2, idx


def neighbours(points_f32, queries_f32, k):
    """exact squared distances and indices of the k + 1 nearest points of every query -> (d2 (Q, k+1) f64 ascending, idx (Q, k+1) int64; inf / -1 where
    the cloud has fewer finite points, and for queries that are not finite)"""
    return _candidates(points_f32, queries_f32, k + 1)


def reference_covariance(nb):
    """nb (M,k,3) f64 neighbour coordinates -> (C (M,3,3), w (M,3) ascending eigenvalues of the sample covariance, V (M,3,3) its eigenvectors in columns)"""
    c = nb - nb.mean(1, keepdims=True)
    cov = np.einsum("nki,nkj->nij", c, c) / nb.shape[1]
    w, V = np.linalg.eigh(cov)
    v = V[:, :, 0]
    C = np.eye(3)[None] - 0.999 * v[:, :, None] * v[:, None, :]
    return C, w, V


def classify(points_f32, k, subset=None):
    """per point (or per point of `subset`, indices into the cloud): dict with
    tie (bool), relgap, C (reference output), w, V (sample covariance eigen-decomposition), d2 / idx (the k + 1 + _EXTRA nearest, the point itself included),
    short (fewer than k finite neighbours: the reference writes the identity)"""
    p32 = np.asarray(points_f32, dtype=np.float32).reshape(-1, 3)
    p = _f64(p32)
    sel = np.arange(len(p)) if subset is None else np.asarray(subset, dtype=np.int64)
    m = k + 1 + _EXTRA
    d2, idx = _candidates(p32, p32[sel], m)
    short = ~np.isfinite(d2[:, k - 1])
    safe = np.where(idx >= 0, idx, 0)
    nb = p[safe[:, :k]]
    nb[short] = 0.0
    C, w, V = reference_covariance(nb)
    with np.errstate(divide="ignore", invalid="ignore"):
        relgap = np.where(w[:, 2] > 0.0, (w[:, 1] - w[:, 0]) / w[:, 2], 0.0)
        topgap = np.where(w[:, 2] > 0.0, (w[:, 2] - w[:, 1]) / w[:, 2], 0.0)
    # near-tie at rank k: the group of candidates within TIE_REL of the boundary on either side; a tie iff the group reaches past rank k and does not consist
    # of copies of one coordinate
    lo, hi = d2[:, k - 1:k], d2[:, k:k + 1]
    with np.errstate(invalid="ignore"):
        out_grp = np.isfinite(d2) & ((d2 - lo) <= TIE_REL * d2)
        in_grp = np.isfinite(d2) & np.isfinite(hi) & ((hi - d2) <= TIE_REL * hi)
    ranks = np.arange(m)[None]
    out_grp &= ranks >= k
    in_grp &= ranks < k
    grp = out_grp | in_grp
    differs = (p32[safe] != p32[safe[:, k - 1]][:, None, :]).any(2)
    tie = out_grp.any(1) & (grp & differs).any(1) & ~short
    C[short] = np.eye(3)
    return dict(sel=sel, tie=tie, relgap=relgap, topgap=topgap, C=C, w=w, V=V, d2=d2, idx=idx, short=short, in_grp=in_grp, out_grp=out_grp)


def covariance_bound(relgap):
    with np.errstate(divide="ignore"):
        return TAU_OUT + ETA / np.asarray(relgap, dtype=np.float64)


def rel_frobenius(got, ref):
    got, ref = np.asarray(got, dtype=np.float64).reshape(-1, 9), np.asarray(ref, dtype=np.float64).reshape(-1, 9)
    return np.linalg.norm(got - ref, axis=1) / np.linalg.norm(ref, axis=1)


def _tie_candidates(cls, row, p, k):
    """the reference outputs of the neighbour sets a tie allows: the first k, and every exchange of one tied member inside for one tied candidate outside"""
    idx = cls["idx"][row]
    inside = [j for j in range(k) if cls["in_grp"][row, j]]
    outside = [j for j in range(k, len(idx)) if cls["out_grp"][row, j]]
    sets = [list(idx[:k])]
    for a in inside:
        for b in outside:
            s = list(idx[:k])
            s[a] = idx[b]
            sets.append(s)
    return reference_covariance(p[np.array(sets)])[0]


def assert_covariances(points_f32, k, got, *, what, subset=None, quiet=False, cls=None, cap_is_condition=True):
    """`got`: (N,3,3) (or (len(subset),3,3)) covariances as estimate_covariances wrote them, got[i] = C_i as a matrix.  Every point is held to the rule in the
    module header; returns the figures (worst rel, worst rel x relgap over the non-exempt points, exempt share) and prints them in one line.
    cap_is_condition=False: for a cloud that the reference alone shows to be beyond the exempt cap (tests/test_knn_ref_cpu.py names them): the share is printed,
    every non-exempt point is held to the bound and every exempt one to its own rule, as always."""
    p32 = np.asarray(points_f32, dtype=np.float32).reshape(-1, 3)
    p = _f64(p32)
    cls = classify(p32, k, subset) if cls is None else cls  # (cls: classify(points, k, subset) of the same arguments, kept by a caller that checks many outputs)
    sel = cls["sel"]
    got = np.asarray(got, dtype=np.float64).reshape(-1, 3, 3)
    assert len(got) == len(sel), f"{what}: {len(got)} covariances for {len(sel)} points"
    problems = []

    def report(rows, why):
        for r in rows[:12]:
            nbd = ", ".join(f"{x:.9g}" for x in cls["d2"][r, :k + 2])
            problems.append(f"  point {sel[r]}: {why}: rel {rel[r]:.3e} relgap {cls['relgap'][r]:.3e} bound {bound[r]:.3e} tie {bool(cls['tie'][r])} eig {np.array2string(ev[r], precision=7)}\n"
                            f"    reference d2 of ranks 1..{k + 2}: [{nbd}]  indices {cls['idx'][r, :k + 2].tolist()}")
        if len(rows) > 12:
            problems.append(f"  ... and {len(rows) - 12} more ({why})")

    finite = np.isfinite(got).all((1, 2))
    rel = rel_frobenius(np.where(finite[:, None, None], got, 0.0), cls["C"])
    bound = covariance_bound(cls["relgap"])
    evc = np.linalg.eigvals(np.where(finite[:, None, None], got, np.eye(3)))
    ev = np.sort(evc.real, axis=1)
    report(np.flatnonzero(~finite), "not finite")
    # eigenvalues (general: the output is V L V^-1 and need not be symmetric); the identity of a point with fewer than k neighbours is compared as it is
    normal = finite & ~cls["short"]
    bad_ev = normal & ((np.abs(ev - _LAMBDA).max(1) > EIGENVALUE_TOL) | (np.abs(evc.imag).max(1) > EIGENVALUE_TOL))
    report(np.flatnonzero(bad_ev), "eigenvalues not (1e-3, 1, 1) to 1e-5")
    bad_short = finite & cls["short"] & (got != np.eye(3)).any((1, 2))
    report(np.flatnonzero(bad_short), "fewer than k neighbours but not the identity")
    exempt = (cls["tie"] | (cls["relgap"] < RELGAP_EXEMPT)) & ~cls["short"]
    checked = normal & ~exempt
    order = np.argsort(-(rel / bound))
    report([r for r in order if checked[r] and rel[r] > bound[r]], "beyond the per-point bound")
    for r in np.flatnonzero(exempt & finite):
        if cls["tie"][r]:
            cands = _tie_candidates(cls, r, p, k)
            if not (rel_frobenius(np.repeat(got[r][None], len(cands), 0), cands) <= bound[r]).any():
                report([r], f"tie: matches none of the {len(cands)} candidate neighbour sets")
        elif cls["topgap"][r] >= 1e-3:
            ws, vs = np.linalg.eigh(0.5 * (got[r] + got[r].T))
            out_of_plane = abs(vs[:, 0] @ cls["V"][r][:, 2])
            if out_of_plane > 1e-6:
                report([r], f"degenerate pair: small eigenvector leaves the plane of the two smallest by {out_of_plane:.2e}")
    share = exempt.sum() / max(len(sel), 1)
    cap_ok = exempt.sum() <= EXEMPT_CAP * len(sel) or not cap_is_condition
    if not cap_ok:
        problems.append(f"  exempt share {exempt.sum()} of {len(sel)} = {share:.4%} is above the cap of {EXEMPT_CAP:.1%}: the wrong cloud for this helper")
    figs = dict(what=what, k=k, n=len(sel), exempt=int(exempt.sum()), ties=int(cls["tie"].sum()), short=int(cls["short"].sum()),
                worst_rel=float(rel[checked].max()) if checked.any() else 0.0,
                worst_rel_x_relgap=float((rel[checked] * cls["relgap"][checked]).max()) if checked.any() else 0.0)
    if not quiet:
        print(f"[knn_ref] {what}: k={k} n={figs['n']} exempt={figs['exempt']} ({share:.4%}; ties {figs['ties']}) short={figs['short']} "
              f"worst rel={figs['worst_rel']:.3e} worst rel*relgap={figs['worst_rel_x_relgap']:.3e}")
    assert not problems, f"{what} (k = {k}): {len(problems)} report lines\n" + "\n".join(problems)
    return figs


# ---- the seeded synthetic clouds the k-NN tests share (built exactly as tests/test_knn_gicp_gpu.py builds them) --------------------------------------
def sparse_slab_cloud():
    rng = np.random.default_rng(17)
    sparse = rng.uniform(-40.0, 40.0, size=(30_000, 3)).astype(np.float32)
    sparse[:, 2] *= 0.1
    outliers = np.array([[300.0, 0.0, 0.0], [0.0, -250.0, 3.0], [305.0, 1.0, 0.5]], np.float32)
    return np.concatenate([sparse, outliers])


def duplicates_cloud():
    rng = np.random.default_rng(23)
    base = rng.uniform(-30.0, 30.0, size=(4000, 3)).astype(np.float32)
    base[:, 2] *= 0.05
    dup = np.repeat(base[:1500], 3, axis=0)
    blobs = []
    for c in rng.uniform(-200.0, 200.0, size=(12, 3)).astype(np.float32):
        m = int(rng.integers(4, 41))
        blobs.append(c + rng.normal(0.0, 0.05, size=(m, 3)).astype(np.float32))
    cloud = np.concatenate([base, dup] + blobs).astype(np.float32)
    return cloud[rng.permutation(len(cloud))]


def wall_and_gap_cloud():
    rng = np.random.default_rng(29)
    parts = []
    for i, gap in enumerate([13.0, 18.0, 22.0, 27.0, 33.0, 38.0, 70.0]):
        origin = np.array([400.0 * i, 0.0, 0.0])
        yz = rng.uniform(-6.0, 6.0, size=(1500, 2))
        wall = np.column_stack([np.full(len(yz), gap) + rng.normal(0.0, 0.02, len(yz)), yz])
        lonely = rng.normal(0.0, 0.3, size=(3, 3))
        near = lonely[:1] + rng.normal(0.0, 0.2, size=(4, 3)) + [0.0, 4.5, 0.0]
        parts += [origin + wall, origin + lonely, origin + near]
    cloud = np.concatenate(parts).astype(np.float32)
    return cloud[rng.permutation(len(cloud))]


def scan_cut(scan_f32, n, centre=60_000):
    """the n points of a scan nearest to one of its points: a cut that keeps the scan's local density (a prefix of the file would be one ring of the sensor)"""
    from scipy.spatial import cKDTree

    s = np.asarray(scan_f32, dtype=np.float32).reshape(-1, 3)
    _, idx = cKDTree(s.astype(np.float64)).query(s[centre].astype(np.float64), k=n)
    return s[np.sort(np.atleast_1d(idx))]


def assert_two_neighbour_covariances(points_f32, got, *, what):
    """k = 2: the sample covariance of a point and its nearest neighbour is rank one (relgap = 0 for EVERY point), so rule (ii) of the header is all there is:
    eigenvalues (1e-3, 1, 1) to 1e-5 and the small eigenvector orthogonal, to 1e-6, to the direction to the neighbour -- the only direction the neighbourhood
    has.  Which vector of that plane comes out is decided by the rounding noise of the uncentred sums (the closed form reads the kernel of a matrix that is
    rank one plus that noise): two correct implementations agree only as far as their roundings do, and a comparison with the oracle is a figure, not a check."""
    p32 = np.asarray(points_f32, dtype=np.float32).reshape(-1, 3)
    got = np.asarray(got, dtype=np.float64).reshape(-1, 3, 3)
    assert np.isfinite(got).all(), what
    d2, idx = neighbours(p32, p32, 2)
    assert (d2[:, 1] > 0.0).all(), f"{what}: a cloud with copies of a coordinate has rank-zero neighbourhoods at k = 2"
    seg = p32[idx[:, 1]].astype(np.float64) - p32[idx[:, 0]].astype(np.float64)
    seg /= np.linalg.norm(seg, axis=1, keepdims=True)
    ev = np.sort(np.linalg.eigvals(got).real, axis=1)
    bad = np.flatnonzero(np.abs(ev - _LAMBDA).max(1) > EIGENVALUE_TOL)
    assert len(bad) == 0, f"{what}: eigenvalues of points {bad[:10].tolist()}: {ev[bad[:3]].tolist()}"
    _, vs = np.linalg.eigh(0.5 * (got + got.transpose(0, 2, 1)))
    off = np.abs(np.einsum("ni,ni->n", vs[:, :, 0], seg))
    bad = np.flatnonzero(off > 1e-6)
    assert len(bad) == 0, f"{what}: the small eigenvector of points {bad[:10].tolist()} leaves the plane across the neighbour by {off[bad[:10]].tolist()}"

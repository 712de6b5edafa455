"""f64 numpy restatement of estimate_fpfh (src/gtsam_points/features/fpfh_estimation.cpp:58-93 compute_pair_features, :196-307 estimate_fpfh) for the FPFH tests,
with the clouds those tests share.  Not a test module.

The search is brute force: j is a neighbour of i when d2 = (dx dx + dy dy) + dz dz < r * r, strictly (ann/small_kdtree.hpp:492), j = i included; points with a
non-finite coordinate are nobody's neighbours and have zero rows.  The neighbours are taken in the DEVICE's walk order (include/gtsam_points_hip.h): cell coordinate
floor(coord / r) in f64 clamped to +-(2^20 - 3), the 27 cells around the query in ascending (dz, dy, dx), dx fastest, ascending index inside a cell, at most
max_num_neighbors of them.  Without a binding cap the order decides nothing but the order of the FPFH sum.

SETTLED.  An integer histogram can be compared exactly only where no decision in it hangs on the last bits.  A pair (k, j) is settled when
  - each of the three nf * 11 values is at least MARGIN = 1e-9 from an integer (a NaN value -- a neighbour's NaN normal -- is decided by rule, bin 0, not by rounding,
    and counts as settled),
  - where ||angle1| - |angle2|| < MARGIN, BOTH branches of the swap give the same three bins, each with that margin (a plane with equal normals ties exactly),
and a point is settled when all its pairs are and no candidate's d2 is within MARGIN (relative) of r * r.  An FPFH row is settled when the point and all its
neighbours are.

TOLERANCE of a settled FPFH row, entry-wise (fpfh_tolerance), in units of u = 2^-53.  Every term of an entry's sum is non-negative, so nothing cancels and every
error below is relative to the entry itself.  A term (count * hist_incr) * (1 / d2) carries about 3 roundings (d2 itself is computed alike on both sides); a sum of
n such terms adds at most n - 1 more, whatever its order: an entry is within about (n + 2) u of its exact value, at most 2 n u + 16 u say.  The normaliser
100 / (sum of the first 11 entries) inherits those entries' (2 n + 16) u and adds 10 roundings of its sum and one of its quotient, and the last product one more:
about (4 n + 44) u for one side, at most (4 n + 64) u.  Both sides err, the device and this restatement: (8 n + 128) u = (2 n + 32) 2^-52 <= (2 n + 64) 2^-52
relative to the entry -- the constant below, derived, not measured.  Zero entries are exactly zero on both sides (no term contributes)."""
import numpy as np

MARGIN = 1e-9
CELL_LIMIT = (1 << 20) - 3
FMIN = np.array([-np.pi, -1.0, -1.0])
INV_RANGE = 1.0 / (np.array([np.pi, 1.0, 1.0]) - FMIN)


def fpfh_tolerance(n):
    """relative entry-wise bound between two correct f64 evaluations of an FPFH row over n neighbours"""
    return (2.0 * n + 64.0) * 2.0 ** -52


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def pair_features_branch(p1, n1, p2, n2, swap):
    """compute_pair_features for M pairs (p2, n2: [M, 3]; p1, n1: [3]) with the swap decision given: (features [M, 3] = theta, phi, alpha; angle1, angle2)"""
    p2, n2 = np.atleast_2d(np.asarray(p2, np.float64)), np.atleast_2d(np.asarray(n2, np.float64))
    p1, n1 = np.asarray(p1, np.float64), np.broadcast_to(np.asarray(n1, np.float64), n2.shape)
    with np.errstate(all="ignore"):
        dp = p2 - p1
        d = np.sqrt(_dot(dp, dp))
        u = dp / d[:, None]
        a1, a2 = _dot(n1, u), _dot(n2, u)
        sw = np.asarray(swap, bool)[:, None]
        m, o, u = np.where(sw, n2, n1), np.where(sw, n1, n2), np.where(sw, -u, u)
        alpha = np.where(sw[:, 0], -a2, a1)
        v = _cross(u, m)
        v = v / np.sqrt(_dot(v, v))[:, None]
        w = _cross(m, v)
        f = np.stack([np.arctan2(_dot(w, o), _dot(m, o)), _dot(v, o), alpha], axis=-1)
    f[(d == 0.0) | ~np.isfinite(v).all(axis=1)] = 0.0  # :61-63, :84-86
    return f, a1, a2


def compute_pair_features(p1, n1, p2, n2):
    """the reference's function for one pair: (theta, phi, alpha)"""
    _, a1, a2 = pair_features_branch(p1, n1, p2, n2, [False])
    with np.errstate(invalid="ignore"):
        swap = np.abs(a1) < np.abs(a2)  # :76
    return pair_features_branch(p1, n1, p2, n2, swap)[0][0]


def bins_of(f):
    """(bins int [M, 3], margin [M, 3]: distance of nf * 11 from the nearest integer; inf for NaN, which the rule sends to bin 0)"""
    with np.errstate(invalid="ignore"):
        x = ((f - FMIN) * INV_RANGE) * 11.0
        nan = np.isnan(x)
        b = np.where(nan, 0, np.clip(np.floor(np.where(nan, 0.0, x)), 0, 10)).astype(np.int64)
        margin = np.where(nan, np.inf, np.abs(x - np.rint(x)))
    return b, margin


def cell_of(coord, r):
    return np.clip(np.floor(np.asarray(coord, np.float64) / r), -CELL_LIMIT, CELL_LIMIT).astype(np.int64)


class FpfhRef:
    pass


def estimate(points, normals, radius, max_num_neighbors=10000, tie_rule=True):
    """-> FpfhRef: hist int64 [N, 33], n int64 [N], settled bool [N], spfh / fpfh float64 [N, 33], row_settled bool [N], neighbors (list of index arrays in walk
    order), sq_dists, num_truncated, num_ties (pairs decided through the both-branches rule), min_bin_margin, min_swap_margin"""
    P, Nn = np.asarray(points, np.float32).astype(np.float64), np.asarray(normals, np.float32).astype(np.float64)
    N = P.shape[0]
    r = float(radius)
    r2 = r * r
    finite = np.isfinite(P).all(axis=1)
    with np.errstate(invalid="ignore"):
        cells = np.where(finite[:, None], cell_of(np.where(finite[:, None], P, 0.0), r), 0)
        D = P[:, None, :] - P[None, :, :]
        D2 = (D[..., 0] * D[..., 0] + D[..., 1] * D[..., 1]) + D[..., 2] * D[..., 2]
        inside = (D2 < r2) & finite[:, None] & finite[None, :]
        near_edge = (np.abs(D2 - r2) <= MARGIN * r2) & finite[:, None] & finite[None, :]
    out = FpfhRef()
    out.hist = np.zeros((N, 33), np.int64)
    out.n = np.zeros(N, np.int64)
    out.settled = np.ones(N, bool)
    out.neighbors, out.sq_dists = [], []
    out.num_ties, out.min_bin_margin, out.min_swap_margin = 0, np.inf, np.inf
    for k in range(N):
        js = np.nonzero(inside[k])[0]
        rel = cells[js] - cells[k] + 1  # each in 0 .. 2
        order = np.lexsort((js, rel[:, 0], rel[:, 1], rel[:, 2]))  # (dz, dy, dx) ascending, dx fastest, then the index
        js = js[order][: int(max_num_neighbors)]
        out.neighbors.append(js)
        out.sq_dists.append(D2[k, js])
        out.n[k] = len(js)
        if near_edge[k].any():
            out.settled[k] = False
        others = js[js != k]
        if len(js) <= 1 or len(others) == 0:
            continue
        f0, a1, a2 = pair_features_branch(P[k], Nn[k], P[others], Nn[others], np.zeros(len(others), bool))
        f1 = pair_features_branch(P[k], Nn[k], P[others], Nn[others], np.ones(len(others), bool))[0]
        with np.errstate(invalid="ignore"):
            swap = np.abs(a1) < np.abs(a2)
            gap = np.abs(np.abs(a1) - np.abs(a2))
            tie = gap < MARGIN
        b0, m0 = bins_of(f0)
        b1, m1 = bins_of(f1)
        b = np.where(swap[:, None], b1, b0)
        ok = np.where(swap[:, None], m1, m0).min(axis=1) >= MARGIN
        both = (b0 == b1).all(axis=1) & (np.minimum(m0, m1).min(axis=1) >= MARGIN)
        ok = np.where(tie, both if tie_rule else False, ok)
        out.num_ties += int(tie.sum())
        out.min_bin_margin = min(out.min_bin_margin, float(np.where(swap[:, None], m1, m0).min()))
        if (~tie & np.isfinite(gap)).any():
            out.min_swap_margin = min(out.min_swap_margin, float(gap[~tie & np.isfinite(gap)].min()))
        if not ok.all():
            out.settled[k] = False
        for c in range(3):
            out.hist[k, 11 * c : 11 * c + 11] = np.bincount(b[:, c], minlength=11)
    out.num_truncated = int((out.n == int(max_num_neighbors)).sum())
    out.spfh = np.zeros((N, 33))
    for k in range(N):
        if out.n[k] > 1:
            out.spfh[k] = out.hist[k].astype(np.float64) * (100.0 / float(out.n[k] - 1))  # :245-246
    out.fpfh = np.zeros((N, 33))
    out.row_settled = np.zeros(N, bool)
    for i in range(N):
        js, d2 = out.neighbors[i], out.sq_dists[i]
        out.row_settled[i] = bool(out.settled[i] and out.settled[js].all())
        if len(js) <= 1:
            continue
        acc = np.zeros(33)
        for j, q in zip(js, d2):
            if q == 0.0:
                continue
            acc = acc + out.spfh[j] * (1.0 / q)  # :263-268
        with np.errstate(all="ignore"):
            out.fpfh[i] = acc * (100.0 / acc[:11].sum())  # :271-275
    return out


# ---- the clouds of tests/test_fpfh_ref_cpu.py and tests/test_fpfh_gpu.py: name -> (points f32 [N, 3], normals f32 [N, 3], search_radius) ----------------------------


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def cloud(name):
    rng = np.random.default_rng(20240611)
    if name == "random600":  # uniform in a 4 m box, random unit normals: mean 17, at most ~32 neighbours at r = 0.8
        return rng.uniform(0.0, 4.0, (600, 3)).astype(np.float32), _unit(rng.normal(size=(600, 3))).astype(np.float32), 0.8
    if name == "plane400":  # |angle1| = |angle2| = 0 for every pair: settled only through the both-branches rule
        p = np.concatenate([rng.uniform(0.0, 2.0, (400, 2)), np.full((400, 1), 0.5)], axis=1).astype(np.float32)
        return p, np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (400, 1)), 0.3
    if name == "sphere400":  # radial normals: |angle1| and |angle2| agree to the rounding of the f32 points
        p = _unit(rng.normal(size=(400, 3))).astype(np.float32)
        return p, p.copy(), 0.4
    if name == "one":
        return np.array([[0.25, -0.5, 1.0]], np.float32), np.array([[0.0, 0.0, 1.0]], np.float32), 0.8
    if name == "two":
        return np.array([[0.25, -0.5, 1.0], [0.5, -0.25, 1.25]], np.float32), _unit(np.array([[0.1, 0.2, 1.0], [0.3, -0.2, 0.9]])).astype(np.float32), 0.8
    if name == "cell65":  # more than a wave of candidates in ONE cell
        return rng.uniform(0.05, 0.75, (65, 3)).astype(np.float32), _unit(rng.normal(size=(65, 3))).astype(np.float32), 0.8
    if name == "signed300":  # cells on both sides of zero, a NaN point and a NaN normal
        p = rng.uniform(-2.0, 2.0, (300, 3)).astype(np.float32)
        n = _unit(rng.normal(size=(300, 3))).astype(np.float32)
        p[7, 1] = np.nan
        n[11, 0] = np.nan
        return p, n, 0.8
    raise KeyError(name)


CLOUDS = ("random600", "plane400", "sphere400", "one", "two", "cell65", "signed300")
CAP = 8  # the binding cap of the tests (random600: most points have more neighbours)


def height_field():
    """(target points, target normals, source points, source normals, T_target_source, radius): a bumpy height field over a 20 x 20 grid at 0.25 m, z on a 2^-12 grid,
    analytic normals; the source is the target turned by 90 degrees about z and shifted by whole metres -- every coordinate stays exact in f32"""
    g = np.arange(20) * 0.25
    x, y = [a.ravel() for a in np.meshgrid(g, g, indexing="ij")]
    z = 0.30 * np.sin(1.3 * x + 0.2) + 0.25 * np.cos(0.9 * y - 0.4) + 0.12 * np.sin(2.1 * x + 0.7 * y) + 0.05 * x * y / 4.0
    zx = 0.30 * 1.3 * np.cos(1.3 * x + 0.2) + 0.12 * 2.1 * np.cos(2.1 * x + 0.7 * y) + 0.05 * y / 4.0
    zy = -0.25 * 0.9 * np.sin(0.9 * y - 0.4) + 0.12 * 0.7 * np.cos(2.1 * x + 0.7 * y) + 0.05 * x / 4.0
    tp = np.stack([x, y, np.round(z * 4096.0) / 4096.0], axis=1).astype(np.float32)
    tn = _unit(np.stack([-zx, -zy, np.ones_like(zx)], axis=1)).astype(np.float32)
    shift = np.array([3.0, -2.0, 1.0], np.float32)
    sp = np.stack([-tp[:, 1], tp[:, 0], tp[:, 2]], axis=1) + shift  # exact
    sn = np.stack([-tn[:, 1], tn[:, 0], tn[:, 2]], axis=1)
    assert sp.dtype == np.float32 and np.array_equal(sp.astype(np.float64), np.stack([-tp[:, 1], tp[:, 0], tp[:, 2]], axis=1).astype(np.float64) + shift.astype(np.float64))
    # target = R^T (source - shift): T_target_source = [R^T | -R^T shift], R = the turn by +90 degrees about z
    Rt = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    T = np.eye(4)
    T[:3, :3] = Rt
    T[:3, 3] = -Rt @ shift.astype(np.float64)
    return tp, tn, sp, sn, T, 0.8

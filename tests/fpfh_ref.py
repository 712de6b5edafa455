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
relative to the entry -- the constant below, derived, not measured.  Zero entries are exactly zero on both sides (no term contributes).

EXACT EDGES (estimate(..., exact_edges=True)).  On a cloud whose every d2 and r * r are exact in f64 (assert_exact recomputes them in integers after scaling by a
power of two and in fractions.Fraction, and raises on any other cloud) a candidate at d2 == r * r is decided by the rule -- strictly outside -- and not by rounding:
it no longer unsettles the point.  A candidate within MARGIN of r * r that is not equal to it still does.  On such a cloud n and the walk order are exact for every
finite point, settled or not (a histogram bin may still hang on the last bits): FpfhRef.n, .neighbors and .finite say so separately from .settled.

SIGNED ZEROS.  A zero n2 (after the swap) makes both arguments of theta = atan2(w . n2, n1 . n2) products with zero: exact zeros whose signs follow IEEE 754 (a sum
of zeros is -0 only when every term is), and atan2 of signed zeros is +-0 or +-pi by rule.  No rounding decides that bin, so such a pair counts as settled in theta
however close nf * 11 is to an integer (pi lands on 11, -pi on 0: bins 10 and 0).

TABLE PLACEMENT (pack_cell, hash_key, fpfh_slots, table_placement): csrc/gp_knn_grid.hpp's key and hash and csrc/gp_fpfh.hip's table size, restated to construct and
certify the `wrap2000` cloud and for nothing else."""
import functools
from fractions import Fraction

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


def pair_features_branch(p1, n1, p2, n2, swap, by_rule=None):
    """compute_pair_features for M pairs (p2, n2: [M, 3]; p1, n1: [3]) with the swap decision given: (features [M, 3] = theta, phi, alpha; angle1, angle2).
    by_rule (a list, optional) receives the mask of the pairs whose theta is atan2 of signed zeros (n2 after the swap is the zero vector)"""
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
    if by_rule is not None:
        by_rule.append((o == 0.0).all(axis=1))
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


def assert_exact(points, radius):
    """raises ValueError unless every d2 = (dx dx + dy dy) + dz dz between two finite points and r * r are exact in f64, recomputed without rounding: the
    coordinates scaled by the smallest power of two that makes them integers, every d2 in integer arithmetic (below 2^62: no overflow) and r * r in
    fractions.Fraction.  -> (D2 exact as int64 [M, M] in units of 4^-k, r * r in those units as an int, the finite mask)"""
    P = np.asarray(points, np.float32).astype(np.float64)
    finite = np.isfinite(P).all(axis=1)
    Q = P[finite]
    r = float(radius)
    if Fraction(r) * Fraction(r) != Fraction(r * r):
        raise ValueError("r * r is rounded in f64")
    k = 0
    while k <= 40 and not np.array_equal(np.rint(np.ldexp(Q, k)), np.ldexp(Q, k)):
        k += 1
    if k > 40 or np.abs(np.ldexp(Q, k)).max(initial=0.0) >= 2.0**29:
        raise ValueError("the coordinates are not integers below 2^29 at any scale up to 2^40: the squared distances are not exact")
    Z = np.ldexp(Q, k).astype(np.int64)
    dz = Z[:, None, :] - Z[None, :, :]
    exact = (dz * dz).sum(axis=-1)  # integers: no rounding anywhere
    D = Q[:, None, :] - Q[None, :, :]
    D2 = (D[..., 0] * D[..., 0] + D[..., 1] * D[..., 1]) + D[..., 2] * D[..., 2]
    if exact.max(initial=0) >= 2**53 or not np.array_equal(np.ldexp(D2, 2 * k), exact.astype(np.float64)):
        raise ValueError("a squared distance is rounded in f64")
    r2 = Fraction(r * r) * 4**k
    if r2.denominator != 1:
        raise ValueError("r * r is not on the squared distances' grid")  # (then no tie exists and exact_edges has nothing to decide)
    return exact, int(r2), finite


def exact_ties(points, radius):
    """the ordered pairs (i, j) of finite points at d2 == r * r exactly, counted in integers (assert_exact): int [T, 2]"""
    exact, r2, finite = assert_exact(points, radius)
    idx = np.nonzero(finite)[0]
    a, b = np.nonzero(exact == r2)
    return np.stack([idx[a], idx[b]], axis=1)


def estimate(points, normals, radius, max_num_neighbors=10000, tie_rule=True, exact_edges=False):
    """-> FpfhRef: hist int64 [N, 33], n int64 [N], settled bool [N], spfh / fpfh float64 [N, 33], row_settled bool [N], neighbors (list of index arrays in walk
    order), sq_dists, num_truncated, num_ties (pairs decided through the both-branches rule), min_bin_margin, min_swap_margin, finite bool [N], cells int64 [N, 3],
    num_exact_ties.  n and neighbors are given for every point, whatever `settled` says.  exact_edges: see the module's text; the guard (assert_exact) runs here,
    so a cloud that does not qualify cannot use it."""
    P, Nn = np.asarray(points, np.float32).astype(np.float64), np.asarray(normals, np.float32).astype(np.float64)
    N = P.shape[0]
    r = float(radius)
    r2 = r * r
    finite = np.isfinite(P).all(axis=1)
    with np.errstate(invalid="ignore"):
        cells = np.where(finite[:, None], cell_of(np.where(finite[:, None], P, 0.0), r), 0)
        D = P[:, None, :] - P[None, :, :]
        D2 = (D[..., 0] * D[..., 0] + D[..., 1] * D[..., 1]) + D[..., 2] * D[..., 2]
        del D
        inside = (D2 < r2) & finite[:, None] & finite[None, :]
        near_edge = (np.abs(D2 - r2) <= MARGIN * r2) & finite[:, None] & finite[None, :]
    out = FpfhRef()
    out.num_exact_ties = 0
    if exact_edges:
        assert_exact(points, radius)  # raises on a cloud whose d2 or r * r are rounded
        out.num_exact_ties = int((near_edge & (D2 == r2)).sum())
        near_edge &= D2 != r2  # d2 == r * r exactly: outside by the rule, nothing hangs on rounding
    out.finite, out.cells = finite, cells
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
        rule0, rule1 = [], []
        f0, a1, a2 = pair_features_branch(P[k], Nn[k], P[others], Nn[others], np.zeros(len(others), bool), rule0)
        f1 = pair_features_branch(P[k], Nn[k], P[others], Nn[others], np.ones(len(others), bool), rule1)[0]
        with np.errstate(invalid="ignore"):
            swap = np.abs(a1) < np.abs(a2)
            gap = np.abs(np.abs(a1) - np.abs(a2))
            tie = gap < MARGIN
        b0, m0 = bins_of(f0)
        b1, m1 = bins_of(f1)
        m0[rule0[0], 0] = np.inf  # theta = atan2 of signed zeros: decided by IEEE 754's rule, not by rounding
        m1[rule1[0], 0] = np.inf
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
        keep = d2 != 0.0
        if keep.any():
            # acc = acc + spfh[j] * (1.0 / q) over the neighbours in walk order (:263-268): accumulate adds strictly in sequence, 0 + x = x
            acc = np.add.accumulate(out.spfh[js[keep]] * (1.0 / d2[keep])[:, None], axis=0)[-1]
        with np.errstate(all="ignore"):
            out.fpfh[i] = acc * (100.0 / acc[:11].sum())  # :271-275
    return out


def walk_end(ref, k):
    """where query k's capped walk stopped, read from the restatement: (the 64-candidate batch, counted inside its cell, of the last accepted neighbour; the number of
    further candidates of that batch).  The device takes a cell's finite points 64 at a time in ascending index."""
    last = int(ref.neighbors[k][-1])
    members = np.nonzero(ref.finite & (ref.cells == ref.cells[last]).all(axis=1))[0]
    pos = int(np.searchsorted(members, last))
    return pos // 64, min(len(members), (pos // 64 + 1) * 64) - pos - 1


# ---- the device's table placement, restated (csrc/gp_knn_grid.hpp pack_cell, csrc/gp_key_table.hpp hash_key and key_claim, csrc/gp_fpfh.hip fpfh_slots) -----------


def pack_cell(x, y, z):
    """three cell coordinates in 21-bit fields, each offset by 2^20: uint64"""
    x, y, z = (np.asarray(c, np.int64) + (1 << 20) for c in (x, y, z))
    return (x.astype(np.uint64) << np.uint64(42)) | (y.astype(np.uint64) << np.uint64(21)) | z.astype(np.uint64)


def hash_key(k):
    """the 64-bit finaliser of the grid's keys, low 32 bits: uint32 (the products wrap modulo 2^64, as the device's)"""
    k = np.atleast_1d(np.asarray(k, np.uint64)).copy()
    with np.errstate(over="ignore"):
        k ^= k >> np.uint64(33)
        k *= np.uint64(0xFF51AFD7ED558CCD)
        k ^= k >> np.uint64(33)
        k *= np.uint64(0xC4CEB9FE1A85EC53)
        k ^= k >> np.uint64(33)
    return (k & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def fpfh_slots(n):
    slots = 1024
    while slots < 2 * int(n):
        slots <<= 1
    return slots


def table_placement(points, radius):
    """the table of one call by linear probing, the finite points' cells inserted ONE AFTER ANOTHER in index order.  The device inserts concurrently: which key sits
    in which slot of a run differs from call to call, but the SET of occupied slots under linear probing does not depend on the insertion order, and a run that
    crosses from slot `mask` to slot 0 crosses it in any order.  -> dict: mask, keys (distinct, in order of first appearance), cells, home, slot, probes (slots
    looked at on insertion, the final one included), wrapped (the key sits below its home slot: its probe ran across the end of the table)"""
    P = np.asarray(points, np.float32).astype(np.float64)
    P = P[np.isfinite(P).all(axis=1)]
    cells = cell_of(P, float(radius))
    keys = pack_cell(cells[:, 0], cells[:, 1], cells[:, 2])
    _, first = np.unique(keys, return_index=True)
    first = np.sort(first)
    keys, cells = keys[first], cells[first]
    mask = fpfh_slots(len(np.asarray(points))) - 1
    home = (hash_key(keys) & np.uint32(mask)).astype(np.int64)
    table = {}
    slot, probes = np.zeros(len(keys), np.int64), np.zeros(len(keys), np.int64)
    for i, h in enumerate(home.tolist()):
        s, c = h, 1
        while s in table:
            s, c = (s + 1) & mask, c + 1
        table[s] = i
        slot[i], probes[i] = s, c
    return dict(mask=mask, keys=keys, cells=cells, home=home, slot=slot, probes=probes, wrapped=slot < home)


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


# ---- the edge clouds of tests/test_fpfh_edges_gpu.py, certified in tests/test_fpfh_ref_cpu.py; figures measured with the restatement alone --------------------------
#   lattice384   the 8 x 8 x 6 lattice at 0.25 m shifted by -0.75 (cells -1 .. 1), random unit normals, r = 0.75.  Exact: 5472 ordered pairs at d2 == r * r, 6 to 93
#                neighbours.  With exact_edges 100 % settled; without it nothing is.
#   dense1500    uniform in a 1.2 m box about the origin (8 cells of about 190 points: three batches each), random unit normals, r = 0.8: 281 to 1359 neighbours.
#   clamp400     r = 0.5; x = 524280 + k / 16, k < 256 drawn at random (cells 2^20 - 16 .. 2^20 + 15 before the clamp at 2^20 - 3), y and z on a 1/64 grid in [0, 1).
#   clamp400neg  its mirror image in x (the clamp at -(2^20 - 3)).  Both exact.
#   wrap2000     2040 points, r = 0.8, 4096 slots: 1951 uniform in a 40 m box, five clumps of 16 in one cell each (there the cap of 8 binds), and at the front nine
#                planted points whose cells hash to the table's last two slots -- three single points and two face-adjacent cells A, B of three points each, all six
#                mutual neighbours -- found by brute force over cells 64 .. with the restated hash.
#   far600       random600 with (1e5, -2e5, 3e4) added in f32: coordinates on grids of 2^-7, 2^-6 and 2^-9.
#   dirty300     signed300's recipe (a NaN point 7, a NaN normal 11), then: six points copied over one to three others each (the copies keep their own normals), a
#                +inf and a -inf coordinate, the point (3e38, -3e38, 3e38), three zero normals.
EDGE_CLOUDS = ("lattice384", "dense1500", "clamp400", "clamp400neg", "wrap2000", "far600", "dirty300")
EXACT_CLOUDS = ("lattice384", "clamp400", "clamp400neg")
DENSE_CAPS = (1, 2, 63, 64, 65, 100, 128, 129, 200)
EDGE_CAPS = {"lattice384": (10000,), "dense1500": (10000,) + DENSE_CAPS, "clamp400": (10000, CAP), "clamp400neg": (10000, CAP), "wrap2000": (10000, CAP),
             "far600": (10000,), "dirty300": (10000,)}
DIRTY = dict(nan_point=7, nan_normal=11, pos_inf=33, neg_inf=77, huge=150, zero_normals=(5, 90, 200), sources=(20, 61, 102, 143, 184, 225), copies=(1, 2, 3, 1, 2, 3))
WRAP_PLANTED = dict(singles=(0, 1, 2), a=(3, 4, 5), b=(6, 7, 8))


def _wrap_cells(mask):
    """brute force with the restated hash: the first face-adjacent (along x) pair of cells and the first three further cells whose home slot is mask - 1 or mask,
    over cubes of 100^3 cells from (64, 64, 64) upwards in z"""
    for z0 in range(64, 64 + 100 * 64, 100):
        g = np.arange(100)
        X, Y, Z = np.meshgrid(64 + g, 64 + g, z0 + g, indexing="ij")
        hit = (hash_key(pack_cell(X.ravel(), Y.ravel(), Z.ravel())) & np.uint32(mask)).reshape(100, 100, 100) >= mask - 1
        pairs = np.argwhere(hit[:-1] & hit[1:])
        if len(pairs) == 0:
            continue
        a = pairs[0]
        b = a + np.array([1, 0, 0])
        singles = [c for c in np.argwhere(hit) if np.abs(c - a).max() > 2 and np.abs(c - b).max() > 2][:3]
        off = np.array([64, 64, z0])
        return a + off, b + off, [c + off for c in singles]
    raise AssertionError("no adjacent pair of cells at the table's end")


@functools.lru_cache(maxsize=None)
def edge_cloud(name):
    """(points f32 [N, 3], normals f32 [N, 3], search_radius) of an edge cloud; the arrays are shared and read-only"""
    rng = np.random.default_rng(20241020)
    if name == "lattice384":
        g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(6), indexing="ij"), axis=-1).reshape(-1, 3)
        p, n, r = (g * 0.25 - 0.75).astype(np.float32), _unit(rng.normal(size=(384, 3))).astype(np.float32), 0.75
    elif name == "dense1500":
        p, n, r = rng.uniform(-0.6, 0.6, (1500, 3)).astype(np.float32), _unit(rng.normal(size=(1500, 3))).astype(np.float32), 0.8
    elif name in ("clamp400", "clamp400neg"):
        x = 524280.0 + rng.integers(0, 256, 400) / 16.0
        p = np.stack([x, rng.integers(0, 64, 400) / 64.0, rng.integers(0, 64, 400) / 64.0], axis=1)
        if name == "clamp400neg":
            p[:, 0] = -p[:, 0]
        assert np.array_equal(p.astype(np.float32).astype(np.float64), p)
        p, n, r = p.astype(np.float32), _unit(rng.normal(size=(400, 3))).astype(np.float32), 0.5
    elif name == "wrap2000":
        r, N = 0.8, 2040
        a, b, singles = _wrap_cells(fpfh_slots(N) - 1)
        face = np.array([(a[0] + 1) * r, (a[1] + 0.5) * r, (a[2] + 0.5) * r])
        side = rng.uniform(-0.1, 0.1, (6, 3))
        side[:, 0] = np.array([-0.05, -0.1, -0.15, 0.05, 0.1, 0.15])  # three points on either side of the face between A and B
        planted = np.concatenate([(np.array(singles) + 0.5) * r, face + side])
        clumps = np.concatenate([(c + rng.uniform(0.05, 0.75, (16, 3))) for c in np.array([[30.0, 30.0, 30.0], [-31.0, 30.0, 0.0], [30.0, -31.0, 0.0], [0.0, 30.0, -31.0], [-31.0, -31.0, -31.0]]) * r])
        p = np.concatenate([planted, rng.uniform(-20.0, 20.0, (N - 9 - 80, 3)), clumps]).astype(np.float32)
        got = cell_of(p[:9], r)
        assert np.array_equal(got[:3], np.array(singles)) and (got[3:6] == a).all() and (got[6:9] == b).all()
        n = _unit(rng.normal(size=(N, 3))).astype(np.float32)
    elif name == "far600":
        p, n, r = cloud("random600")
        p = p + np.array([1e5, -2e5, 3e4], np.float32)
        assert p.dtype == np.float32
    elif name == "dirty300":
        p, n, r = cloud("signed300")
        special = set(DIRTY["sources"]) | set(DIRTY["zero_normals"]) | {DIRTY[k] for k in ("nan_point", "nan_normal", "pos_inf", "neg_inf", "huge")}
        free = [i for i in rng.permutation(300).tolist() if i not in special]
        for src, count in zip(DIRTY["sources"], DIRTY["copies"]):
            for _ in range(count):
                p[free.pop()] = p[src]
        p[DIRTY["pos_inf"], 0] = np.inf
        p[DIRTY["neg_inf"], 2] = -np.inf
        p[DIRTY["huge"]] = np.array([3e38, -3e38, 3e38], np.float32)
        n[list(DIRTY["zero_normals"])] = 0.0
    else:
        raise KeyError(name)
    p, n = np.ascontiguousarray(p, np.float32), np.ascontiguousarray(n, np.float32)
    p.setflags(write=False), n.setflags(write=False)
    return p, n, r


def dirty_copies():
    """dirty300's coincident groups: {source index: the indices that hold a copy of its point}"""
    p = edge_cloud("dirty300")[0]
    return {s: [i for i in range(len(p)) if i != s and np.array_equal(p[i], p[s])] for s in DIRTY["sources"]}


@functools.lru_cache(maxsize=None)
def edge_ref(name, cap=10000):
    """the restatement of an edge cloud under a cap, computed once per process and shared: never modify it"""
    return estimate(*edge_cloud(name), cap, exact_edges=name in EXACT_CLOUDS)


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

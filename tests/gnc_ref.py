"""f64 numpy restatement of the reference's fast global registration (graduated non-convexity), for tests/test_gnc_ref_cpu.py and tests/test_gnc_gpu.py.

Written from the reference sources (paths relative to the reference tree):
  parameters        include/gtsam_points/registration/graduated_non_convexity.hpp:16-36 (inner_iterations is its `innter_iterations`, :28)
  correspondences   include/gtsam_points/registration/impl/graduated_non_convexity_impl.hpp:27-84: the smaller cloud queries (:75-80: size(source) < size(target), else the
                    roles swap and the pairs are swapped back); more than max_init_samples rows are subsampled in ascending order (:36-40); 1-NN of each query row
                    (:52), with reciprocal_check the match's own 1-NN must be the query (:61-68); pairs without a match are erased, the order kept (:82-84).
                    The subsample is NOT the reference's mt19937 shuffle: it is the device's stratified rule (include/gtsam_points_hip.h), restated in Python integers.
  tuple test        :91-131: three draws per tuple (the device's generator; not necessarily distinct), each edge ratio d_target / d_source against tuple_thresh and its
                    inverse (a NaN ratio passes both comparisons), valid tuples' pairs sorted by source (:122) and made unique by source (:123); the reference's
                    unstable sort leaves the surviving target unspecified: the lowest survives here, as on the device
  mu                :134-140 the diagonal of the target's bounding box (over the points with three finite coordinates), sqrt((dx dx + dy dy) + dz dz)
  loop              :149-198.  The correspondence loop's `j` (:158) SHADOWS the inner-iteration `j` (:150), so `i == 0 && j == 0` (:165) forces the weight to 1 for
                    correspondence 0 only, during outer iteration 0, in every inner iteration.  error = |t - T s|^2 (:161-164), weight = (mu / (mu + error))^2 (:165),
                    inliers: error < (2 max_corr_dist)^2 (:143, :169), alignment :176-186, inlier_rate = inliers / N at the pose before the alignment (:187),
                    mu /= div_factor, stop when mu < max_corr_dist (:194-197)

T s is evaluated as ((r0 x + r1 y) + r2 z) + t and the squared norm as (dx dx + dy dy) + dz dz in plain f64, which the device reproduces to the bit; the sums over the
pairs are numpy's pairwise sums here and fixed trees on the device: they agree to N 2^-52 relative, which the comparisons allow for.
"""
import functools

import numpy as np
from ransac_ref import cross_covariance, make_case, make_small_case, match_features, mix, pose_from, rotation_bound, sample_index, transform  # noqa: F401

DEFAULTS = dict(max_init_samples=5000, reciprocal_check=True, tuple_check=False, tuple_thresh=0.9, max_num_tuples=1000, div_factor=1.4, max_corr_dist=0.25, inner_iterations=3,
                max_iterations=64, dof=6, seed=5489)


def params(**kw):
    p = dict(DEFAULTS)
    assert set(kw) <= set(p), kw
    p.update(kw)
    return p


# ---- correspondences ---------------------------------------------------------------------------------------------------------------------------------------------------
def stratified_sample(seed, n, k):
    """k distinct ascending indices below n (k <= n): index_j = lo + sample_index(seed, j, 0, hi - lo), lo = floor(j n / k), hi = floor((j + 1) n / k)"""
    out = []
    for j in range(k):
        lo, hi = j * n // k, (j + 1) * n // k
        out.append(lo + sample_index(seed, j, 0, hi - lo))
    return np.asarray(out, np.int64)


def query_rows(num_query, max_init_samples, seed, query_indices=None):
    if query_indices is not None:
        return np.asarray(query_indices, np.int64).reshape(-1)
    if num_query > max_init_samples:
        return stratified_sample(seed, num_query, max_init_samples)
    return np.arange(num_query, dtype=np.int64)


def find_correspondences(target_features, source_features, p, query_indices=None):
    """dict: pairs int64 [M][2] (target, source), swapped, rows (the queries), forward / back (the matches, -1 without one)"""
    nt, ns = len(target_features), len(source_features)
    swapped = not ns < nt
    qf, of = (target_features, source_features) if swapped else (source_features, target_features)
    rows = query_rows(len(qf), p["max_init_samples"], p["seed"], query_indices)
    forward = match_features(of, qf, rows)[0]
    back = None
    keep = forward >= 0
    if p["reciprocal_check"]:
        back = np.full(len(rows), -1, np.int64)
        ok = np.flatnonzero(forward >= 0)
        back[ok] = match_features(qf, of, forward[ok])[0]
        keep &= back == rows
    q, m = rows[keep], forward[keep]
    pairs = np.stack([q, m] if swapped else [m, q], axis=1).astype(np.int64).reshape(-1, 2)
    return dict(pairs=pairs, swapped=swapped, rows=rows, forward=forward, back=back)


def match_margins(target_features, query_features, rows):
    """(index, relative gap between the two smallest distances) of the 1-NN of each row: what an exact comparison of matches rests on.  The distances are summed
    serially in ascending j, as match_features sums them.  Target rows that are identical bit for bit (the all-zero rows) count once, at their lowest index: their
    distances are the same number in any arithmetic, so the lowest-index rule decides among them on the device as it does here."""
    T = np.asarray(target_features, np.float32).astype(np.float64)
    first = np.sort(np.unique(np.where(np.isnan(T), np.inf, T), axis=0, return_index=True)[1])
    T = T[first]
    Q = np.asarray(query_features, np.float32).astype(np.float64)[np.asarray(rows, np.int64)]
    idx, gap = np.zeros(len(Q), np.int64), np.zeros(len(Q))
    for b in range(0, len(Q), 256):
        acc = np.zeros((len(Q[b : b + 256]), len(T)))
        with np.errstate(invalid="ignore"):
            for j in range(T.shape[1]):
                d = Q[b : b + 256, j : j + 1] - T[None, :, j]
                acc = acc + d * d
        acc = np.where(np.isnan(acc), np.inf, acc)
        two = np.partition(acc, 1, axis=1)[:, :2] if len(T) > 1 else np.concatenate([acc, np.full_like(acc, np.inf)], axis=1)
        idx[b : b + 256] = first[np.argmin(acc, axis=1)]
        with np.errstate(invalid="ignore", divide="ignore"):
            gap[b : b + 256] = np.where(np.isfinite(two[:, 0]), (two[:, 1] - two[:, 0]) / np.maximum(two[:, 1], 1e-300), np.inf)
    return idx, gap


def tuple_ratios(target32, source32, pairs, max_num_tuples, seed):
    """(indices [T][3] into pairs, ratios [T][3]): edge k joins draws k and (k + 1) % 3 (:102-107)"""
    tp = np.asarray(target32, np.float32).astype(np.float64)
    sp = np.asarray(source32, np.float32).astype(np.float64)
    n = len(pairs)
    idx = np.array([[sample_index(seed, i, k, n) for k in range(3)] for i in range(max_num_tuples)], np.int64).reshape(-1, 3)
    ratios = np.zeros((max_num_tuples, 3))
    for k in range(3):
        a, b = pairs[idx[:, k]], pairs[idx[:, (k + 1) % 3]]
        dt, ds = tp[a[:, 0]] - tp[b[:, 0]], sp[a[:, 1]] - sp[b[:, 1]]
        d1 = np.sqrt((dt[:, 0] * dt[:, 0] + dt[:, 1] * dt[:, 1]) + dt[:, 2] * dt[:, 2])
        d2 = np.sqrt((ds[:, 0] * ds[:, 0] + ds[:, 1] * ds[:, 1]) + ds[:, 2] * ds[:, 2])
        with np.errstate(invalid="ignore", divide="ignore"):
            ratios[:, k] = d1 / d2
    return idx, ratios


def tuple_test(target32, source32, pairs, p):
    """the pairs behind the tuple test (unchanged when it does not run, :91)"""
    if not p["tuple_check"] or len(pairs) <= 3 * p["max_num_tuples"]:
        return pairs
    idx, ratios = tuple_ratios(target32, source32, pairs, p["max_num_tuples"], p["seed"])
    with np.errstate(invalid="ignore"):
        valid = ~((ratios < p["tuple_thresh"]) | (ratios > 1.0 / p["tuple_thresh"])).any(axis=1)
    lowest = {}
    for t, s in pairs[idx[valid].reshape(-1)].tolist():
        lowest[s] = min(lowest.get(s, t), t)
    return np.array([[lowest[s], s] for s in sorted(lowest)], np.int64).reshape(-1, 2)


# ---- the loop ----------------------------------------------------------------------------------------------------------------------------------------------------------
def diameter(target32):
    p = np.asarray(target32, np.float32).reshape(-1, 3).astype(np.float64)
    p = p[np.isfinite(p).all(axis=1)]
    if not len(p):
        return 0.0
    d = p.max(axis=0) - p.min(axis=0)
    return float(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))


def errors_and_weights(t, s32, T, mu, outer):
    """(e, w) of every pair at T: the weight of pair 0 is forced to 1 throughout outer iteration 0 (the shadowed j of :165)"""
    d = t - transform(s32, T)
    e = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    q = mu / (mu + e)
    w = q * q
    if outer == 0 and len(w):
        w[0] = 1.0
    return e, w


def weighted_cross_covariance(t, s, w):
    """ransac_ref.cross_covariance(t, s, w) with numpy's sums over the pairs instead of the serial ones (tests/test_gnc_ref_cpu.py holds the two together)"""
    sw = w.sum()
    mt, ms = (w[:, None] * t).sum(axis=0) / sw, (w[:, None] * s).sum(axis=0) / sw
    H = ((w[:, None] * (t - mt))[:, :, None] * (s - ms)[:, None, :]).sum(axis=0)
    return H, mt, ms


def align_step(t, s, T, mu, outer, p):
    """one alignment at the pose T: dict of the new pose, H, the means, sum_weights, sum_errors, num_inliers, e, w"""
    e, w = errors_and_weights(t, s, T, mu, outer)
    H, mt, ms = weighted_cross_covariance(t, s, w)
    thresh = (2.0 * p["max_corr_dist"]) * (2.0 * p["max_corr_dist"])
    return dict(T=pose_from(H, mt, ms, p["dof"]), H=H, mean_t=mt, mean_s=ms, sum_weights=float(w.sum()), sum_errors=float(e.sum()), num_inliers=int((e < thresh).sum()), e=e, w=w)


def schedule(mu0, p):
    """[(outer iteration, mu)] of every alignment, and mu behind the last division: the reference's own sequence of divisions"""
    mu, out = float(mu0), []
    for i in range(p["max_iterations"]):
        out += [(i, mu)] * p["inner_iterations"]
        mu = mu / p["div_factor"]
        if mu < p["max_corr_dist"]:
            break
    return out, mu


def gnc_loop(target32, source32, pairs, p, mu0=None):
    """the loop on its own poses: dict of T, inlier_rate, num_alignments, final_mu, steps (align_step of every alignment, with `mu`, `outer` and `T_before`)"""
    tp = np.asarray(target32, np.float32).astype(np.float64)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    T = np.eye(4)
    if not len(pairs):
        return dict(T=T, inlier_rate=0.0, num_alignments=0, final_mu=0.0, steps=[])
    t, s = tp[pairs[:, 0]], np.asarray(source32, np.float32)[pairs[:, 1]]
    sched, final_mu = schedule(diameter(target32) if mu0 is None else mu0, p)
    steps, rate = [], 0.0
    for outer, mu in sched:
        st = align_step(t, s.astype(np.float64), T, mu, outer, p)
        st.update(mu=mu, outer=outer, T_before=T)
        rate = st["num_inliers"] / float(len(pairs))
        T = st["T"]
        steps.append(st)
    return dict(T=T, inlier_rate=rate, num_alignments=len(steps), final_mu=final_mu, steps=steps)


def estimate_pose_gnc(target32, source32, target_features, source_features, p, query_indices=None):
    """the three stages: gnc_loop's dict with `pairs`, `initial_pairs` (before the tuple test), `swapped`, `num_initial`"""
    c = find_correspondences(target_features, source_features, p, query_indices)
    pairs = tuple_test(target32, source32, c["pairs"], p)
    out = gnc_loop(target32, source32, pairs, p)
    out.update(pairs=pairs, initial_pairs=c["pairs"], swapped=c["swapped"], num_initial=len(c["rows"]), corr=c)
    return out


@functools.lru_cache(maxsize=None)
def case_result(small, dof, reciprocal, far=0.0):
    """the restatement on make_case / make_small_case, computed once for the tests that share it: (case, params, estimate_pose_gnc's dict)"""
    c = make_small_case(dof, far=far) if small else make_case(dof)
    p = params(dof=dof, reciprocal_check=reciprocal)
    return c, p, estimate_pose_gnc(c["target"], c["source"], c["target_features"], c["source_features"], p)


def pose_error(T, T_true):
    """(Frobenius norm of the rotation difference, norm of the translation difference)"""
    return float(np.linalg.norm(T[:3, :3] - T_true[:3, :3])), float(np.linalg.norm(T[:3, 3] - T_true[:3, 3]))

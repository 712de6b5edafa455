"""CPU checks of the continuous-time factors' restatement (tests/ct_ref.py) the GPU tests compare against, of the fixtures those tests use, and of what the
library decides on the host: the exports and the argument refusals made before any device work."""
import ctypes as C

import numpy as np
import pytest

import ct_ref
from helpers import expmap

from gtsam_points_amd.features import IntegratedCTGICPFactorGPU, IntegratedCTICPFactorGPU  # noqa: F401  (what the restatement stands beside: no device code, no tests of it)

T0 = expmap([0.01, -0.02, 0.03, 0.1, 0.2, -0.1])
T1 = T0 @ expmap([0.02, 0.01, -0.03, 0.3, -0.1, 0.05])
# the poses the factors are linearised at: near, but not at, the truth (T0, T1) the fixtures were skewed with
A0 = T0 @ expmap([0.003, -0.002, 0.001, 0.02, -0.01, 0.03])
A1 = T1 @ expmap([-0.002, 0.004, 0.001, -0.03, 0.02, 0.01])
POSE_PAIRS = {"moving": (A0, A1), "still": (A0, A0.copy()), "far": (A0, A0 @ expmap([0.4, -0.3, 0.5, 1.0, 2.0, -1.5]))}


def bin_layout(name, n):
    """bin of every point for the layouts the GPU tests cover (tile = 1024 points)"""
    i = np.arange(n)
    if name == "one":
        return np.zeros(n, dtype=np.int64)
    if name == "own":
        return i
    if name == "eight":
        return i * 8 // n
    return (i >= {"edge": 1024, "before": 1023, "after": 1025}[name]).astype(np.int64)


LAYOUTS = ["one", "edge", "before", "after", "own", "eight"]


def fixture(n, layout="eight"):
    return ct_ref.skewed_scan(n, T0, T1, bin_layout(layout, n))


def make_ref(kind, fx, cutoff=1.0):
    return ct_ref.CTFactorRef(kind, fx["target_points"], fx["target_normals"], fx["target_covs"], fx["points"], fx["covs"], fx["times"], cutoff)


# ---- the pose table ----------------------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("pair", list(POSE_PAIRS))
def test_pose_table_ends_and_orthonormality(pair):
    P0, P1 = POSE_PAIRS[pair]
    T, D0, D1 = ct_ref.pose_table(P0, P1, np.array([0.0, 0.25, 0.5, 1.0]))
    assert np.abs(D0[0] - np.eye(6)).max() < 1e-14 and np.abs(D1[0]).max() == 0.0
    assert np.abs(D0[-1]).max() < 1e-13 and np.abs(D1[-1] - np.eye(6)).max() < 1e-13
    assert np.abs(T[0] - P0).max() < 1e-15 and np.abs(T[-1] - P1).max() < 1e-13
    for Tt in T:
        assert np.abs(Tt[:3, :3] @ Tt[:3, :3].T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(Tt[:3, :3]) - 1.0) < 1e-14
        assert np.array_equal(Tt[3], [0.0, 0.0, 0.0, 1.0])


def test_pose_table_derivatives_match_central_differences():
    """D0 / D1 are the right-trivialised derivatives of T(t): T(t; P0 Exp(d0), P1 Exp(d1)) = T(t) Exp(D0 d0 + D1 d1) to first order"""
    h = 1e-6
    table = np.array([0.0, 0.3, 0.7, 1.0])
    for P0, P1 in POSE_PAIRS.values():
        T, D0, D1 = ct_ref.pose_table(P0, P1, table)
        for which, D in ((0, D0), (1, D1)):
            for k in range(6):
                d = np.zeros(6)
                d[k] = h
                plus = ct_ref.pose_table(P0 @ expmap(d) if which == 0 else P0, P1 @ expmap(d) if which == 1 else P1, table)[0]
                minus = ct_ref.pose_table(P0 @ expmap(-d) if which == 0 else P0, P1 @ expmap(-d) if which == 1 else P1, table)[0]
                for b in range(len(table)):
                    col = (ct_ref.logmap(ct_ref.inverse(T[b]) @ plus[b]) - ct_ref.logmap(ct_ref.inverse(T[b]) @ minus[b])) / (2 * h)
                    assert np.abs(col - D[b][:, k]).max() < 1e-8, (which, k, b)


# ---- the records -------------------------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("pair", list(POSE_PAIRS))
def test_record_matches_central_differences(kind, pair):
    """with correspondences and M frozen: [b_0 | b_1] = 1/2 the central-difference gradient of error() over the 12 tangent directions (the HessianFactor's g = -b is
    -1/2 of it) and H = J^T J with J the central differences of the stacked residuals"""
    P0, P1 = POSE_PAIRS[pair]
    ref = make_ref(kind, fixture(600))
    L = ref.linearize(P0, P1)
    assert L["num_inliers"] > 300 or pair == "far"
    assert L["num_inliers"] > 20
    H, b = ct_ref.system12(L)
    h = 1e-6
    grad, cols = np.zeros(12), []
    for k in range(12):
        d = np.zeros(12)
        d[k] = h
        plus, minus = (P0 @ expmap(d[:6]), P1 @ expmap(d[6:])), (P0 @ expmap(-d[:6]), P1 @ expmap(-d[6:]))
        grad[k] = (ref.error(*plus) - ref.error(*minus)) / (2 * h)
        cols.append(((ref.residuals(*plus) - ref.residuals(*minus)) / (2 * h)).ravel())
    J = np.stack(cols, axis=1)
    rho = ref.residuals(P0, P1)
    assert abs((rho * rho).sum() - L["error"]) <= 1e-12 * L["error"]
    assert np.abs(0.5 * grad - b).max() <= 1e-6 * np.abs(b).max()
    assert np.abs(J.T @ rho.ravel() - b).max() <= 1e-6 * np.abs(b).max()
    assert np.abs(J.T @ J - H).max() <= 1e-6 * np.abs(H).max()
    assert ref.searches == 1  # error() and residuals() never search once correspondences are stored


def test_gicp_error_keeps_the_mahalanobis_of_the_linearisation():
    ref = make_ref(1, fixture(300))
    ref.linearize(A0, A1)
    M = ref.M.copy()
    ref.error(T0, T1)
    assert np.array_equal(ref.M, M)
    fresh = make_ref(1, fixture(300))
    fresh.error(T0, T1)  # nothing stored: searches, and takes M, at the given poses
    assert fresh.searches == 1 and not np.array_equal(fresh.M, M)


def test_deskewing_with_the_true_poses_puts_the_scan_back_on_the_walls():
    fx = fixture(500)
    ref = make_ref(0, fx)
    world = ref.deskewed(T0, T1)
    _, d1, _ = ct_ref.nearest(world[:, :3], fx["target_points"])
    raw, _, _ = ct_ref.pose_table(T0, T0, ref.table)
    _, d_raw, _ = ct_ref.nearest(ct_ref.transform(raw, ref.indices, ref.p), fx["target_points"])
    assert np.median(d1) < np.median(d_raw)
    local = ref.deskewed(T0, T1, local=True)
    assert np.abs((T0 @ local.T).T - world).max() < 1e-12 and (world[:, 3] == 1.0).all()


# ---- the time table ----------------------------------------------------------------------------------------------------------------------------------------------


def test_time_table_cases():
    table, idx = ct_ref.time_table(np.full(7, 0.25, np.float32))
    assert np.array_equal(table, [1.0]) and not idx.any()  # all times equal: one bin, normalised by itself
    table, idx = ct_ref.time_table(np.array([0.0, 0.0, 0.1, 0.1], np.float32))
    assert np.array_equal(table, [0.0, 1.0]) and np.array_equal(idx, [0, 0, 1, 1])
    # the threshold: strict, and compared in f64 on the f32 times.  1e-3 is no dyadic number, so no two f32 times are exactly 1e-3 apart; the two f32 gaps around
    # it are float32(1e-3) = 0.0010000000475 (a new bin -- a comparison in f32 would see no excess) and the f32 just below (none)
    above = np.float32(1e-3)
    below = np.nextafter(above, np.float32(0.0))
    assert float(below) < 1e-3 < float(above)
    assert np.array_equal(ct_ref.time_table(np.array([0.0, above], np.float32))[1], [0, 1])
    assert np.array_equal(ct_ref.time_table(np.array([0.0, below], np.float32))[1], [0, 0])
    assert np.array_equal(ct_ref.time_table(np.array([0.0, 1.0, 1.0 + 2.0**-10], np.float32))[1], [0, 1, 1])  # 2^-10 < 1e-3 < 2^-9, exact in f32 next to 1
    assert np.array_equal(ct_ref.time_table(np.array([0.0, 1.0, 1.0 + 2.0**-9], np.float32))[1], [0, 1, 2])
    # unsorted: greedy in index order, a time that goes back joins the last bin
    table, idx = ct_ref.time_table(np.array([0.0, 0.5, 0.2, 0.9, 0.1], np.float32))
    assert np.array_equal(idx, [0, 1, 1, 2, 2]) and np.array_equal(table, [0.0, 0.5 / float(np.float32(0.9)), 1.0])
    # not starting at 0: no offset is taken off
    table, idx = ct_ref.time_table(np.array([10.0, 10.05, 10.1], np.float32))
    assert np.array_equal(idx, [0, 1, 2]) and table[0] == 10.0 / float(np.float32(10.1)) and table[-1] == 1.0
    # a last time of 0: the 1e-9 guard
    table, idx = ct_ref.time_table(np.array([-0.5, 0.0], np.float32))
    assert np.array_equal(table, [-0.5 / 1e-9, 0.0]) and np.array_equal(idx, [0, 1])
    assert ct_ref.time_table(np.zeros(0, np.float32))[0].size == 0


def test_bin_layouts_give_the_bins_they_name():
    for name, bins in (("one", 1), ("edge", 2), ("before", 2), ("after", 2), ("own", 2049), ("eight", 8)):
        table, idx = ct_ref.time_table(ct_ref.bins_to_times(bin_layout(name, 2049)))
        assert len(table) == bins and np.array_equal(idx, bin_layout(name, 2049)), name


# ---- the fixtures of the GPU tests: no query on a tie or on the cut-off ----------------------------------------------------------------------------------------------

SIZES = [1, 255, 256, 257, 1023, 1024, 1025, 2049]
MARGIN = 1e-9


def guarded_cases():
    """(n, layout, poses, cut-off) of every search the GPU tests compare exactly"""
    cases = [(n, "eight", "moving", 1.0) for n in SIZES]
    cases += [(2049, layout, "moving", 1.0) for layout in LAYOUTS]
    cases += [(2049, "eight", "still", 1.0), (600, "eight", "far", 1.0)]
    return cases


def one_match_cutoff(ref, P0, P1):
    """a cut-off (distance) between the smallest and the second-smallest nearest distance of the fixture: exactly one point matches"""
    T, _, _ = ct_ref.pose_table(P0, P1, ref.table)
    _, d1, _ = ct_ref.nearest(ct_ref.transform(T, ref.indices, ref.p), ref.tp)
    lo, hi = np.sort(d1)[:2]
    return float(np.sqrt(0.5 * (lo + hi)))


@pytest.mark.parametrize("case", guarded_cases(), ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}")
def test_fixtures_have_no_ties_and_nothing_on_the_cutoff(case):
    n, layout, pair, cutoff = case
    ref = make_ref(0, fixture(n, layout), cutoff)
    P0, P1 = POSE_PAIRS[pair]
    T, _, _ = ct_ref.pose_table(P0, P1, ref.table)
    gap, edge = ct_ref.margins(T, ref.indices, ref.p, ref.tp, ref.max_sq)
    assert gap > MARGIN and edge > MARGIN, (gap, edge)
    if n == 2049 and layout == "eight" and pair == "moving":
        c = one_match_cutoff(ref, P0, P1)
        gap, edge = ct_ref.margins(T, ref.indices, ref.p, ref.tp, c * c)
        assert edge > MARGIN and (ct_ref.correspondences(T, ref.indices, ref.p, ref.tp, c * c) >= 0).sum() == 1
        assert (ct_ref.correspondences(T, ref.indices, ref.p, ref.tp, 1e-12) >= 0).sum() == 0 and ct_ref.margins(T, ref.indices, ref.p, ref.tp, 1e-12)[1] > 1e-12


# ---- the library's host side -------------------------------------------------------------------------------------------------------------------------------------

NEW_SYMBOLS = ["gp_ct_factor_create", "gp_ct_factor_destroy", "gp_ct_factor_linearize", "gp_ct_factor_compute_error", "gp_ct_factor_deskew", "gp_ct_factor_num_time_bins",
               "gp_ct_factor_time_table", "gp_ct_factor_pose_table", "gp_ct_factor_correspondences"]


def test_new_names_are_exported():
    import gtsam_points_amd as gpa
    from gtsam_points_amd import _capi

    lib = _capi.load()
    for s in NEW_SYMBOLS:
        assert s in _capi.EXPORTED_SYMBOLS and hasattr(lib, s), s
    for name in ("IntegratedCTICPFactorGPU", "IntegratedCTGICPFactorGPU"):
        assert name in gpa.__all__ and hasattr(gpa, name), name
    assert issubclass(gpa.IntegratedCTGICPFactorGPU, gpa.IntegratedCTICPFactorGPU)


def test_entry_points_refuse_bad_arguments_without_a_device():
    from gtsam_points_amd import _capi

    lib = _capi.load()
    INVALID = 1  # GP_ERROR_INVALID_ARGUMENT
    fake = C.c_void_p(64)  # never dereferenced: every call below is refused first
    h = C.c_void_p()
    # (grid, target points, normals, covs, num_target, points, covs, times, num_points, max_sq, kind, stream, out)
    good = [fake, fake, fake, fake, 1, fake, fake, fake, 1, 1.0, 0, None, C.byref(h)]
    for kind, nulls in ((0, (0, 5, 7, 2)), (1, (0, 5, 7, 3, 6))):  # a NULL grid, points or times; kind 0 without normals; kind 1 without either covariance array
        for at in nulls:
            args = list(good)
            args[10] = kind
            args[at] = None
            assert lib.gp_ct_factor_create(*args) == INVALID and not h.value, (kind, at)
            assert b"gp_ct_factor_create" in lib.gp_last_error()
    for at, bad in ((9, -1.0), (9, float("nan")), (10, 2), (8, -1)):  # a negative cut-off; a kind that is neither; a negative count
        args = list(good)
        args[at] = bad
        assert lib.gp_ct_factor_create(*args) == INVALID and not h.value, (at, bad)
    assert lib.gp_ct_factor_destroy(None) == 0 and lib.gp_ct_factor_num_time_bins(None) == 0
    assert lib.gp_ct_factor_linearize(None, None, None, None) == INVALID and lib.gp_ct_factor_compute_error(None, None, None, None) == INVALID
    assert lib.gp_ct_factor_deskew(None, None, None, 0, None) == INVALID and lib.gp_ct_factor_time_table(None, None, None) == INVALID
    assert lib.gp_ct_factor_pose_table(None, None) == INVALID and lib.gp_ct_factor_correspondences(None, None) == INVALID

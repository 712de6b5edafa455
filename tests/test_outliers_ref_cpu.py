"""tests/outliers_ref.py checked without a GPU: the restatement against a literal triple loop, every edge case of the device tests on the restatement alone, the
tie-band condition on the golden scans that lets tests/test_outliers_gpu.py compare inlier sets exactly, and the C entry points' refusals (host code)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import outliers_ref as orf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gp_cloud_mean_neighbor_distances", "gp_cloud_mean_neighbor_distances_from", "gp_cloud_inlier_threshold", "gp_cloud_select_below", "gp_cloud_select_mask",
               "gp_cloud_sort_by_time_indices")
NEW_NAMES = ("find_inlier_points_gpu", "remove_outliers_gpu", "filter_gpu", "sort_by_time_gpu")


def literal_find_inlier_points(points, k, std_thresh):
    """:576-612 and :619-629 as loops over python floats (f64), brute-force neighbours"""
    p = [[float(c) for c in row] for row in np.asarray(points, np.float32)]
    n = len(p)
    dists = []
    for i in range(n):
        def sq_norm(j):
            dx, dy, dz = p[j][0] - p[i][0], p[j][1] - p[i][1], p[j][2] - p[i][2]
            return dx * dx + dy * dy + dz * dz

        nearest = sorted(range(n), key=lambda j: (sq_norm(j), j))
        sum_dist = 0.0
        for j in range(k):
            sum_dist += math.sqrt(sq_norm(nearest[j]))
        dists.append(sum_dist / k)
    sum_dists = sum_sq_dists = 0.0
    for d in dists:
        sum_dists += d
        sum_sq_dists += d * d
    mean = sum_dists / n
    var = sum_sq_dists / n - mean * mean
    thresh = mean + math.sqrt(var) * std_thresh
    return [i for i in range(n) if dists[i] < thresh], dists, mean, var, thresh


def test_restatement_equals_the_literal_loops():
    rng = np.random.default_rng(0)
    pts = rng.normal(size=(60, 3)).astype(np.float32) * 3
    pts[50:] *= 6  # a sparse fringe: real outliers
    for k, std in [(1, 1.0), (5, 1.0), (10, 1.0), (10, 2.0), (20, 0.5), (60, 1.0)]:
        inl, dists, mean, var, thresh = literal_find_inlier_points(pts, k, std)
        for brute in (False, True):
            r = orf.find_inlier_points(pts, k, std, brute=brute)
            assert np.array_equal(r["dists"], np.array(dists)), (k, brute)  # same operations in the same order: the same bits
            assert (r["mean"], r["var"], r["thresh"]) == (mean, var, thresh) and r["indices"].tolist() == inl and r["m"] == 60 and r["num_short"] == 0
        if k == 10 and std == 1.0:
            assert 0 < len(inl) < 60 and not set(range(50, 60)) <= set(inl)
    # the caller's lists (first overload) in list order
    nb = orf.knn_indices(pts, 7)
    a = orf.find_inlier_points(pts, 7, 1.0)
    b = orf.find_inlier_points(pts, 7, 1.0, neighbors=nb.reshape(-1))
    assert np.array_equal(a["dists"], b["dists"]) and np.array_equal(a["indices"], b["indices"])


def test_edge_cases_on_the_restatement():
    rng = np.random.default_rng(1)
    r = orf.find_inlier_points(np.zeros((0, 3), np.float32), 10, 1.0)
    assert len(r["indices"]) == 0 and (r["mean"], r["var"], r["thresh"], r["m"], r["num_short"]) == (0.0, 0.0, 0.0, 0, 0)
    r = orf.find_inlier_points(np.ones((1, 3), np.float32), 1, 1.0)  # d = 0, thresh = 0: 0 < 0 is false, as in the reference
    assert r["dists"].tolist() == [0.0] and r["thresh"] == 0.0 and len(r["indices"]) == 0 and r["m"] == 1
    r = orf.find_inlier_points(rng.normal(size=(9, 3)), 10, 1.0)  # n < k: every point is short
    assert r["num_short"] == 9 and r["m"] == 0 and np.isinf(r["dists"]).all() and len(r["indices"]) == 0 and r["thresh"] == 0.0
    r = orf.find_inlier_points(rng.normal(size=(10, 3)), 10, 1.0)  # n == k: every list is the whole cloud
    assert r["num_short"] == 0 and r["m"] == 10 and 0 < len(r["indices"]) < 10
    for n in (127, 128, 129, 255, 256, 257, 1025):
        pts = rng.normal(size=(n, 3)).astype(np.float32)
        r = orf.find_inlier_points(pts, 10, 1.0)
        assert r["m"] == n and 0.5 * n < len(r["indices"]) < n and (np.diff(r["indices"]) > 0).all()
        assert len(orf.find_inlier_points(pts, 1, 1.0)["indices"]) == 0  # k = 1: every d is 0, nothing lies below 0
        assert 0 < len(orf.find_inlier_points(pts, 32, 1.0)["indices"]) < n
    # 64 copies of one point + 64 distinct points, k = 10: the copies have d = 0 whichever of their 63 twins are listed
    pts = np.concatenate([np.tile(np.float32([[1.5, -2.0, 0.25]]), (64, 1)), rng.normal(size=(64, 3)).astype(np.float32) * 4])
    r = orf.find_inlier_points(pts, 10, 1.0)
    assert (r["dists"][:64] == 0).all() and (r["dists"][64:] > 0).all() and set(range(64)) <= set(r["indices"].tolist())
    # one NaN and one inf coordinate in 300 points: short, out of the statistics, out of the result
    pts = rng.normal(size=(300, 3)).astype(np.float32)
    pts[17, 1], pts[211, 2] = np.nan, np.inf
    r = orf.find_inlier_points(pts, 10, 1.0)
    clean = orf.find_inlier_points(np.delete(pts, [17, 211], axis=0), 10, 1.0)
    assert r["num_short"] == 2 and r["m"] == 298 and np.isinf(r["dists"][[17, 211]]).all() and not {17, 211} & set(r["indices"].tolist())
    assert (r["mean"], r["var"], r["thresh"]) == (clean["mean"], clean["var"], clean["thresh"]) and len(r["indices"]) == len(clean["indices"])
    # std_thresh = 0: below the mean; std_thresh = -1: below mean - sigma
    pts = rng.normal(size=(500, 3)).astype(np.float32)
    r0, r1, rm = (orf.find_inlier_points(pts, 10, s) for s in (0.0, 1.0, -1.0))
    assert r0["thresh"] == r0["mean"] and rm["thresh"] < r0["thresh"] < r1["thresh"] and len(rm["indices"]) < len(r0["indices"]) < len(r1["indices"])
    assert set(rm["indices"].tolist()) <= set(r0["indices"].tolist()) <= set(r1["indices"].tolist())
    # lists with -1 and n: those points are short, the others keep the reference's d
    nb = orf.knn_indices(pts, 10)
    bad = nb.copy()
    bad[3, 9], bad[400, 0] = -1, 500
    r = orf.find_inlier_points(pts, 10, 1.0, neighbors=bad)
    assert r["num_short"] == 2 and r["m"] == 498 and np.isinf(r["dists"][[3, 400]]).all()
    keep = np.ones(500, bool)
    keep[[3, 400]] = False
    assert np.array_equal(r["dists"][keep], r1["dists"][keep])


def test_sort_by_time_and_filter_restatements():
    rng = np.random.default_rng(2)
    vals = np.concatenate([rng.normal(size=990).astype(np.float32), np.float32([0.0, -0.0, 1e-45, -1e-45, 1e-40, np.inf, -np.inf, -3.5, 3.5, 2.0 ** -126])])
    t = vals[rng.integers(0, len(vals), size=5000)]
    t[[5, 1700, 4999]] = np.nan
    t[[10, 11, 12, 13]] = np.float32([-0.0, 0.0, -0.0, 0.0])
    idx = orf.sort_by_time(t)
    want = sorted(range(len(t)), key=lambda i: (math.isnan(t[i]), 0.0 if math.isnan(t[i]) else float(t[i]), i))  # python's sort is stable; -0.0 == 0.0
    assert idx.tolist() == want
    s = t[idx]
    assert np.isnan(s[-3:]).all() and idx[-3:].tolist() == [5, 1700, 4999] and (s[1:-3] >= s[:-4]).all()
    zeros = idx[np.flatnonzero(s == 0)]
    assert (np.diff(zeros) > 0).all() and {10, 11, 12, 13} <= set(zeros.tolist())
    k = orf.time_sort_keys(np.float32([-np.inf, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, np.inf, np.nan]))
    assert (np.diff(k.astype(np.int64)) >= 0).all() and k[3] == k[4] and k[-1] == 0xFFFFFFFF and len(set(k.tolist())) == 8
    assert orf.sort_by_time(np.zeros(0, np.float32)).tolist() == [] and orf.sort_by_time(np.float32([3.0])).tolist() == [0]
    mask = rng.integers(0, 2, size=1000).astype(bool)
    assert orf.filter_indices(mask).tolist() == [i for i in range(1000) if mask[i]] and orf.filter_indices(mask.astype(np.uint8) * 7).tolist() == orf.filter_indices(mask).tolist()


def test_tie_band_is_empty_on_the_golden_scans():
    """tests/test_outliers_gpu.py compares the device's inlier set with the restatement's EXACTLY.  That is fair only if no point lies so close to the threshold that
    two correct roundings may disagree: for both scans, k in {5, 10, 20} and std_thresh in {1, 2}, no point has |d_i - thresh| <= 1e-9 thresh (the closest one
    measured lies 7.6e-6 thresh away), and mean^2 / var is between 0.45 and 0.61, so the one-pass variance does not cancel.  A condition on the inputs, not a
    relaxation of the comparison."""
    kept = {}
    closest = np.inf
    for name in orf.SCANS:
        pts = orf.scan(name)
        assert len(np.unique(pts, axis=0)) == len(pts)  # no duplicate points
        for k in orf.KS:
            for std in orf.STD_THRESHS:
                r = orf.scan_reference(name, k, std)
                gap = float(np.abs(r["dists"] - r["thresh"]).min() / r["thresh"])
                closest = min(closest, gap)
                assert gap > 1e-9, (name, k, std, gap)
                assert 0.4 < r["mean"] ** 2 / r["var"] < 0.7, (name, k, std, r["mean"] ** 2 / r["var"])
                kept[name, k, std] = len(r["indices"])
    print(f"closest point to a threshold: {closest:.2e} thresh")
    assert closest > 1e-6
    assert (len(orf.scan(orf.SCANS[0])), kept[orf.SCANS[0], 10, 1.0]) == (124_668, 115_152)
    assert (len(orf.scan(orf.SCANS[1])), kept[orf.SCANS[1], 10, 1.0]) == (124_605, 115_308)


def test_header_binding_table_and_package_have_the_new_names():
    hdr = open(os.path.join(ROOT, "include", "gtsam_points_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    from gtsam_points_amd import _capi

    for s in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + s + r"\s*\(", hdr), f"{s} is not declared in include/gtsam_points_hip.h"
        assert s in _capi.EXPORTED_SYMBOLS, f"{s} is not in _capi.EXPORTED_SYMBOLS"
    import gtsam_points_amd as gpa

    for name in NEW_NAMES:
        assert callable(getattr(gpa, name)) and name in gpa.__all__, name


def test_argument_checks_need_no_device():
    """NULL arrays with n > 0, n < 0, k outside its range, a std_thresh that is not finite: GP_ERROR_INVALID_ARGUMENT before any device work (this host has no
    device); n == 0 is legal everywhere and launches nothing"""
    from gtsam_points_amd import _capi

    lib = _capi.load()
    p, q, o = C.c_void_p(256), C.c_void_p(512), C.c_void_p(1024)  # never dereferenced
    short, kept = C.c_int(7), C.c_int(7)
    stats = (C.c_double * 4)(7, 7, 7, 7)
    for k in (0, 33, -1):
        assert lib.gp_cloud_mean_neighbor_distances(p, q, 100, k, o, C.byref(short), None) == 1
    for grid, pts, out in [(None, q, o), (p, None, o), (p, q, None)]:
        assert lib.gp_cloud_mean_neighbor_distances(grid, pts, 100, 10, out, C.byref(short), None) == 1
    assert lib.gp_cloud_mean_neighbor_distances(p, q, -1, 10, o, C.byref(short), None) == 1
    assert lib.gp_cloud_mean_neighbor_distances(None, None, 0, 10, None, C.byref(short), None) == 0 and short.value == 0
    assert lib.gp_cloud_mean_neighbor_distances(None, None, 0, 10, None, None, None) == 0
    for k in (0, -5):
        assert lib.gp_cloud_mean_neighbor_distances_from(p, 100, q, k, o, C.byref(short), None) == 1
    for pts, nb, out in [(None, q, o), (p, None, o), (p, q, None)]:
        assert lib.gp_cloud_mean_neighbor_distances_from(pts, 100, nb, 10, out, C.byref(short), None) == 1
    assert lib.gp_cloud_mean_neighbor_distances_from(p, -1, q, 10, o, None, None) == 1
    short.value = 7
    assert lib.gp_cloud_mean_neighbor_distances_from(None, 0, None, 1000, None, C.byref(short), None) == 0 and short.value == 0
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert lib.gp_cloud_inlier_threshold(p, 100, bad, stats, None) == 1 and b"finite" in lib.gp_last_error()
    assert lib.gp_cloud_inlier_threshold(None, 100, 1.0, stats, None) == 1 and lib.gp_cloud_inlier_threshold(p, 100, 1.0, None, None) == 1
    assert lib.gp_cloud_inlier_threshold(p, -1, 1.0, stats, None) == 1
    assert lib.gp_cloud_inlier_threshold(None, 0, 1.0, stats, None) == 0 and list(stats) == [0.0, 0.0, 0.0, 0.0]
    for vals, out, cnt in [(None, o, C.byref(kept)), (p, None, C.byref(kept)), (p, o, None)]:
        assert lib.gp_cloud_select_below(vals, 100, 1.0, out, cnt, None) == 1
        assert lib.gp_cloud_select_mask(vals, 100, out, cnt, None) == 1
    assert lib.gp_cloud_select_below(p, -1, 1.0, o, C.byref(kept), None) == 1 and lib.gp_cloud_select_mask(p, -1, o, C.byref(kept), None) == 1
    assert lib.gp_cloud_select_below(None, 0, 1.0, None, C.byref(kept), None) == 0 and kept.value == 0
    kept.value = 7
    assert lib.gp_cloud_select_mask(None, 0, None, C.byref(kept), None) == 0 and kept.value == 0
    for t, out in [(None, o), (p, None)]:
        assert lib.gp_cloud_sort_by_time_indices(t, 100, out, None) == 1
    assert lib.gp_cloud_sort_by_time_indices(p, -1, o, None) == 1 and lib.gp_cloud_sort_by_time_indices(None, 0, None, None) == 0

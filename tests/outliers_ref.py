"""f64 numpy restatement of find_inlier_points / remove_outliers (point_cloud_cpu_funcs.cpp:576-650), sort_by_time (:459-465) and filter / filter_by_index
(point_cloud_cpu.hpp:164-203), for tests/test_outliers_ref_cpu.py and tests/test_outliers_gpu.py.

THIS RESTATEMENT IS THE REFERENCE: point_cloud_cpu_funcs.cpp does not compile against the stand-in headers under oracle/ref_shim (tests/test_sampling_ref_cpu.py records
the same fact), so no output of the reference's own binary is recorded.  Every step cites the line it restates.

  neighbours   the k nearest points of the cloud itself (KdTree::knn_search over the cloud's own points, :619-629), the point itself among them at distance 0:
               scipy's cKDTree on the f32 coordinates cast to f64, or a brute-force search; or the caller's lists (the first overload, :576)
  d_i          sum_dist += (points[index] - pt).norm() for j = 0 .. k - 1, then / k (:582-588): a serial f64 sum in list order; the search returns its list in
               ascending distance, so the sum does not depend on which of several equidistant neighbours it kept
  statistics   sum_dists += d, sum_sq_dists += d * d serially (:591-596); mean = sum / n, var = sum_sq / n - mean^2 (one pass, not clamped), thresh = mean +
               sqrt(var) * std_thresh (:598-600)
  inliers      d_i < thresh, strict, ascending index (:605-609)

What the reference leaves undefined is defined as the device version defines it (include/gtsam_points_hip.h):
  short points a non-finite coordinate, fewer than k neighbours (n < k: the reference's lists keep their -1 and it reads points[-1]), a listed index outside
               [0, n), or a listed neighbour that is not finite: d_i = +inf, left out of mean and var (the divisor is the number m of points that are not short),
               never an inlier, counted in num_short; m = 0 gives thresh = 0 and nothing kept.  With no short point the formulas are the reference's.
  sort_by_time stable (equal times in ascending index: one of std::sort's legal outcomes), -0.0 = +0.0, NaN times last in ascending index."""
import functools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SCANS = ("000000.bin", "000001.bin")
KS = (5, 10, 20)
STD_THRESHS = (1.0, 2.0)


def scan(name):
    return np.fromfile(os.path.join(GOLDEN, "kitti_00", name), dtype=np.float32).reshape(-1, 3)


def knn_indices(points32, k, brute=False):
    """(n, k) int64 lists in ascending distance, -1 where the cloud has fewer than k (finite) points; rows of non-finite points are all -1"""
    p = np.asarray(points32, np.float32).reshape(-1, 3).astype(np.float64)
    n = len(p)
    out = np.full((n, k), -1, np.int64)
    ok = np.isfinite(p).all(axis=1)
    good = np.flatnonzero(ok)
    if len(good) == 0:
        return out
    kk = min(k, len(good))
    if brute:
        d2 = ((p[good][:, None, :] - p[good][None, :, :]) ** 2).sum(axis=2)
        idx = np.argsort(d2, axis=1, kind="stable")[:, :kk]
    else:
        from scipy.spatial import cKDTree

        _, idx = cKDTree(p[good]).query(p[good], k=kk)
        idx = np.asarray(idx).reshape(len(good), kk)
    out[good, :kk] = good[idx]
    return out


def mean_neighbor_distances(points32, neighbors, k):
    """d[n] (f64, +inf for short points) and the short mask, from (n, k) or flat lists: the serial sum of :582-588"""
    p = np.asarray(points32, np.float32).reshape(-1, 3).astype(np.float64)
    n = len(p)
    nb = np.asarray(neighbors, np.int64).reshape(n, k)
    short = ~np.isfinite(p).all(axis=1) | ((nb < 0) | (nb >= n)).any(axis=1)
    total = np.zeros(n)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(k):  # list order
            q = p[np.clip(nb[:, j], 0, max(n - 1, 0))] if n else p
            diff = q - p
            total += np.sqrt(diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1] + diff[:, 2] * diff[:, 2])
        d = total / k
    short |= ~np.isfinite(d)
    d[short] = np.inf
    return d, short


def serial_sum(x):
    """x[0] + x[1] + ... in this order, in f64 (np.add.accumulate is strictly sequential)"""
    return float(np.add.accumulate(np.asarray(x, np.float64))[-1]) if len(x) else 0.0


def inlier_statistics(d, std_thresh):
    """(mean, var, thresh, m) of :591-600 over the entries that are not short"""
    fin = d[np.isfinite(d)]
    m = len(fin)
    if m == 0:
        return 0.0, 0.0, 0.0, 0
    mean = serial_sum(fin) / m
    var = serial_sum(fin * fin) / m - mean * mean
    with np.errstate(invalid="ignore"):
        thresh = mean + float(np.sqrt(np.float64(var))) * std_thresh
    return mean, var, thresh, m


def find_inlier_points(points32, k=10, std_thresh=1.0, neighbors=None, brute=False):
    points32 = np.asarray(points32, np.float32).reshape(-1, 3)
    nb = knn_indices(points32, k, brute=brute) if neighbors is None else neighbors
    d, short = mean_neighbor_distances(points32, nb, k)
    mean, var, thresh, m = inlier_statistics(d, std_thresh)
    with np.errstate(invalid="ignore"):
        inliers = np.flatnonzero(np.isfinite(d) & (d < thresh))
    return dict(indices=inliers, dists=d, mean=mean, var=var, thresh=thresh, m=m, num_short=int(short.sum()))


@functools.lru_cache(maxsize=None)
def scan_dists(name, k):
    """the mean distances of a golden scan, computed once per session and shared (read-only)"""
    pts = scan(name)
    d, short = mean_neighbor_distances(pts, knn_indices(pts, k), k)
    assert not short.any()
    d.setflags(write=False)
    return d


def scan_reference(name, k, std_thresh):
    d = scan_dists(name, k)
    mean, var, thresh, m = inlier_statistics(d, std_thresh)
    return dict(indices=np.flatnonzero(d < thresh), dists=d, mean=mean, var=var, thresh=thresh, m=m, num_short=0)


def time_sort_keys(times32):
    """uint32 keys monotone in the float order: -0 -> +0, every NaN the largest key"""
    t = np.ascontiguousarray(np.asarray(times32, np.float32).reshape(-1))
    bits = t.view(np.uint32).copy()
    bits[bits == np.uint32(0x80000000)] = 0
    neg = (bits & np.uint32(0x80000000)) != 0
    keys = np.where(neg, ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)
    keys[np.isnan(t)] = np.uint32(0xFFFFFFFF)
    return keys


def sort_by_time(times32):
    """the indices of :459-465 with the stable tie rule"""
    return np.argsort(time_sort_keys(times32), kind="stable")


def filter_indices(mask):
    return np.flatnonzero(np.asarray(mask).reshape(-1) != 0)

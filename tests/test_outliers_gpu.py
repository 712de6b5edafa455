"""find_inlier_points_gpu / remove_outliers_gpu / filter_gpu / sort_by_time_gpu on the device against tests/outliers_ref.py (the f64 numpy restatement of
point_cloud_cpu_funcs.cpp:459-465, 576-650 and point_cloud_cpu.hpp:164-203, which is the reference: see its docstring).

Bounds (derived, not measured; no point is exempt):
  mean distance  |d_gpu - d_ref| <= (k + 8) 2^-52 d_ref per point: k correctly rounded additions and one division (2^-53 each), k square roots and squared norms
                 within a few ulp on either side.
  statistics     |thresh_gpu - thresh_ref| <= 1e-9 thresh_ref, the same for the mean, 1e-8 var for the variance: n 2^-53 ~ 1.4e-11 per sum (the device adds in a tree,
                 the restatement serially), amplified by at most 1 + mean^2 / var ~ 3 in the one-pass variance.  Loose, not tuned.
  inlier set     exact, against the restatement's set AND against {i : d_gpu[i] < thresh_gpu} recomputed on the host; tests/test_outliers_ref_cpu.py asserts that no
                 point of the inputs used here lies within 1e-9 thresh of a threshold, so the two roundings cannot disagree about any point."""
import functools

import numpy as np
import pytest

import outliers_ref as orf
from test_sampling_gpu import ATTRS, make_frame, rows
from test_sampling_ref_cpu import scan_attrs

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def scan_frame_attrs(name):
    return scan_attrs(orf.scan(name), seed=11)


_FRAMES = {}


def scan_frame(gpu, name):
    """one upload of a golden scan with all five attributes, shared (read-only) by the tests"""
    if name not in _FRAMES:
        _FRAMES[name] = make_frame(gpu, scan_frame_attrs(name))
    return _FRAMES[name]


_TREES = {}


def scan_tree(gpu, name):
    if name not in _TREES:
        _TREES[name] = gpu.KdTreeGPU(scan_frame(gpu, name))
    return _TREES[name]


def points_frame(gpu, pts, with_attrs=False):
    pts = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 3)
    if with_attrs:
        return make_frame(gpu, scan_attrs(pts, seed=5)), scan_attrs(pts, seed=5)
    return make_frame(gpu, {"points": pts}, names=("points",))


def check_against(out, ref, k, what):
    """a remove_outliers_gpu result against a restatement dict: distances to the derived bound, statistics, the exact set; returns the worst distance error in units of
    the bound"""
    d = out.mean_dists_gpu.cpu().numpy()
    idx = out.inlier_indices_gpu.cpu().numpy()
    assert d.dtype == np.float64 and idx.dtype == np.int32 and d.shape == ref["dists"].shape
    fin = np.isfinite(ref["dists"])
    assert np.array_equal(np.isfinite(d), fin) and (d[~fin] == np.inf).all(), what
    err = np.abs(d[fin] - ref["dists"][fin])
    bound = (k + 8) * 2.0 ** -52 * ref["dists"][fin]
    worst = float((err / np.maximum(bound, 1e-300)).max()) if fin.any() else 0.0
    print(f"{what}: worst |d_gpu - d_ref| = {worst:.3f} of the bound (k + 8) 2^-52 d")
    assert (err <= bound).all(), (what, worst)
    assert out.num_short == ref["num_short"], what
    if np.isfinite(ref["thresh"]):
        assert abs(out.dist_thresh - ref["thresh"]) <= 1e-9 * abs(ref["thresh"]), (what, out.dist_thresh, ref["thresh"])
        assert abs(out.dist_mean - ref["mean"]) <= 1e-9 * abs(ref["mean"]), what
        assert abs(out.dist_var - ref["var"]) <= 1e-8 * abs(ref["var"]) + 1e-300, (what, out.dist_var, ref["var"])
    with np.errstate(invalid="ignore"):
        own = np.flatnonzero(np.isfinite(d) & (d < out.dist_thresh))
    assert np.array_equal(idx, own), what
    assert np.array_equal(idx, ref["indices"]), (what, len(idx), len(ref["indices"]))
    assert (np.diff(idx) > 0).all() and out.size() == len(idx)
    return worst


@pytest.mark.parametrize("k", orf.KS)
def test_mean_distances_thresholds_and_inlier_sets_on_the_scans(gpu, k):
    """items 1 - 3 of the issue: both golden scans, std_thresh in {1, 2}; every attribute of the result equals sample_gpu(frame, ref_indices) byte for byte"""
    for name in orf.SCANS:
        frame = scan_frame(gpu, name)
        attrs = scan_frame_attrs(name)
        gen = frame.generation
        for std in orf.STD_THRESHS:
            ref = orf.scan_reference(name, k, std)
            out = gpu.remove_outliers_gpu(frame, k=k, std_thresh=std, tree=scan_tree(gpu, name))
            check_against(out, ref, k, f"{name} k = {k} std_thresh = {std} ({len(ref['indices'])} of {len(ref['dists'])} kept)")
            assert frame.generation == gen and frame.size() == len(ref["dists"])  # the input is untouched
            got, want = rows(out), rows(gpu.sample_gpu(frame, ref["indices"]))
            assert sorted(got) == sorted(ATTRS)
            for a in ATTRS:
                assert got[a].tobytes() == want[a].tobytes() == attrs[a][ref["indices"]].tobytes(), (name, a)
            if std == 1.0:
                assert np.array_equal(gpu.find_inlier_points_gpu(frame, k=k, std_thresh=std, tree=scan_tree(gpu, name)).cpu().numpy(), ref["indices"])
    if k == 10:
        assert len(orf.scan_reference(orf.SCANS[0], 10, 1.0)["indices"]) == 115_152 and len(orf.scan_reference(orf.SCANS[1], 10, 1.0)["indices"]) == 115_308


@pytest.mark.parametrize("k", orf.KS)
def test_both_overloads_and_every_grid_agree_to_the_bit(gpu, k):
    """item 4: KdTreeGPU.knn_search's lists as `neighbors` give the same mean_dists_gpu bytes and the same indices as the fused path; a shared tree, the call's own
    grid and a tree with another cell size give the same bytes (the search is exact: the cell size must not show)"""
    name = orf.SCANS[0]
    frame = scan_frame(gpu, name)
    fused = gpu.remove_outliers_gpu(frame, k=k, tree=scan_tree(gpu, name))
    d = fused.mean_dists_gpu.cpu().numpy().tobytes()
    idx = fused.inlier_indices_gpu.cpu().numpy().tobytes()
    nb, _, found = scan_tree(gpu, name).knn_search(orf.scan(name), k)
    assert (found == k).all()
    for neighbors in (nb, nb.reshape(-1)):
        two = gpu.remove_outliers_gpu(frame, k=k, neighbors=neighbors)
        assert two.mean_dists_gpu.cpu().numpy().tobytes() == d and two.inlier_indices_gpu.cpu().numpy().tobytes() == idx
        assert (two.dist_thresh, two.dist_mean, two.dist_var, two.num_short) == (fused.dist_thresh, fused.dist_mean, fused.dist_var, 0)
    own = gpu.remove_outliers_gpu(frame, k=k)
    coarse = gpu.remove_outliers_gpu(frame, k=k, tree=gpu.KdTreeGPU(frame, cell_size=1.0))
    for other in (own, coarse):
        assert other.mean_dists_gpu.cpu().numpy().tobytes() == d and other.inlier_indices_gpu.cpu().numpy().tobytes() == idx and other.dist_thresh == fused.dist_thresh
    with pytest.raises(gpu.GPError, match="not built over"):
        gpu.remove_outliers_gpu(frame, k=k, tree=scan_tree(gpu, orf.SCANS[1]))
    with pytest.raises(ValueError):
        gpu.remove_outliers_gpu(frame, k=k, neighbors=nb[:-1])


def test_two_runs_give_identical_bytes(gpu):
    name = orf.SCANS[1]
    frame = scan_frame(gpu, name)
    a = gpu.remove_outliers_gpu(frame, tree=scan_tree(gpu, name))
    b = gpu.remove_outliers_gpu(frame, tree=scan_tree(gpu, name))
    assert a.mean_dists_gpu.cpu().numpy().tobytes() == b.mean_dists_gpu.cpu().numpy().tobytes()
    assert a.inlier_indices_gpu.cpu().numpy().tobytes() == b.inlier_indices_gpu.cpu().numpy().tobytes()
    assert (a.dist_thresh, a.dist_mean, a.dist_var) == (b.dist_thresh, b.dist_mean, b.dist_var)


def test_smallest_shapes(gpu):
    """item 6, each case against the restatement"""
    rng = np.random.default_rng(21)
    out = gpu.remove_outliers_gpu(points_frame(gpu, np.zeros((0, 3))), k=10)
    assert out.size() == 0 and out.num_short == 0 and (out.dist_mean, out.dist_var, out.dist_thresh) == (0.0, 0.0, 0.0) and out.mean_dists_gpu.shape == (0,)
    assert out.points_gpu.shape == (0, 3) and gpu.find_inlier_points_gpu(points_frame(gpu, np.zeros((0, 3)))).shape == (0,)
    one = np.float32([[1.0, 2.0, 3.0]])
    out = gpu.remove_outliers_gpu(points_frame(gpu, one), k=1)  # d = 0, thresh = 0: nothing is below it, as in the reference
    check_against(out, orf.find_inlier_points(one, 1, 1.0), 1, "n = 1, k = 1")
    assert out.size() == 0 and out.dist_thresh == 0.0 and out.mean_dists_gpu.cpu().numpy().tolist() == [0.0]
    nine = rng.normal(size=(9, 3)).astype(np.float32)
    out = gpu.remove_outliers_gpu(points_frame(gpu, nine), k=10)  # n < k: every point is short
    check_against(out, orf.find_inlier_points(nine, 10, 1.0), 10, "n = 9, k = 10")
    assert out.num_short == 9 and out.size() == 0 and out.dist_thresh == 0.0
    ten = rng.normal(size=(10, 3)).astype(np.float32)
    check_against(gpu.remove_outliers_gpu(points_frame(gpu, ten), k=10), orf.find_inlier_points(ten, 10, 1.0), 10, "n = k = 10")
    for n in (127, 128, 129, 255, 256, 257, 1025):  # lane, workgroup and tile edges of the search, the compaction and the reduction
        pts = (rng.normal(size=(n, 3)) * 2).astype(np.float32)
        frame, attrs = points_frame(gpu, pts, with_attrs=True)
        ref = orf.find_inlier_points(pts, 10, 1.0)
        out = gpu.remove_outliers_gpu(frame, k=10)
        check_against(out, ref, 10, f"n = {n}")
        got = rows(out)
        for a in ATTRS:
            assert got[a].tobytes() == attrs[a][ref["indices"]].tobytes(), (n, a)
        if n in (129, 1025):
            out1 = gpu.remove_outliers_gpu(frame, k=1)  # every d is 0: nothing is kept
            check_against(out1, orf.find_inlier_points(pts, 1, 1.0), 1, f"n = {n}, k = 1")
            assert out1.size() == 0 and (out1.mean_dists_gpu.cpu().numpy() == 0).all()
            check_against(gpu.remove_outliers_gpu(frame, k=32), orf.find_inlier_points(pts, 32, 1.0), 32, f"n = {n}, k = 32")
            for std in (0.0, -1.0):
                check_against(gpu.remove_outliers_gpu(frame, k=10, std_thresh=std), orf.find_inlier_points(pts, 10, std), 10, f"n = {n}, std_thresh = {std}")
    dup = np.concatenate([np.tile(np.float32([[1.5, -2.0, 0.25]]), (64, 1)), (rng.normal(size=(64, 3)) * 4).astype(np.float32)])
    out = gpu.remove_outliers_gpu(points_frame(gpu, dup), k=10)  # the copies: d = 0 whichever of the 63 twins the search lists
    check_against(out, orf.find_inlier_points(dup, 10, 1.0), 10, "64 copies + 64 points")
    assert (out.mean_dists_gpu.cpu().numpy()[:64] == 0).all()
    bad = (rng.normal(size=(300, 3)) * 2).astype(np.float32)
    bad[17, 1], bad[211, 2] = np.nan, np.inf
    out = gpu.remove_outliers_gpu(points_frame(gpu, bad), k=10)  # short, out of the statistics (taken over the other 298), out of the result
    check_against(out, orf.find_inlier_points(bad, 10, 1.0), 10, "NaN + inf in 300 points")
    idx = out.inlier_indices_gpu.cpu().numpy()
    assert out.num_short == 2 and 17 not in idx and 211 not in idx and np.isfinite(out.points_gpu.cpu().numpy()).all()
    pts = (rng.normal(size=(500, 3)) * 2).astype(np.float32)
    nb = orf.knn_indices(pts, 10).astype(np.int32)
    nb[3, 9], nb[400, 0] = -1, 500  # never dereferenced: those two points are short
    out = gpu.remove_outliers_gpu(points_frame(gpu, pts), k=10, neighbors=nb)
    check_against(out, orf.find_inlier_points(pts, 10, 1.0, neighbors=nb), 10, "neighbors with -1 and n")
    assert out.num_short == 2 and np.isinf(out.mean_dists_gpu.cpu().numpy()[[3, 400]]).all()
    big_k = orf.knn_indices(pts, 40)  # caller-supplied lists have no upper bound on k
    check_against(gpu.remove_outliers_gpu(points_frame(gpu, pts), k=40, neighbors=big_k), orf.find_inlier_points(pts, 40, 1.0, neighbors=big_k), 40, "neighbors, k = 40")


def test_refusals_run_nothing(gpu):
    frame = points_frame(gpu, np.random.default_rng(3).normal(size=(100, 3)))
    for kwargs in (dict(k=0), dict(k=33), dict(k=-1), dict(std_thresh=float("nan")), dict(std_thresh=float("inf")), dict(k=0, neighbors=np.zeros((100, 0), np.int32))):
        with pytest.raises(gpu.GPError):
            gpu.remove_outliers_gpu(frame, **kwargs)
        with pytest.raises(gpu.GPError):
            gpu.find_inlier_points_gpu(frame, **kwargs)


@pytest.mark.parametrize("n", [1, 15, 16, 256, 257, 16_384, 16_385, 100_003])  # (15 / 16: a scan thread's sixteen elements, one short of them; 16 384 / 16 385: one scan tile, one past it)
def test_filter_keeps_the_masked_rows(gpu, n):
    import torch

    rng = np.random.default_rng(n)
    pts = rng.normal(size=(n, 3)).astype(np.float32)
    attrs = scan_attrs(pts, seed=6)
    frame = make_frame(gpu, attrs)
    gen = frame.generation
    masks = {"none": np.zeros(n, bool), "all": np.ones(n, bool), "alternating": np.arange(n) % 2 == 0, "first": np.arange(n) == 0, "last": np.arange(n) == n - 1,
             "random": rng.integers(0, 2, size=n).astype(bool)}
    for what, mask in masks.items():
        forms = [mask, mask.astype(np.uint8), torch.from_numpy(mask), torch.from_numpy(mask.astype(np.uint8) * 255).to("cuda:0")] if what in ("alternating", "random") else [mask]
        for form in forms:
            out = gpu.filter_gpu(frame, form)
            assert np.array_equal(out.sample_indices_gpu.cpu().numpy(), orf.filter_indices(mask)) and out.size() == int(mask.sum()), (n, what)
            got = rows(out)
            for a in ATTRS:
                assert got[a].tobytes() == attrs[a][mask].tobytes(), (n, what, a)
    on_device = gpu.filter_gpu(frame, frame.points_gpu[:, 2] > 0.25)  # a predicate evaluated with torch on the device
    assert on_device.points_gpu.cpu().numpy().tobytes() == pts[pts[:, 2] > 0.25].tobytes()
    for wrong in (np.ones(n + 1, bool), np.ones(n - 1, bool), torch.ones(2 * n, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            gpu.filter_gpu(frame, wrong)
    with pytest.raises(ValueError):
        gpu.filter_gpu(frame, np.ones(n, np.float32))
    assert frame.generation == gen
    if n == 1:
        empty = gpu.filter_gpu(points_frame(gpu, np.zeros((0, 3))), np.zeros(0, bool))
        assert empty.size() == 0 and empty.sample_indices_gpu.shape == (0,)


def times_case(n, seed):
    rng = np.random.default_rng(seed)
    vals = np.concatenate([rng.normal(size=986).astype(np.float32) * 10, np.float32([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 2.0 ** -126, np.inf, -np.inf, -3.5, 3.5, 1e38, -1e38, 7.0])])
    assert len(vals) == 1000
    t = vals[rng.integers(0, 1000, size=n)]
    if n >= 257:
        t[[5, n // 2, n - 1]] = np.nan
        t[[10, 11, 12, 13]] = np.float32([-0.0, 0.0, -0.0, 0.0])
    return t


@pytest.mark.parametrize("n", [0, 1, 2, 257, 124_668])
def test_sort_by_time(gpu, n):
    pts = orf.scan(orf.SCANS[0])[:n] if n else np.zeros((0, 3), np.float32)
    attrs = scan_attrs(pts, seed=8)
    t = times_case(n, seed=n)
    cases = {"ties": t}
    if n >= 2:
        finite_sorted = np.sort(t[~np.isnan(t)])
        cases["sorted"] = finite_sorted
        cases["reversed"] = finite_sorted[::-1].copy()
        if n == 2:
            cases["equal"] = np.float32([0.0, -0.0])
    for what, times in cases.items():
        m = len(times)
        a = {k: v[:m] for k, v in attrs.items()}
        a["times"] = times.reshape(m, 1)
        frame = make_frame(gpu, a)
        gen = frame.generation
        out = gpu.sort_by_time_gpu(frame)
        want = orf.sort_by_time(times)
        idx = out.sample_indices_gpu.cpu().numpy()
        assert idx.dtype == np.int32 and np.array_equal(idx, want), (n, what)
        got = rows(out)
        for name in ATTRS:
            assert got[name].tobytes() == a[name][want].tobytes(), (n, what, name)
        s = got["times"].reshape(-1)
        nans = int(np.isnan(times).sum())
        assert np.isnan(s[m - nans:]).all() and (s[1 : m - nans] >= s[: max(m - nans - 1, 0)]).all() and frame.generation == gen
        if what == "sorted":
            assert np.array_equal(idx, np.arange(m))  # already sorted, ties included: the identity (stable)
    with pytest.raises(gpu.GPError):
        gpu.sort_by_time_gpu(make_frame(gpu, attrs, names=("points", "covs")))


@pytest.mark.parametrize("n", [257, 5000])  # (5000: more than one sort tile)
def test_a_faulted_time_sort_is_run_again_with_one_class(gpu, n):
    """the retry rule the time sort shares with the plan build (gp_sort.hpp, with_sort_fallback): the hook makes tile 0 of the first sort raise the fault word, the host
    sorts again with one ticket class, the result is the same and the hooks' counter rises by exactly one"""
    lib = gpu.load()
    times = times_case(n, seed=n)
    frame = make_frame(gpu, {"points": np.zeros((n, 3), np.float32), "times": times.reshape(n, 1)}, names=("points", "times"))
    before = lib.gp_debug_voxelgrid_hooks(0, 1)
    try:
        idx = gpu.sort_by_time_gpu(frame).sample_indices_gpu.cpu().numpy()
    finally:
        after = lib.gp_debug_voxelgrid_hooks(0, 0)
    assert np.array_equal(idx, orf.sort_by_time(times)) and after == before + 1

"""estimate_pose_ransac_gpu and the weighted alignments at their edges, against tests/ransac_ref.py.  Inputs: rr.make_small_case (at most 512 target points, 256 source
points, D = 8) and tests/registration_edges.py, held to their conditions by tests/test_ransac_edges_ref_cpu.py.  The per-iteration comparison is compare() of
tests/test_ransac_gpu.py with the bounds derived there (exact samples, matches and status; rr.rotation_bound; translation = that bound x |mean_s| + 1e-12 x extent;
inliers exact at the device's own pose up to the points within 1e-10 of a cell face).

For samples rr.rotation_bound calls unconditioned (the rotation is not determined by the sample) the device's pose is held to being a rigid pose that is a MINIMISER:
  sum |T s - t|^2 at the device's pose <= the same sum at the restatement's SVD pose + 1e-12 x extent^2
both minimise the same sum, the margin is the f64 rounding of forming it (a few 2^-53 x extent^2 per term).

Not reachable: GP_RANSAC_SAMPLE_FAILED needs more than 64 redraws in one iteration, about (2/3)^64 = 5e-12 per iteration even at N_s = 3; there is no test hook for
it, the redraw loop is covered through rr.draw_samples on the three-point cloud of tests/test_ransac_gpu.py.
Not distinguishable: `<` for `<=` in the zero-feature rule -- no f32 value widens to exactly 1e-3; what the boundary rows tell apart is f64 from f32 arithmetic in
that rule (float32(1e-3) is above 1e-3 in f64 and equal to it in f32)."""
import ctypes as C

import numpy as np
import pytest

import ransac_ref as rr
import registration_edges as re_
from test_ransac_gpu import compare

pytestmark = pytest.mark.gpu

_DEVICE = {}
KEYS = ("status", "source_indices", "target_indices", "poses", "inliers")


def device_case(gpu, dof, far=0.0):
    import torch

    if (dof, far) not in _DEVICE:
        c = rr.make_small_case(dof, far)
        _DEVICE[dof, far] = (gpu.PointCloudGPU(c["target"]), gpu.PointCloudGPU(c["source"]), torch.from_numpy(c["target_features"]).cuda(), torch.from_numpy(c["source_features"]).cuda())
    return _DEVICE[dof, far]


def arrays(hyp):
    dev = {k: getattr(hyp, k).cpu().numpy() for k in KEYS}
    dev["poses"] = dev["poses"].reshape(-1, 4, 4).transpose(0, 2, 1)
    return dev


def run(gpu, dof, far=0.0, source_features=None, **kw):
    sample_indices = kw.pop("sample_indices", None)
    t, s, tf, sf = device_case(gpu, dof, far)
    kw.setdefault("max_iterations", re_.EDGE_ITERATIONS)
    p = gpu.RANSACParams(dof=dof, **kw)
    res, hyp = gpu.estimate_pose_ransac_gpu(t, s, tf, sf if source_features is None else source_features, p, sample_indices=sample_indices, return_hypotheses=True)
    return res, arrays(hyp), p


def same_result(a, b):
    return (a.best_iteration, a.best_inliers, a.inlier_rate, a.num_scored, a.early_stopped) == (b.best_iteration, b.best_inliers, b.inlier_rate, b.num_scored, b.early_stopped) and \
        a.T_target_source.tobytes() == b.T_target_source.tobytes()


@pytest.mark.parametrize("dof", [6, 4])
def test_chunk_geometry(gpu, dof):
    """chunk_iterations of 1, not dividing max_iterations, equal to it and larger: the same arrays and result when nothing stops early"""
    case = rr.make_small_case(dof)
    runs = []
    for chunk in re_.CHUNKS:
        res, dev, p = run(gpu, dof, chunk_iterations=chunk, early_stop_inlier_rate=re_.NEVER_STOP)
        _, status = compare(dof, res, dev, p, case=case)
        assert not (status == rr.SKIPPED).any() and not res.early_stopped and res.num_scored == int((status == rr.SCORED).sum())
        runs.append((res, dev))
    for res, dev in runs[1:]:
        assert same_result(res, runs[0][0])
        for k in KEYS:
            assert dev[k].tobytes() == runs[0][1][k].tobytes(), k


def test_a_stop_inside_the_first_chunk(gpu):
    case = rr.make_small_case(6)
    res, dev, p = run(gpu, 6, chunk_iterations=7, early_stop_inlier_rate=0.3)
    _, status = compare(6, res, dev, p, case=case)
    assert (status[7:] == rr.SKIPPED).all() and (status[:7] != rr.SKIPPED).all() and res.early_stopped
    assert res.num_scored == int((status[:7] == rr.SCORED).sum()) > 0 and res.best_iteration < 7
    assert (dev["source_indices"][7:] == -1).all() and (dev["poses"][7:] == 0).all() and (dev["inliers"][7:] == -1).all()


def test_equality_is_not_a_stop(gpu):
    """early_stop_inlier_rate = best / N_s with N_s = 256: N_s x rate == best exactly and the rule is strictly greater; one representable step lower it is a stop"""
    case = rr.make_small_case(6)
    res0, dev0, _ = run(gpu, 6, chunk_iterations=7, early_stop_inlier_rate=re_.NEVER_STOP)
    best, ns = res0.best_inliers, len(case["source"])
    rate = best / float(ns)
    assert ns == 256 and ns * rate == best and res0.best_iteration < re_.EDGE_ITERATIONS - 7
    res, dev, p = run(gpu, 6, chunk_iterations=7, early_stop_inlier_rate=rate)
    _, status = compare(6, res, dev, p, case=case)
    assert not res.early_stopped and not (status == rr.SKIPPED).any() and same_result(res, res0)
    res, dev, p = run(gpu, 6, chunk_iterations=7, early_stop_inlier_rate=float(np.nextafter(rate, 0.0)))
    _, status = compare(6, res, dev, p, case=case)
    behind = (res0.best_iteration // 7 + 1) * 7
    assert res.early_stopped and (status[behind:] == rr.SKIPPED).all() and (status[:behind] != rr.SKIPPED).all() and res.best_iteration == res0.best_iteration


def nothing_scored(res):
    assert np.array_equal(res.T_target_source, np.eye(4)) and res.best_iteration == -1 and res.best_inliers == 0 and res.inlier_rate == 0.0
    assert res.num_scored == 0 and res.early_stopped is False


@pytest.mark.parametrize("dof", [6, 4])
def test_no_scored_hypothesis(gpu, dof):
    import torch

    c = rr.make_small_case(dof)
    samples = 3 if dof == 6 else 2
    want_src = np.array([rr.draw_samples(5489, it, 256, samples) + [-1] * (3 - samples) for it in range(re_.EDGE_ITERATIONS)], np.int32)
    # every source feature 2^-10 <= 1e-3: INVALID_FEATURE, the sample drawn, nothing matched or aligned
    res, dev, p = run(gpu, dof, source_features=torch.full((256, 8), 2.0 ** -10, dtype=torch.float32, device="cuda"))
    nothing_scored(res)
    assert (dev["status"] == rr.INVALID_FEATURE).all() and np.array_equal(dev["source_indices"], want_src)
    assert (dev["target_indices"] == -1).all() and (dev["poses"] == 0).all() and (dev["inliers"] == -1).all()
    # poly_error_thresh = 0 on f32-rounded data: POLY_REJECTED wherever the features were valid; matched, not aligned
    res, dev, p = run(gpu, dof, poly_error_thresh=0.0)
    ref = rr.hypotheses(c["target"], c["source"], c["target_features"], c["source_features"], re_.EDGE_ITERATIONS, dof=dof, poly_error_thresh=0.0)
    nothing_scored(res)
    assert np.array_equal(dev["status"], ref["status"]) and np.isin(dev["status"], (rr.POLY_REJECTED, rr.INVALID_FEATURE)).all() and (dev["status"] == rr.POLY_REJECTED).sum() > 20
    assert np.array_equal(dev["source_indices"], ref["source_indices"]) and np.array_equal(dev["target_indices"], ref["target_indices"])
    assert (dev["poses"] == 0).all() and (dev["inliers"] == -1).all()
    # every aligned hypothesis' own pose on the taboo list: TABOO, aligned (the pose is there), not scored
    res1, dev1, _ = run(gpu, dof, early_stop_inlier_rate=re_.NEVER_STOP)
    own = [dev1["poses"][it] for it in np.flatnonzero(dev1["status"] == rr.SCORED)]
    assert 1 <= len(own) <= 64 and res1.num_scored == len(own)
    res, dev, p = run(gpu, dof, early_stop_inlier_rate=re_.NEVER_STOP, taboo_list=own)
    nothing_scored(res)
    assert np.array_equal(dev["status"], np.where(dev1["status"] == rr.SCORED, rr.TABOO, dev1["status"]))
    for k in ("source_indices", "target_indices", "poses"):
        assert dev[k].tobytes() == dev1[k].tobytes(), k
    assert (dev["inliers"] == -1).all()


@pytest.mark.parametrize("dof", [6, 4])
def test_feature_boundary_rows_and_the_nan_row(gpu, dof):
    case = rr.make_small_case(dof)
    given = re_.boundary_samples(dof)
    samples = 3 if dof == 6 else 2
    res, dev, p = run(gpu, dof, max_iterations=len(given), sample_indices=given, early_stop_inlier_rate=re_.NEVER_STOP)
    compare(dof, res, dev, p, sample_indices=given, case=case)
    s = dev["status"]
    assert (s[0:4] != rr.INVALID_FEATURE).all() and (s[4:8] == rr.INVALID_FEATURE).all() and (s[8:12] != rr.INVALID_FEATURE).all() and (s[12:16] == rr.INVALID_FEATURE).all()
    for it in range(8, 12):
        assert dev["target_indices"][it, it % samples] == 0  # the NaN row has no match: target 0


def test_taboo_list_of_64_with_only_the_last_matching(gpu):
    case = rr.make_small_case(6)
    res1, dev1, _ = run(gpu, 6, early_stop_inlier_rate=re_.NEVER_STOP)
    taboo = re_.decoy_poses(63) + [res1.T_target_source]
    res, dev, p = run(gpu, 6, early_stop_inlier_rate=re_.NEVER_STOP, taboo_list=taboo)
    _, status = compare(6, res, dev, p, case=case)
    assert status[res1.best_iteration] == rr.TABOO and (status == rr.SCORED).any()
    res63, dev63, _ = run(gpu, 6, early_stop_inlier_rate=re_.NEVER_STOP, taboo_list=taboo[:63])
    assert not (dev63["status"] == rr.TABOO).any() and same_result(res63, res1)
    with pytest.raises(gpu.GPError):
        run(gpu, 6, taboo_list=re_.decoy_poses(64) + [res1.T_target_source])


@pytest.mark.parametrize("dof", [6, 4])
def test_clouds_1e5_m_from_the_origin(gpu, dof):
    case = rr.make_small_case(dof, 1e5)
    res, dev, p = run(gpu, dof, far=1e5, early_stop_inlier_rate=re_.NEVER_STOP)
    _, status = compare(dof, res, dev, p, case=case)
    angle, trans = rr.taboo_delta(res.T_target_source, case["T_true"])
    assert angle < 1e-3 and res.best_inliers > 0.9 * 256, (angle, trans)  # (f32 points at 1e5 m are rounded to 1 / 128 m; the translation's lever arm is 1.4e5 m)


def test_null_array_pointers_through_the_c_abi(gpu):
    """gp_ransac_hypotheses with only status and inliers set: the library keeps the other three arrays itself; the result and the two arrays are the all-arrays run's"""
    import torch

    t, s, tf, sf = device_case(gpu, 6)
    res0, dev0, p0 = run(gpu, 6, chunk_iterations=7, early_stop_inlier_rate=re_.NEVER_STOP)
    H = re_.EDGE_ITERATIONS
    lib = gpu._capi.load()
    params = gpu._capi.RansacParams(H, 6, 7, 0, re_.NEVER_STOP, p0.poly_error_thresh, p0.inlier_voxel_resolution, p0.taboo_thresh_rot, p0.taboo_thresh_trans, p0.seed, None)
    ptr = lambda x: C.c_void_p(x.data_ptr())
    for with_arrays in (True, False):
        status = torch.full((H,), -7, dtype=torch.int32, device="cuda")
        inliers = torch.full((H,), -7, dtype=torch.int32, device="cuda")
        hyp = gpu._capi.RansacHypotheses(status.data_ptr(), None, None, None, inliers.data_ptr())
        res = gpu._capi.RansacResult()
        torch.cuda.synchronize()
        gpu._capi.check(lib.gp_ransac_estimate_pose(ptr(t.points_gpu), t.size(), ptr(s.points_gpu), s.size(), ptr(tf), ptr(sf), 8, C.byref(params), None,
                                                    C.byref(hyp) if with_arrays else None, C.byref(res), None), "gp_ransac_estimate_pose")
        T = np.array(list(res.T_target_source), np.float64).reshape(4, 4).T
        assert T.tobytes() == res0.T_target_source.tobytes() and res.inlier_rate == res0.inlier_rate
        assert (res.best_inliers, res.best_iteration, res.num_scored, bool(res.early_stopped)) == (res0.best_inliers, res0.best_iteration, res0.num_scored, False)
        if with_arrays:
            assert np.array_equal(status.cpu().numpy(), dev0["status"]) and np.array_equal(inliers.cpu().numpy(), dev0["inliers"])


def test_degenerate_samples(gpu):
    c = re_.degenerate_cloud()
    src, tgt = c["source"].astype(np.float64), c["target"].astype(np.float64)
    extent = float(max(np.abs(src).max(), np.abs(tgt).max()))
    grid = rr.OccupancySet(1.0).insert(c["target"])
    tc, sc = gpu.PointCloudGPU(c["target"]), gpu.PointCloudGPU(c["source"])
    for dof in (6, 4):
        cases = [(sample, what) for d, sample, what in re_.DEGENERATE_SAMPLES if d == dof]
        k = 3 if dof == 6 else 2
        given = np.array([s for s, _ in cases], np.int32)
        p = gpu.RANSACParams(dof=dof, max_iterations=len(cases), early_stop_inlier_rate=2.0)
        res, hyp = gpu.estimate_pose_ransac_gpu(tc, sc, c["target_features"], c["source_features"], p, sample_indices=given, return_hypotheses=True)
        dev = arrays(hyp)
        assert (dev["status"] == rr.SCORED).all() and np.array_equal(dev["source_indices"], given) and np.array_equal(dev["target_indices"], given)
        for it, (sample, what) in enumerate(cases):
            s, t = src[list(sample[:k])], tgt[list(sample[:k])]
            H, mt, ms = rr.cross_covariance(t, s)
            assert not rr.rotation_bound(H, dof)[0], what
            P = dev["poses"][it]
            R = P[:3, :3]
            assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and np.linalg.det(R) > 0.0 and np.array_equal(P[3], [0, 0, 0, 1]), what
            if dof == 4:
                assert np.array_equal(R[2], [0, 0, 1]) and np.array_equal(R[:, 2], [0, 0, 1]), what
            want = rr.alignment_residual(rr.pose_from(H, mt, ms, dof), s, t)
            got = rr.alignment_residual(P, s, t)
            print(f"dof {dof} {what}: residual {got:.3e} against the SVD pose's {want:.3e} + {1e-12 * extent ** 2:.3e}")
            assert got <= want + 1e-12 * extent ** 2, what
            if (H == 0).all() or (dof == 4 and (H[:2, :2] == 0).all()):
                assert np.array_equal(R, np.eye(3)) and np.array_equal(P[:3, 3], mt - ms), what  # identity rotation, t = mean_t - mean_s
            count, band = grid.calc_overlap(c["source"], P), rr.band_count(c["source"], P, 1.0)
            assert abs(int(dev["inliers"][it]) - count) <= band, what
        first = int(np.argmax(dev["inliers"]))
        assert res.best_iteration == first and res.best_inliers == dev["inliers"][first] and res.num_scored == len(cases) and not res.early_stopped


def align_fns(gpu, dof):
    return (gpu.align_points_se3_gpu, rr.align_points_se3) if dof == 6 else (gpu.align_points_4dof_gpu, rr.align_points_4dof)


@pytest.mark.parametrize("n", re_.ALIGN_SIZES)
@pytest.mark.parametrize("dof", [6, 4])
def test_alignment_at_the_workgroup_edges_with_zero_weights(gpu, dof, n):
    """the device on all n points, a third of them under weight 0, against the restatement on the others alone: bound + n 2^-52 as in test_weighted_alignment_alone
    (the translation: that x the 20 m the points span, + 1e-12 x 20)"""
    fn, ref_fn = align_fns(gpu, dof)
    t, s, w = re_.align_case(dof, n)
    keep = w != 0
    got, want = fn(t, s, w), ref_fn(t[keep], s[keep], w[keep])
    H, _, _ = rr.cross_covariance(t[keep], s[keep], w[keep])
    ok, bound = rr.rotation_bound(H, dof)
    R = got[:3, :3]
    assert ok and np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and np.linalg.det(R) > 0.0 and np.array_equal(got[3], [0, 0, 0, 1])
    err = np.linalg.norm(R - want[:3, :3])
    print(f"dof {dof} n {n}: rotation difference = {err / (bound + n * 2.0 ** -52):.3f} of the bound")
    assert err <= bound + n * 2.0 ** -52
    assert np.abs(got[:3, 3] - want[:3, 3]).max() <= (bound + n * 2.0 ** -52) * 20 + 1e-12 * 20


@pytest.mark.parametrize("dof", [6, 4])
def test_alignment_of_degenerate_point_sets(gpu, dof):
    fn, _ = align_fns(gpu, dof)
    for n in (1, 256, 257):
        s = np.tile([1.5, -2.25, 0.5], (n, 1))  # all points identical: H = 0 exactly (every x - mean is 0: the mean of n equal dyadic numbers is exact)
        t = np.tile([4.0, 0.75, -1.5], (n, 1))
        w = np.full(n, 0.5)
        got = fn(t, s, w)
        assert np.array_equal(got[:3, :3], np.eye(3)) and np.array_equal(got[:3, 3], [2.5, 3.0, -2.0]) and np.array_equal(got[3], [0, 0, 0, 1]), n
    if dof == 4:  # the points differ in z only: the 2x2 block of H vanishes
        z = np.arange(300.0) * 0.25
        s = np.stack([np.full(300, 1.5), np.full(300, -2.25), z], axis=1)
        t = np.stack([np.full(300, 4.0), np.full(300, 0.75), 2.0 - z], axis=1)
        got = fn(t, s, np.ones(300))
        assert np.array_equal(got[:3, :3], np.eye(3)) and np.array_equal(got[:2, 3], [2.5, 3.0])

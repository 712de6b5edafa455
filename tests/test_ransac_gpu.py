"""estimate_pose_ransac_gpu against tests/ransac_ref.py (the f64 numpy restatement of the reference's RANSAC; see its docstring), on the per-iteration arrays.

Inputs: rr.make_case -- a golden scan cut to at most 4096 points, the source 2048 of them moved by a known pose and rounded to f32, synthetic D = 33 descriptors with
~60 % true matches and 41 all-zero rows.  tests/test_ransac_ref_cpu.py holds these inputs to the conditions the exact comparisons rest on (no polygon error within
1e-12 of the threshold, no pose within 1e-9 of a taboo threshold, no feature ties, conditioning, no point near a cell face).

Bounds (derived, not measured):
  samples, matches, status   exact
  rotation     dof 6: |R_gpu - R_ref|_F <= 1e-12 sigma1 / sigma2 of H where sigma2 / sigma1 >= 1e-6: the sensitivity of the rotation U diag(1, 1, +-1) V^T to rounding in
               H (a sample's H has rank 2; the two methods -- one-sided Jacobi on the device, LAPACK in the restatement -- each leave a few 2^-53 sigma1 / sigma2).
               dof 4: the rotation is atan2(h10 - h01, h00 + h11): <= 1e-12 |H2|_F / hypot(h00 + h11, h10 - h01) (rr.rotation_bound).  H itself is formed in the same
               operations on both sides.  Below the conditioning limit only orthonormality to 1e-12 and a positive determinant are required.
  translation  t = mean_t - R mean_s: the rotation bound x |mean_s| + 1e-12 x the clouds' extent
  inliers      exact, against the restatement's occupancy set evaluated at the device's own downloaded pose; a hypothesis with points within 1e-10 of a cell face
               (the CPU test allows 1 % of them) is allowed that many points of difference"""
import functools

import numpy as np
import pytest

import ransac_ref as rr

pytestmark = pytest.mark.gpu

_DEVICE = {}


def device_case(gpu, dof):
    import torch

    if dof not in _DEVICE:
        c = rr.make_case(dof)
        _DEVICE[dof] = (gpu.PointCloudGPU(c["target"]), gpu.PointCloudGPU(c["source"]), torch.from_numpy(c["target_features"]).cuda(), torch.from_numpy(c["source_features"]).cuda())
    return _DEVICE[dof]


@functools.lru_cache(maxsize=None)
def target_set(dof):
    return rr.OccupancySet(1.0).insert(rr.make_case(dof)["target"])


def run(gpu, dof, **kw):
    sample_indices = kw.pop("sample_indices", None)
    t, s, tf, sf = device_case(gpu, dof)
    p = gpu.RANSACParams(dof=dof, **kw)
    res, hyp = gpu.estimate_pose_ransac_gpu(t, s, tf, sf, p, sample_indices=sample_indices, return_hypotheses=True)
    dev = {k: getattr(hyp, k).cpu().numpy() for k in ("status", "source_indices", "target_indices", "poses", "inliers")}
    dev["poses"] = dev["poses"].reshape(-1, 4, 4).transpose(0, 2, 1)  # column-major rows -> (row, col)
    return res, dev, p


def compare(dof, res, dev, p, sample_indices=None, case=None):
    """the device's per-iteration arrays and result against the restatement run with the same parameters; returns the restatement's pre-skip hypotheses.
    case: another input than rr.make_case(dof) (tests/test_ransac_edges_gpu.py: rr.make_small_case), at inlier_voxel_resolution 1.0 like it"""
    c = rr.make_case(dof) if case is None else case
    H = p.max_iterations
    samples = 3 if dof == 6 else 2
    ref = rr.hypotheses(c["target"], c["source"], c["target_features"], c["source_features"], H, dof=dof, seed=p.seed, poly_error_thresh=p.poly_error_thresh,
                        taboo_list=tuple(p.taboo_list), taboo_thresh_rot=p.taboo_thresh_rot, taboo_thresh_trans=p.taboo_thresh_trans, sample_indices=sample_indices)
    grid = target_set(dof) if case is None else rr.OccupancySet(1.0).insert(c["target"])
    counts = np.full(H, -1, np.int64)
    band = np.zeros(H, np.int64)
    for it in np.flatnonzero(ref["status"] == rr.SCORED):
        T = dev["poses"][it] if dev["status"][it] == rr.SCORED else ref["poses"][it]  # (an iteration the device skipped has no device pose; it cannot matter any more)
        counts[it] = grid.calc_overlap(c["source"], T)
        band[it] = rr.band_count(c["source"], T, 1.0)
    status, best_it, best = rr.select(ref["status"], counts, p.chunk_iterations, len(c["source"]), p.early_stop_inlier_rate)
    assert np.array_equal(dev["status"], status), np.flatnonzero(dev["status"] != status)[:10]
    skipped = status == rr.SKIPPED
    want_src = np.where(skipped[:, None], -1, ref["source_indices"])
    assert np.array_equal(dev["source_indices"], want_src)
    tried = np.isin(status, (rr.SCORED, rr.TABOO, rr.POLY_REJECTED))
    assert np.array_equal(dev["target_indices"], np.where(tried[:, None], ref["target_indices"], -1))
    aligned = np.isin(status, (rr.SCORED, rr.TABOO))
    assert (dev["poses"][~aligned] == 0.0).all() and (dev["inliers"][status != rr.SCORED] == -1).all()
    extent = float(max(np.abs(c["target"]).max(), np.abs(c["source"]).max()))
    worst = 0.0
    for it in np.flatnonzero(aligned):
        T, Tr = dev["poses"][it], ref["poses"][it]
        R = T[:3, :3]
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and np.linalg.det(R) > 0.0 and np.array_equal(T[3], [0, 0, 0, 1]), it
        ok, bound = rr.rotation_bound(ref["H"][it], dof)
        if not ok:
            continue
        err = np.linalg.norm(R - Tr[:3, :3])
        worst = max(worst, err / bound)
        assert err <= bound, (it, err, bound)
        ms = c["source"][ref["source_indices"][it, :samples]].astype(np.float64).mean(axis=0)
        assert np.linalg.norm(T[:3, 3] - Tr[:3, 3]) <= bound * np.linalg.norm(ms) + 1e-12 * extent, it
    print(f"dof {dof}: worst rotation difference = {worst:.3f} of the bound")
    scored = np.flatnonzero(status == rr.SCORED)
    assert len(scored) > 0 and (np.abs(dev["inliers"][scored] - counts[scored]) <= band[scored]).all()
    # the result: the first argmax of the device's own counts among the scored hypotheses
    first = scored[np.argmax(dev["inliers"][scored])]
    assert res.best_iteration == first and res.best_inliers == dev["inliers"][first] and res.num_scored == len(scored)
    assert res.inlier_rate == dev["inliers"][first] / float(len(c["target"]))
    assert np.array_equal(res.T_target_source, dev["poses"][first])
    assert res.early_stopped == bool((dev["inliers"][scored] > len(c["source"]) * p.early_stop_inlier_rate).any())
    if (band[scored] == 0).all():
        assert res.best_iteration == best_it and res.best_inliers == best
    return ref, status


@pytest.mark.parametrize("dof", [6, 4])
def test_hypotheses_against_the_restatement(gpu, dof):
    res, dev, p = run(gpu, dof, max_iterations=rr.CASE_ITERATIONS)
    ref, status = compare(dof, res, dev, p)
    for s in (rr.SCORED, rr.INVALID_FEATURE, rr.POLY_REJECTED):
        assert (status == s).any(), s
    if dof == 4:
        assert (dev["source_indices"][:, 2] == -1).all() and (dev["target_indices"][:, 2] == -1).all()


@pytest.mark.parametrize("dof", [6, 4])
def test_pose_is_found_at_2000_iterations(gpu, dof):
    c = rr.make_case(dof)
    t, s, tf, sf = device_case(gpu, dof)
    res = gpu.estimate_pose_ransac_gpu(t, s, tf, sf, gpu.RANSACParams(dof=dof, max_iterations=2000))
    angle, trans = rr.taboo_delta(res.T_target_source, c["T_true"])
    assert angle < 0.5 * np.pi / 180.0 and trans < 0.25, (angle, trans)  # the reference's own taboo thresholds: "the same pose"
    assert res.inlier_rate == res.best_inliers / float(len(c["target"])) and res.best_inliers > 0.8 * len(c["source"])


def test_same_seed_same_arrays_other_seed_other_samples(gpu):
    _, a, _ = run(gpu, 6, max_iterations=rr.CASE_ITERATIONS, seed=77)
    _, b, _ = run(gpu, 6, max_iterations=rr.CASE_ITERATIONS, seed=77)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    _, d, _ = run(gpu, 6, max_iterations=rr.CASE_ITERATIONS, seed=78)
    assert (a["source_indices"] != d["source_indices"]).mean() > 0.9


def test_early_stop_skips_the_chunks_behind_the_crossing(gpu):
    res, dev, p = run(gpu, 6, max_iterations=rr.CASE_ITERATIONS, chunk_iterations=64, early_stop_inlier_rate=0.3)
    ref, status = compare(6, res, dev, p)
    first = int(np.flatnonzero(status == rr.SKIPPED)[0])
    assert first % 64 == 0 and 0 < first < rr.CASE_ITERATIONS and (status[first:] == rr.SKIPPED).all() and res.early_stopped
    assert (dev["source_indices"][first:] == -1).all()


def test_taboo_list(gpu):
    res1, dev1, p1 = run(gpu, 6, max_iterations=rr.CASE_ITERATIONS)
    res2, dev2, p2 = run(gpu, 6, max_iterations=rr.CASE_ITERATIONS, taboo_list=[res1.T_target_source])
    ref, status = compare(6, res2, dev2, p2)
    assert (status == rr.TABOO).any() and dev2["status"][res1.best_iteration] == rr.TABOO
    angle, trans = rr.taboo_delta(res2.T_target_source, res1.T_target_source)
    assert not (angle < p2.taboo_thresh_rot and trans < p2.taboo_thresh_trans)


def test_explicit_sample_indices(gpu):
    """the caller's samples instead of the generator's: the restatement's own draws of another seed, reversed"""
    c = rr.make_case(6)
    given = np.array([rr.draw_samples(99, it, len(c["source"]), 3)[::-1] for it in range(64)], np.int32)
    res, dev, p = run(gpu, 6, max_iterations=64, sample_indices=given)
    compare(6, res, dev, p, sample_indices=given)
    assert np.array_equal(dev["source_indices"], given)
    with pytest.raises(IndexError):
        run(gpu, 6, max_iterations=64, sample_indices=np.full((64, 3), len(c["source"]), np.int32))


def test_three_source_points_and_a_collinear_triplet(gpu):
    """N_s = 3: the generator's redraws until the three indices are distinct, and explicit samples; the three points lie on a line, so the rotation about the line is
    free: the pose must be a rigid transform that maps the line's points onto their matches"""
    T = np.eye(4)
    T[:3, :3] = rr.rot([1.0, 0.5, -0.2], 0.9)
    T[:3, 3] = [2.0, 1.0, -3.0]
    line = np.array([[1.0, 2.0, 0.5], [2.5, 3.0, 1.0], [5.5, 5.0, 2.0]])  # p0 + s d, s = 0, 1, 3
    source = line.astype(np.float32)
    rng = np.random.default_rng(4)
    target = np.concatenate([line @ T[:3, :3].T + T[:3, 3], rng.normal(size=(30, 3)) * 20]).astype(np.float32)
    tf = rng.normal(size=(33, 33)).astype(np.float32)
    sf = tf[:3] + 0.001
    for given in (None, np.array([[0, 1, 2], [2, 0, 1], [1, 2, 0], [0, 2, 1]], np.int32)):
        p = gpu.RANSACParams(max_iterations=4, poly_error_thresh=0.5, inlier_voxel_resolution=1.0)
        res, hyp = gpu.estimate_pose_ransac_gpu(gpu.PointCloudGPU(target), gpu.PointCloudGPU(source), tf, sf, p, sample_indices=given, return_hypotheses=True)
        src = hyp.source_indices.cpu().numpy()
        want = np.array([rr.draw_samples(p.seed, it, 3, 3) for it in range(4)]) if given is None else given
        assert np.array_equal(src, want) and (np.sort(src, axis=1) == [0, 1, 2]).all()
        assert (hyp.status.cpu().numpy() == rr.SCORED).all() and np.array_equal(hyp.target_indices.cpu().numpy(), src)
        grid = rr.OccupancySet(1.0).insert(target)
        for it in range(4):
            P = hyp.poses.cpu().numpy()[it].reshape(4, 4).T
            R = P[:3, :3]
            assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and np.linalg.det(R) > 0.0
            assert np.abs(source.astype(np.float64) @ R.T + P[:3, 3] - target[:3]).max() < 1e-5  # (f32 rounding of the inputs: 2^-24 x 8 m)
            assert int(hyp.inliers.cpu().numpy()[it]) == grid.calc_overlap(source, P)
        assert res.best_iteration == 0 and res.best_inliers == 3 and res.inlier_rate == 3 / 33.0


def test_refusals(gpu):
    c = rr.make_case(6)
    t, s, tf, sf = device_case(gpu, 6)
    two = gpu.PointCloudGPU(c["source"][:2])
    with pytest.raises(gpu.GPError):  # fewer source points than samples
        gpu.estimate_pose_ransac_gpu(t, two, tf, sf[:2])
    gpu.estimate_pose_ransac_gpu(t, two, tf, sf[:2], gpu.RANSACParams(dof=4, max_iterations=8))  # (two are enough for dof 4)
    with pytest.raises(gpu.GPError):  # an empty target
        gpu.estimate_pose_ransac_gpu(gpu.PointCloudGPU(), s, tf[:0], sf)
    import torch

    with pytest.raises(gpu.GPError):
        gpu.estimate_pose_ransac_gpu(gpu.PointCloudGPU.from_device(torch.zeros((0, 3), dtype=torch.float32, device="cuda:0")), s, tf[:0], sf)
    with pytest.raises(gpu.GPError):  # mismatched D
        gpu.estimate_pose_ransac_gpu(t, s, tf, sf[:, :32])
    with pytest.raises(gpu.GPError):  # dof
        gpu.estimate_pose_ransac_gpu(t, s, tf, sf, gpu.RANSACParams(dof=5))
    wide = torch.zeros((len(c["target"]), 129), device="cuda:0")
    with pytest.raises(gpu.GPError):  # D > 128
        gpu.estimate_pose_ransac_gpu(t, s, wide, wide[: len(c["source"])])
    with pytest.raises(gpu.GPError):  # more than 64 taboo poses
        gpu.estimate_pose_ransac_gpu(t, s, tf, sf, gpu.RANSACParams(taboo_list=[np.eye(4)] * 65))


def test_weighted_alignment_alone(gpu):
    """align_points_se3_gpu / align_points_4dof_gpu against the restatement's SVD: a noisy weighted N-point problem (well conditioned: bound 1e-12 sigma1 / sigma2 with
    the sums' own rounding, N 2^-53 relative, far inside it), the exact recovery of a known transform, and a mirrored cloud (the det < 0 branch)"""
    rng = np.random.default_rng(8)
    for dof, fn, ref_fn in ((6, gpu.align_points_se3_gpu, rr.align_points_se3), (4, gpu.align_points_4dof_gpu, rr.align_points_4dof)):
        T = np.eye(4)
        T[:3, :3] = rr.rot([0.3, 0.5, -1.0], 0.8) if dof == 6 else rr.rot([0, 0, 1], -2.1)
        T[:3, 3] = [1.0, -4.0, 0.3]
        for n in (1, 3, 257, 1000):
            s = rng.normal(size=(n, 3)) * 5
            t = s @ T[:3, :3].T + T[:3, 3]
            w = rng.random(n) + 0.1
            if n >= 3:
                assert np.abs(fn(t, s, w) - T).max() < 1e-12, (dof, n)
            noisy = t + rng.normal(size=t.shape) * 0.05
            got, want = fn(noisy, s, w), ref_fn(noisy, s, w)
            H, _, _ = rr.cross_covariance(noisy, s, w)
            ok, bound = rr.rotation_bound(H, dof) if n >= 3 else (False, 0.0)
            R = got[:3, :3]
            assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and np.linalg.det(R) > 0.0
            if ok:
                assert np.linalg.norm(R - want[:3, :3]) <= bound + n * 2.0 ** -52, (dof, n)
                assert np.abs(got[:3, 3] - want[:3, 3]).max() <= (bound + n * 2.0 ** -52) * 20 + 1e-12 * 20
    s = rng.normal(size=(50, 3))
    got = gpu.align_points_se3_gpu(s * [1.0, 1.0, -1.0], s)
    want = rr.align_points_se3(s * [1.0, 1.0, -1.0], s)
    assert abs(np.linalg.det(got[:3, :3]) - 1.0) < 1e-12 and np.linalg.norm(got[:3, :3] - want[:3, :3]) < 1e-10

"""GPU tests of BASELINE configs[4]: exact k-NN, covariance estimation and GICP linearisation vs the oracle
(modelled on src/test/test_kdtree.cpp:92-163 for the k-NN part)."""
import numpy as np
import pytest

import icp_ref
import knn_ref
import oracle
from helpers import BLOCKS, assert_linearized_close, expmap

pytestmark = pytest.mark.gpu
PARITY_TOL = 1e-7
MARGIN = 1e-9  # test_icp_gpu.py's: the smallest relative tie / cut-off gap at which two f64 searches must agree
XI = np.array([0.01, -0.02, 0.015, 0.10, -0.05, 0.03])
NEARBY = np.array([0.002, -0.001, 0.003, 0.01, 0.02, -0.01])


def test_knn_matches_bruteforce(gpu):
    """1000 uniform points in [-100,100]^3, k in {1,2,3,5,10,15,20}: squared distances within 1e-6, with/without max_sq_dist"""
    rng = np.random.default_rng(0)
    p = rng.uniform(-100, 100, (1000, 3)).astype(np.float32)
    q = rng.uniform(-100, 100, (300, 3)).astype(np.float32)
    tree = gpu.KdTreeGPU(gpu.PointCloudGPU(p), cell_size=10.0)
    d2 = ((q[:, None, :].astype(np.float64) - p[None].astype(np.float64)) ** 2).sum(2)
    for k in [1, 2, 3, 5, 10, 15, 20]:
        idx, d, nf = tree.knn_search(q, k)
        ref = np.sort(d2, 1)[:, :k]
        assert (nf == k).all()
        assert np.abs(d - ref).max() < 1e-6
        assert np.abs(np.take_along_axis(d2, idx.astype(np.int64), 1) - d).max() < 1e-9
    idx, d, nf = tree.knn_search(q, 5, max_sq_dist=400.0)
    refc = (np.sort(d2, 1)[:, :5] < 400.0).sum(1)
    np.testing.assert_array_equal(nf, refc)
    assert ((idx >= 0).sum(1) == refc).all()


def test_knn_matches_oracle_kdtree_on_scan(gpu, kitti00):
    p = kitti00["target_points"]
    q = kitti00["source_points"][:3000]
    tree = gpu.KdTreeGPU(gpu.PointCloudGPU(p), cell_size=0.5)
    idx, d, nf = tree.knn_search(q, 10)
    oidx, od = oracle.OracleKdTree(p).knn(q, 10, num_threads=4)
    assert np.abs(d - od).max() < 1e-9
    assert (idx == oidx).mean() > 0.999  # ties at equal distance may be ordered differently


def test_covariances_match_oracle(gpu, kitti00):
    p = kitti00["source_points"]
    frame = gpu.PointCloudGPU(p)
    short = gpu.estimate_covariances_gpu(frame, 10)
    assert short == 0
    got = frame.covs_gpu.cpu().numpy().reshape(-1, 3, 3).transpose(0, 2, 1).astype(np.float64)
    ref, _ = oracle.estimate_covariances(p, 10, 4)
    rel = np.linalg.norm((got - ref).reshape(len(p), -1), axis=1) / np.linalg.norm(ref.reshape(len(p), -1), axis=1)
    # parity <= 1e-5 relative Frobenius except degenerate neighbourhoods (near-equal small eigenvalues: the eigenvector of the
    # reference's closed-form solver is itself arbitrary there); f32 output rounding alone is ~6e-8
    assert np.median(rel) < 2e-7
    assert (rel < 1e-5).mean() > 0.995
    w = np.linalg.eigvalsh(0.5 * (got + got.transpose(0, 2, 1)))
    np.testing.assert_allclose(np.median(w, 0), [1e-3, 1.0, 1.0], atol=1e-5)
    knn_ref.assert_covariances(p, 10, got, what="gpu kitti00_dec8 source")  # every point: bound by its own relgap, eigenvalues, ties by rule
    # too few points for k neighbours -> identity + count (covariance_estimation.cpp:27-31)
    tiny = gpu.PointCloudGPU(p[:5])
    assert gpu.estimate_covariances_gpu(tiny, 10) == 5
    np.testing.assert_array_equal(tiny.covs_gpu.cpu().numpy()[0], np.eye(3, dtype=np.float32).reshape(9))


@pytest.mark.parametrize("xi", [np.zeros(6), [0.01, -0.02, 0.015, 0.10, -0.05, 0.03]])
def test_gicp_linearize_matches_oracle(gpu, kitti00, xi):
    tgt = gpu.PointCloudGPU(kitti00["target_points"], kitti00["target_covs"])
    src = gpu.PointCloudGPU(kitti00["source_points"], kitti00["source_covs"])
    f = gpu.IntegratedGICPFactorGPU(0, 1, tgt, src)
    fo = oracle.OracleGICPFactor(kitti00["target_points"], kitti00["target_covs"], kitti00["source_points"], kitti00["source_covs"], 4)
    delta = expmap(xi)
    L, Lo = f.linearize_delta(delta), fo.linearize(delta)
    assert_linearized_close(L, Lo, PARITY_TOL, "gicp")
    # error() with correspondences / Mahalanobis frozen at the linearisation point
    de = delta @ expmap([0.002, -0.001, 0.003, 0.01, 0.02, -0.01])
    e = f.error({0: np.eye(4), 1: de})
    eo = fo.evaluate(de).error
    assert abs(e - eo) < PARITY_TOL * eo
    hf = f.linearize({0: np.eye(4), 1: delta})
    assert np.array_equal(hf.G[(1, 1)], L.H_source) and hf.keys == [0, 1]
    # the correspondences are kept between calls (the error evaluation above re-used those of the linearise); an error evaluation whose
    # linearisation pose is NOT the stored one must search again, and a second linearise at the first pose must give the first record
    import ctypes as C

    d2 = delta @ expmap([0.01, 0.0, -0.01, 0.05, 0.0, 0.02])
    out = C.c_double()
    gpu._capi.check(f._lib.gp_gicp_factor_compute_error(f._h, gpu.types._pose16(d2), gpu.types._pose16(de), C.byref(out)), "gicp compute_error")
    fo.linearize(d2)
    eo2 = fo.evaluate(de).error
    assert abs(out.value - eo2) < PARITY_TOL * eo2
    L2 = f.linearize_delta(delta)
    for k in BLOCKS:
        assert np.array_equal(getattr(L2, k), getattr(L, k)), k


def _check_gicp(gpu, tp, tc, sp, sc, delta, what, tgt=None):
    """one GICP factor on the device against the oracle's at `delta`: record, inlier count, error at a nearby pose on the stored correspondences.  The search
    is the ICP factor's: the same condition on the inputs (icp_ref's margins: no tie, nothing on the cut-off) before anything is compared."""
    tie, cut = icp_ref.ICPFactorRef(tp, sp).margins(delta)
    assert tie.min() > MARGIN and cut.min() > MARGIN, f"{what}: a correspondence two f64 implementations could decide differently (tie {tie.min():.2e}, cut-off {cut.min():.2e})"
    f = gpu.IntegratedGICPFactorGPU(0, 1, tgt if tgt is not None else gpu.PointCloudGPU(tp, tc), gpu.PointCloudGPU(sp, sc))
    fo = oracle.OracleGICPFactor(tp, tc, sp, sc, 4)
    L, Lo = f.linearize_delta(delta), fo.linearize(delta)
    print(f"[gicp] {what}: inliers {L.num_inliers} / {Lo.num_inliers}, error {L.error!r} / {Lo.error!r}")
    assert_linearized_close(L, Lo, PARITY_TOL, what)  # (the inlier counts are compared for equality)
    for k in BLOCKS + ["error"]:
        assert np.isfinite(getattr(L, k)).all(), k
    de = delta @ expmap(NEARBY)
    e, eo = f.error({0: np.eye(4), 1: de}), fo.evaluate(de).error
    assert abs(e - eo) <= PARITY_TOL * max(eo, 1e-300), (e, eo)
    return f, L, Lo


@pytest.fixture(scope="module")
def gicp_target(gpu, kitti00):
    return gpu.PointCloudGPU(kitti00["target_points"], kitti00["target_covs"])


@pytest.mark.parametrize("n", [1, 255, 257, 1024, 1025])
def test_gicp_source_sizes_at_lane_workgroup_and_tile_edges(gpu, kitti00, gicp_target, n):
    """one lane, one short of / one past a workgroup's stride, exactly one tile, one point into a second tile"""
    sp, sc = kitti00["source_points"][100 : 100 + n], kitti00["source_covs"][100 : 100 + n]
    _, L, _ = _check_gicp(gpu, kitti00["target_points"], kitti00["target_covs"], sp, sc, expmap(XI), f"n={n}", gicp_target)
    assert L.num_inliers == {1: 1, 255: 214, 257: 216, 1024: 909, 1025: 910}[n]  # the oracle's counts on this fixture


def test_gicp_every_point_beyond_the_cut_off(gpu, kitti00, gicp_target):
    far = expmap([0.0, 0.0, 0.0, 0.0, 0.0, 500.0])  # half a kilometre above the scan
    f, L, Lo = _check_gicp(gpu, kitti00["target_points"], kitti00["target_covs"], kitti00["source_points"][:1025], kitti00["source_covs"][:1025], far, "all beyond", gicp_target)
    assert Lo.num_inliers == 0 and L.num_inliers == 0 and L.error == 0.0
    for k in BLOCKS:
        assert not np.any(getattr(L, k)), k
    assert f.error({0: np.eye(4), 1: far}) == 0.0


def test_gicp_non_orthonormal_pose_takes_the_explicit_sums(gpu, kitti00, gicp_target):
    delta = expmap(XI)
    delta[:3, :3] = delta[:3, :3] @ (np.eye(3) + 1e-6 * np.random.default_rng(11).normal(size=(3, 3)))  # orthonormal to 1e-6 only, as test_icp_gpu.py builds it
    assert np.abs(delta[:3, :3].T @ delta[:3, :3] - np.eye(3)).max() > 1e-7
    _, L, _ = _check_gicp(gpu, kitti00["target_points"], kitti00["target_covs"], kitti00["source_points"], kitti00["source_covs"], delta, "non-orthonormal", gicp_target)
    assert L.num_inliers == 14989


def test_gicp_target_of_one_point(gpu, kitti00):
    tp, tc = kitti00["target_points"][:1], kitti00["target_covs"][:1]
    sp = (tp.astype(np.float64) + np.random.default_rng(5).uniform(-0.9, 0.9, (300, 3))).astype(np.float32)  # some within 1 m of the one point, some beyond
    _, L, _ = _check_gicp(gpu, tp, tc, sp, kitti00["source_covs"][:300], np.eye(4), "one target point")
    assert 0 < L.num_inliers < 300


def test_gicp_two_linearises_are_bit_identical(gpu, kitti00, gicp_target):
    src = gpu.PointCloudGPU(kitti00["source_points"], kitti00["source_covs"])
    for delta in (expmap(XI), expmap(XI) @ np.diag([1.0 + 1e-6, 1.0, 1.0, 1.0])):  # the rigid and the general kernels
        f = gpu.IntegratedGICPFactorGPU(0, 1, gicp_target, src)
        A, B = f.linearize_delta(delta), f.linearize_delta(delta)
        Cc = gpu.IntegratedGICPFactorGPU(0, 1, gicp_target, src).linearize_delta(delta)
        for k in BLOCKS + ["error", "num_inliers"]:
            assert np.array_equal(getattr(A, k), getattr(B, k)) and np.array_equal(getattr(A, k), getattr(Cc, k)), k
        assert A.num_inliers > 14000


def test_binned_and_hashed_structures_agree(gpu, kitti00):
    """the default search structure (occupancy-block grid over the cells + cell-sorted points) and the hashed multi-level grid (the
    fallback of clouds whose bounding box is too large for the block grid) return the same neighbours; a cloud with non-finite points
    and one with a far outlier (bounding box beyond the block budget -> fallback) still give exact answers"""
    lib = gpu.load()
    p = kitti00["target_points"]
    q = kitti00["source_points"][:4000]
    res = []
    for hashed in (0, 1):  # GP_TUNE_KNN_STRUCTURE of THIS structure (gp_point_grid_create_ex)
        tree = gpu.KdTreeGPU(gpu.PointCloudGPU(p), cell_size=0.5, structure=hashed)
        res.append(tree.knn_search(q, 10))
        res.append(tree.knn_search(q, 1, max_sq_dist=0.04))
    assert np.abs(res[0][1] - res[2][1]).max() == 0.0 and (res[0][0] == res[2][0]).mean() > 0.999
    np.testing.assert_array_equal(res[1][2], res[3][2])
    assert np.array_equal(res[1][1][res[1][2] == 1], res[3][1][res[3][2] == 1])
    # non-finite points are left out of the structure; queries that are not finite find nothing
    p2 = p.copy()
    p2[[3, 77, 5000]] = [np.nan, np.inf, -np.inf]
    keep = np.isfinite(p2).all(1)
    q2 = q.copy()
    q2[5] = np.nan
    idx, d, nf = gpu.KdTreeGPU(gpu.PointCloudGPU(p2), cell_size=0.5).knn_search(q2, 5)
    oidx, od = oracle.OracleKdTree(p2[keep]).knn(np.delete(q2, 5, 0), 5, num_threads=4)
    assert nf[5] == 0 and (np.delete(nf, 5) == 5).all()
    assert np.abs(np.delete(d, 5, 0) - od).max() < 1e-9
    # covariance estimation: the per-lane search on the binned structure (default), the row-tiled pass, two binned levels and the hashed grid agree
    # (same exact neighbour sets; ties may be ordered differently, which the sample covariance does not see)
    covs = []
    for mode in (0, 3, 4, 1):
        fr0 = gpu.PointCloudGPU(p)
        assert gpu.estimate_covariances_gpu(fr0, 10, structure=mode) == 0
        covs.append(fr0.download("covs").astype(np.float64))
        knn_ref.assert_covariances(p, 10, covs[-1], what=f"gpu structure {mode} kitti00_dec8 target")
    for other in covs[1:]:
        rel = np.linalg.norm((covs[0] - other).reshape(len(p), -1), axis=1) / np.linalg.norm(other.reshape(len(p), -1), axis=1)
        assert (rel < 1e-5).mean() > 0.999, (rel < 1e-5).mean()  # all but the neighbourhoods with exact distance ties at rank k
    # covariance estimation on the same cloud: identity + counted as short for the three non-finite points
    fr = gpu.PointCloudGPU(p2)
    assert gpu.estimate_covariances_gpu(fr, 10) == 3
    np.testing.assert_array_equal(fr.download("covs")[77], np.eye(3, dtype=np.float32))
    # a far outlier: 40 km away at 0.1 m cells the bounding box needs > 2^24 blocks -> hashed fallback, still exact
    p3 = np.concatenate([p, np.array([[40000.0, -30000.0, 5000.0]], np.float32)])
    idx3, d3, nf3 = gpu.KdTreeGPU(gpu.PointCloudGPU(p3), cell_size=0.1).knn_search(q[:500], 10)
    oidx3, od3 = oracle.OracleKdTree(p3).knn(q[:500], 10, num_threads=4)
    assert np.abs(d3 - od3).max() < 1e-9


def _cov_rel(a, b):
    a, b = a.reshape(len(a), -1).astype(np.float64), b.reshape(len(b), -1).astype(np.float64)
    return np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)


def test_sparse_neighbourhoods_go_through_the_cooperative_pass(gpu, kitti00):
    """Round 5: queries with fewer than k points within a cell edge of their cell (the far field of a scan) are searched by one WAVE each
    (covariance_far_kernel: the blocks of a cube shell dealt to the lanes, the lanes' lists merged after every shell) instead of one lane walking empty space.
    Exact like the per-lane search: (i) a cloud that is ALL far field -- uniform points a metre apart -- against the oracle's kd-tree covariances; (ii) GP_TUNE_KNN_STRUCTURE
    7 (round 4's search, every query lane by lane) gives the same covariances on a real scan and on the sparse cloud; (iii) outliers tens of metres from everything (past
    the kernel's eight block shells: the superblock walk on one lane) and a neighbour count below the list size; semantics: features/covariance_estimation.cpp:18-77,
    ann/knn_result.hpp:89-109."""
    rng = np.random.default_rng(17)
    sparse = rng.uniform(-40.0, 40.0, size=(30_000, 3)).astype(np.float32)  # ~0.06 points per m^3 ... one point per ~2.6 m cube: every query is "sparse"
    sparse[:, 2] *= 0.1  # (a slab: neighbours within a few metres)
    outliers = np.array([[300.0, 0.0, 0.0], [0.0, -250.0, 3.0], [305.0, 1.0, 0.5]], np.float32)
    cloud = np.concatenate([sparse, outliers])
    ref, _ = oracle.estimate_covariances(cloud, 10, 4)
    got = {}
    for structure in (0, 7):
        fr = gpu.PointCloudGPU(cloud)
        assert gpu.estimate_covariances_gpu(fr, 10, structure=structure) == 0
        got[structure] = fr.download("covs")
        rel = _cov_rel(got[structure], ref)
        assert np.median(rel) < 2e-7 and (rel < 1e-5).mean() > 0.995, (structure, np.median(rel), (rel < 1e-5).mean())
        knn_ref.assert_covariances(cloud, 10, got[structure], what=f"gpu structure {structure} sparse slab")
    rel07 = _cov_rel(got[0], got[7])
    assert (rel07 < 1e-6).mean() > 0.999, (rel07 < 1e-6).mean()  # the same neighbour sets (exact ties at rank k aside)
    # a real scan: near field through the per-lane search, far field through the cooperative pass -- against round 4's search
    res = {}
    for structure in (0, 7):
        fr = gpu.PointCloudGPU(kitti00["target_points"])
        assert gpu.estimate_covariances_gpu(fr, 10, structure=structure) == 0
        res[structure] = fr.download("covs")
        knn_ref.assert_covariances(kitti00["target_points"], 10, res[structure], what=f"gpu structure {structure} kitti00_dec8 target")
    rel = _cov_rel(res[0], res[7])
    assert (rel < 1e-6).mean() > 0.999, (rel < 1e-6).mean()
    # k below the list size, and a cloud with fewer than k points in reach of the cooperative pass
    for k in (3, 7):
        fr = gpu.PointCloudGPU(cloud)
        assert gpu.estimate_covariances_gpu(fr, k) == 0
        refk, _ = oracle.estimate_covariances(cloud, k, 4)
        relk = _cov_rel(fr.download("covs"), refk)
        assert np.median(relk) < 2e-7 and (relk < 1e-5).mean() > 0.99, (k, np.median(relk))
        knn_ref.assert_covariances(cloud, k, fr.download("covs"), what="gpu structure 0 sparse slab")
    few = gpu.PointCloudGPU(cloud[:7])
    assert gpu.estimate_covariances_gpu(few, 10) == 7
    np.testing.assert_array_equal(few.download("covs")[3], np.eye(3, dtype=np.float32))


def test_cooperative_pass_with_duplicate_points_and_clusters(gpu):
    """exact ties in distance (duplicated points: the same coordinates, so whichever duplicate is kept the covariance is the same) and isolated tight clusters (fewer than k
    points within metres, then a dense blob): the cooperative pass and the per-lane search agree with the oracle's kd-tree covariances"""
    rng = np.random.default_rng(23)
    base = rng.uniform(-30.0, 30.0, size=(4000, 3)).astype(np.float32)
    base[:, 2] *= 0.05
    dup = np.repeat(base[:1500], 3, axis=0)  # every one of these three times
    blobs = []
    for c in rng.uniform(-200.0, 200.0, size=(12, 3)).astype(np.float32):  # 12 clusters of 4 .. 40 points, tens of metres apart
        m = int(rng.integers(4, 41))
        blobs.append(c + rng.normal(0.0, 0.05, size=(m, 3)).astype(np.float32))
    cloud = np.concatenate([base, dup] + blobs).astype(np.float32)
    cloud = cloud[rng.permutation(len(cloud))]
    ref, _ = oracle.estimate_covariances(cloud, 10, 4)
    for structure in (0, 7):
        fr = gpu.PointCloudGPU(cloud)
        assert gpu.estimate_covariances_gpu(fr, 10, structure=structure) == 0
        rel = _cov_rel(fr.download("covs"), ref)
        # (degenerate neighbourhoods -- a point and its two copies among the ten: rank-deficient sample covariances, where the eigenvector of the reference's closed form is
        # itself arbitrary -- are excluded by the same 1e-5 / fraction rule as test_covariances_match_oracle)
        assert np.median(rel) < 1e-6 and (rel < 1e-5).mean() > 0.9, (structure, np.median(rel), (rel < 1e-5).mean())
        knn_ref.assert_covariances(cloud, 10, fr.download("covs"), what=f"gpu structure {structure} duplicates and clusters")


def test_cooperative_pass_skips_empty_shells_and_finds_what_lies_behind_them(gpu):
    """Isolated points with a few neighbours a superblock (4 m) away, then NOTHING for 13-70 m, then a wall: the ten neighbours straddle the gap, covariance_far_kernel walks
    3 .. 17 shells of superblocks most of which are empty, and the stopping rule must not fire on the near handful.  (Written for a variant that skipped empty shells through a
    coarser occupancy level -- measured, no faster, removed: profiles/r05_c5_summary.txt item 8 -- and kept: it holds any walk to the oracle's kd-tree covariances and to round 4's
    lane-by-lane search, structure 7.)"""
    rng = np.random.default_rng(29)
    parts = []
    for i, gap in enumerate([13.0, 18.0, 22.0, 27.0, 33.0, 38.0, 70.0]):
        origin = np.array([400.0 * i, 0.0, 0.0])
        yz = rng.uniform(-6.0, 6.0, size=(1500, 2))
        wall = np.column_stack([np.full(len(yz), gap) + rng.normal(0.0, 0.02, len(yz)), yz])  # a wall `gap` metres from the lonely points
        lonely = rng.normal(0.0, 0.3, size=(3, 3))                                            # three lonely points ...
        near = lonely[:1] + rng.normal(0.0, 0.2, size=(4, 3)) + [0.0, 4.5, 0.0]               # ... and four more a superblock away: fewer than k together
        parts += [origin + wall, origin + lonely, origin + near]
    cloud = np.concatenate(parts).astype(np.float32)
    cloud = cloud[rng.permutation(len(cloud))]
    ref, _ = oracle.estimate_covariances(cloud, 10, 4)
    got = {}
    for structure in (0, 7):
        fr = gpu.PointCloudGPU(cloud)
        assert gpu.estimate_covariances_gpu(fr, 10, structure=structure) == 0
        got[structure] = fr.download("covs")
        rel = _cov_rel(got[structure], ref)
        assert np.median(rel) < 1e-6 and (rel < 1e-5).mean() > 0.995, (structure, np.median(rel), (rel < 1e-5).mean())
        knn_ref.assert_covariances(cloud, 10, got[structure], what=f"gpu structure {structure} wall and gap")
    lonely_idx = np.where(np.abs(cloud[:, 0] - 400.0 * np.round(cloud[:, 0] / 400.0)) < 8.0)[0]  # the points in front of the walls
    assert len(lonely_idx) == 7 * 7
    rel = _cov_rel(got[0][lonely_idx], ref[lonely_idx])
    assert (rel < 1e-5).all(), rel.max()  # every one of them reaches across its gap
    assert (_cov_rel(got[0], got[7]) < 1e-6).mean() > 0.999


def test_side_stream_is_the_candidate_that_does_not_wait_for_the_callers_grid(gpu):
    """gp_estimate_covariances' second launch overlaps the first only when the two streams' hardware queues sit on different dispatch pipes; the library probes its candidate
    streams once per caller stream and keeps the one with the shortest delay (gp_knn.hip, SideStream).  The choice is the probe's minimum, it is made once, and the covariances do
    not depend on it (bit-identical between a call on the null stream and one on a stream of the caller's)."""
    import ctypes as C

    import torch

    from gtsam_points_amd import _capi

    lib = _capi.load()
    for stream in (None, torch.cuda.Stream()):
        sp = C.c_void_p(stream.cuda_stream) if stream is not None else None
        delays, chosen = (C.c_float * 4)(), C.c_int(-1)
        _capi.check(lib.gp_debug_side_stream_probe(sp, delays, C.byref(chosen)), "gp_debug_side_stream_probe")
        d = list(delays)
        assert 0 <= chosen.value < 4 and any(x >= 0 for x in d), d
        probed = [x for x in d if x >= 0]
        assert d[chosen.value] >= 0 and d[chosen.value] <= min(probed) + 2.0, (d, chosen.value)
        again, chosen2 = (C.c_float * 4)(), C.c_int(-1)
        _capi.check(lib.gp_debug_side_stream_probe(sp, again, C.byref(chosen2)), "gp_debug_side_stream_probe")
        assert list(again) == d and chosen2.value == chosen.value  # probed once per caller stream
    # more caller streams than the per-thread table holds (16): the oldest entries make room, every caller still gets a probed choice
    many = [torch.cuda.Stream() for _ in range(20)]
    for st in many:
        delays, chosen = (C.c_float * 4)(), C.c_int(-1)
        _capi.check(lib.gp_debug_side_stream_probe(C.c_void_p(st.cuda_stream), delays, C.byref(chosen)), "gp_debug_side_stream_probe")
        assert list(delays)[chosen.value] >= 0
    rng = np.random.default_rng(3)
    pts = np.concatenate([rng.uniform(-20, 20, (60_000, 3)) * [1, 1, 0.05], rng.uniform(-60, 60, (3_000, 3))]).astype(np.float32)
    a = gpu.PointCloudGPU(pts)
    gpu.estimate_covariances_gpu(a, 10)
    b = gpu.PointCloudGPU(pts)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        gpu.estimate_covariances_gpu(b, 10, stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(a.download("covs"), b.download("covs"))

"""Normal estimation on the device (gp_estimate_normals_from_covs, gp_estimate_normals_covariances; gtsam_points_amd.features): every normal of every cloud
against the numpy restatement of features/normal_estimation.cpp, point by point (tests/normals_ref.py: direction to the bound the covariances are already held
to, unit length, the sign rule outside its band; tests/test_normals_ref_cpu.py shows the reference alone to pass it), the covariances of the fused call bit for
bit against gp_estimate_covariances, the two paths against each other, and the normals in use: surface validation of a VGICP factor, and the factor's cached
pointer when the normals are estimated again."""
import ctypes as C

import numpy as np
import pytest

import knn_ref
import normals_ref
import oracle
from helpers import BLOCKS, assert_linearized_close, expmap

pytestmark = pytest.mark.gpu
PARITY_TOL = 1e-6  # tests/test_vgicp_gpu.py's, for the default kernel


@pytest.fixture(scope="module")
def scan():
    import os

    return np.fromfile(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kitti_00", "000000.bin"), dtype=np.float32).reshape(-1, 3)


@pytest.fixture(scope="module")
def clouds(scan):
    return {
        "kitti_00/000000.bin": scan,
        "sparse slab": knn_ref.sparse_slab_cloud(),
        "wall and gap": knn_ref.wall_and_gap_cloud(),
        "duplicates and clusters": knn_ref.duplicates_cloud(),
    }


_CLS = {}


def _cls(name, cloud, k, subset=None):
    key = (name, k)
    if key not in _CLS:
        _CLS[key] = knn_ref.classify(cloud, k, subset)
    return _CLS[key]


def _surface_keep(points, normals, delta):
    """lookup_voxels.cuh:41-50 restated in numpy (as tests/test_vgicp_gpu.py restates it): rejected when normalized(T p) . (R n) > 0.174 = cos(80 deg)"""
    p, n = points.astype(np.float64), normals.astype(np.float64)
    q = p @ delta[:3, :3].T + delta[:3, 3]
    tn = n @ delta[:3, :3].T
    return ~(((q / np.linalg.norm(q, axis=1, keepdims=True)) * tn).sum(1) > 0.174)


def _lin(gpu, f, delta):
    rec = gpu._capi.Linearized6()
    gpu._capi.check(f._lib.gp_vgicp_factor_linearize(f._h, gpu.types._pose16(delta), C.byref(rec)), "linearize")
    return gpu.LinearizedSystem6(rec)


# ---- 1. the k-NN path ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", [("kitti_00/000000.bin", 5), ("kitti_00/000000.bin", 10), ("kitti_00/000000.bin", 20), ("sparse slab", 5), ("sparse slab", 10),
                                    ("sparse slab", 20), ("wall and gap", 10), ("duplicates and clusters", 10)])
def test_knn_normals_every_point(gpu, clouds, name, k):
    """normals only (covs_dev = NULL) and the fused call, each held to the per-point rules"""
    cloud = clouds[name]
    cls = _cls(name, cloud, k)
    fr = gpu.PointCloudGPU(cloud)
    assert gpu.estimate_normals_gpu(fr, k) == int(cls["short"].sum()) and fr.covs_gpu is None
    normals_ref.assert_normals(cloud, k, fr.download("normals"), what=f"gpu normals only, {name}", cls=cls)
    both = gpu.PointCloudGPU(cloud)
    assert gpu.estimate_normals_covariances_gpu(both, k) == int(cls["short"].sum())
    normals_ref.assert_normals(cloud, k, both.download("normals"), what=f"gpu fused, {name}", cls=cls)
    knn_ref.assert_covariances(cloud, k, both.download("covs"), what=f"gpu fused, {name}", cls=cls)


def test_knn_normals_of_a_million_points(gpu):
    """the 1 M-point C2 source (heavy-first order, two-stream launch, cooperative far pass), checked on a seeded sample of 20 000 points"""
    from gtsam_points_amd import synthetic

    cloud = synthetic.make_c2_workload(1_000_000, 1_000_000, seed=42)["source_points"]
    subset = np.sort(np.random.default_rng(7).choice(len(cloud), 20_000, replace=False))
    for k in (5, 10, 20):
        cls = knn_ref.classify(cloud, k, subset)
        fr = gpu.PointCloudGPU(cloud)
        short = gpu.estimate_normals_covariances_gpu(fr, k)
        normals_ref.assert_normals(cloud, k, fr.download("normals")[subset], what="gpu fused, C2 source 1 M (sample)", subset=subset, cls=cls)
        knn_ref.assert_covariances(cloud, k, fr.download("covs")[subset], what="gpu fused, C2 source 1 M (sample)", subset=subset, cls=cls)
        only = gpu.PointCloudGPU(cloud)
        assert gpu.estimate_normals_gpu(only, k) == short
        assert np.array_equal(only.download("normals"), fr.download("normals"))


def test_edges_one_neighbour_too_few_points_and_non_finite_ones(gpu, clouds, scan):
    """k = 1: every sample covariance is the zero matrix, the identity basis gives (1, 0, 0), turned where p.x > 1.  Fewer than k points: all short, the same
    rule.  Non-finite points: (+-1, 0, 0), counted as short; their finite neighbours as ever."""
    cloud = clouds["sparse slab"]
    want = np.zeros((len(cloud), 3), np.float32)
    want[:, 0] = np.where(cloud[:, 0] > 1.0, -1.0, 1.0)
    for call in (gpu.estimate_normals_gpu, gpu.estimate_normals_covariances_gpu):
        fr = gpu.PointCloudGPU(cloud)
        assert call(fr, 1) == 0
        np.testing.assert_array_equal(fr.download("normals"), want)
    for k in (10, 20):
        few = knn_ref.scan_cut(scan, k - 1)
        for call in (gpu.estimate_normals_gpu, gpu.estimate_normals_covariances_gpu):
            fr = gpu.PointCloudGPU(few)
            assert call(fr, k) == k - 1
            normals_ref.assert_normals(few, k, fr.download("normals"), what=f"gpu, {k - 1} points", cap_is_condition=False)
            w = np.zeros((k - 1, 3), np.float32)
            w[:, 0] = np.where(few[:, 0] > 1.0, -1.0, 1.0)
            np.testing.assert_array_equal(fr.download("normals"), w)
        np.testing.assert_array_equal(fr.download("covs"), np.repeat(np.eye(3, dtype=np.float32)[None], k - 1, 0))
    holes = clouds["kitti_00/000000.bin"][:40_000].copy()
    rng = np.random.default_rng(59)
    rows = rng.choice(len(holes), 400, replace=False)
    for r in rows:
        holes[r, rng.choice(3, rng.integers(1, 4), replace=False)] = rng.choice([np.nan, np.inf, -np.inf])
    cls = knn_ref.classify(holes, 10)
    for call in (gpu.estimate_normals_gpu, gpu.estimate_normals_covariances_gpu):
        fr = gpu.PointCloudGPU(holes)
        assert call(fr, 10) == int(cls["short"].sum()) >= 400
        normals_ref.assert_normals(holes, 10, fr.download("normals"), what="gpu, 1 % non-finite points", cls=cls, cap_is_condition=False)


# ---- 2. from given covariances -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["kitti_00/000000.bin", "sparse slab", "wall and gap", "duplicates and clusters"])
def test_normals_from_device_covariances(gpu, clouds, name):
    cloud = clouds[name]
    fr = gpu.PointCloudGPU(cloud)
    gpu.estimate_covariances_gpu(fr, 10)
    given = fr.covs_gpu.cpu().numpy()
    assert gpu.estimate_normals_gpu(fr, 10) == 0  # covariances present: read off them
    assert np.array_equal(fr.covs_gpu.cpu().numpy(), given)
    normals_ref.assert_normals_from_covs(cloud, given, fr.download("normals"), what=f"gpu from covariances, {name}")


def test_normals_from_golden_and_identity_covariances(gpu, kitti07, scan):
    for i in range(3):
        fr = gpu.PointCloudGPU(kitti07[f"points_{i}"], kitti07[f"covs_{i}"])
        assert gpu.estimate_normals_gpu(fr) == 0
        normals_ref.assert_normals_from_covs(kitti07[f"points_{i}"], fr.covs_gpu.cpu().numpy(), fr.download("normals"), what=f"gpu from kitti07 golden covariances {i}")
    few = gpu.PointCloudGPU(knn_ref.scan_cut(scan, 9))  # identity covariances of short points: (+-1, 0, 0)
    assert gpu.estimate_covariances_gpu(few, 10) == 9
    gpu.estimate_normals_gpu(few)
    normals_ref.assert_normals_from_covs(knn_ref.scan_cut(scan, 9), few.covs_gpu.cpu().numpy(), few.download("normals"), what="gpu from identity covariances")


# ---- 3. one search, same bits --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [5, 10, 20])
def test_fused_call_writes_the_same_bits(gpu, clouds, k):
    import torch

    for name in ("kitti_00/000000.bin", "sparse slab", "duplicates and clusters"):
        cloud = clouds[name]
        a, b, c = gpu.PointCloudGPU(cloud), gpu.PointCloudGPU(cloud), gpu.PointCloudGPU(cloud)
        short_a = gpu.estimate_covariances_gpu(a, k)
        short_b = gpu.estimate_normals_covariances_gpu(b, k)
        short_c = gpu.estimate_normals_gpu(c, k)
        assert short_a == short_b == short_c
        assert torch.equal(a.covs_gpu, b.covs_gpu), (name, k)
        assert torch.equal(b.normals_gpu, c.normals_gpu), (name, k)
        assert c.covs_gpu is None


# ---- 4. the two paths agree ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["kitti_00/000000.bin", "sparse slab", "wall and gap"])
def test_the_two_paths_agree(gpu, clouds, name):
    cloud = clouds[name]
    cls = _cls(name, cloud, 10)
    fr = gpu.PointCloudGPU(cloud)
    gpu.estimate_normals_covariances_gpu(fr, 10)
    knn = fr.download("normals").astype(np.float64)
    gpu.estimate_normals_gpu(fr)  # covariances present: from the device's own f32 covariances
    frm = fr.download("normals").astype(np.float64)
    ok = ~(cls["tie"] | (cls["relgap"] < knn_ref.RELGAP_EXEMPT) | cls["short"])
    sin = normals_ref.sin_angle(knn, frm)
    bound = normals_ref.direction_bound(cls["relgap"]) + knn_ref.TAU_OUT / normals_ref.SCALE
    print(f"[normals_ref] {name}: k-NN path against from-covariances path, worst sin / (sum of bounds) = {float((sin[ok] / bound[ok]).max()):.3e}")
    bad = np.flatnonzero(ok & (sin > bound))
    assert len(bad) == 0, (bad[:10].tolist(), sin[bad[:10]].tolist(), bound[bad[:10]].tolist())


# ---- 5. end to end: the normals in the surface-validation gate ------------------------------------------------------------------------------------------
def test_surface_validation_on_estimated_normals(gpu):
    from gtsam_points_amd import synthetic

    d = synthetic.make_pair(20000, 40000, seed=5)
    tgt = gpu.PointCloudGPU(d["target_points"], d["target_covs"])
    vm = gpu.GaussianVoxelMapGPU(0.5, target_points_drop_rate=0.0)
    vm.insert(tgt)
    src = gpu.PointCloudGPU(d["source_points"])
    assert gpu.estimate_normals_covariances_gpu(src, 10) == 0
    normals, covs = src.download("normals"), src.covs_gpu.cpu().numpy()
    omap = oracle.OracleVoxelMap(0.5)
    omap.insert(d["target_points"], d["target_covs"])
    # at the true pose every estimated normal faces the sensor and the gate keeps the cloud; evaluated 12 m further along x the rays reach a sixth of the
    # points from behind (3231 by the numpy reference's normals) and the gate decides the record
    for what, delta in [("true pose", d["T_true"]), ("12 m off", d["T_true"] @ expmap([0.0, 0.0, 0.0, 12.0, 0.0, 0.0]))]:
        f = gpu.IntegratedVGICPFactorGPU(0, 1, vm, src)
        L0 = _lin(gpu, f, delta)
        f.set_enable_surface_validation(True)
        L1 = _lin(gpu, f, delta)
        keep = _surface_keep(d["source_points"], normals, delta)
        print(f"[normals_ref] surface validation on estimated normals, {what}: gate rejects {int((~keep).sum())} of {len(keep)}, inliers {L0.num_inliers} -> {L1.num_inliers}")
        fo = oracle.OracleVGICPFactor(omap, d["source_points"][keep], covs[keep], 2)
        assert_linearized_close(L1, fo.linearize(delta), PARITY_TOL, f"surface validation on estimated normals, {what}")
        assert L1.num_inliers <= L0.num_inliers
        if what == "12 m off":
            assert (~keep).sum() > 1000 and 0 < L1.num_inliers < L0.num_inliers
        de = delta @ expmap([0.002, -0.001, 0.003, 0.01, 0.02, -0.01])
        err = C.c_double()
        gpu._capi.check(f._lib.gp_vgicp_factor_compute_error(f._h, gpu.types._pose16(delta), gpu.types._pose16(de), C.byref(err)), "compute_error")
        eo = fo.error(de)
        assert abs(err.value - eo) <= PARITY_TOL * abs(eo)
    delta = d["T_true"]
    keep = _surface_keep(d["source_points"], normals, delta)
    # the sign rule at work: ground and walls lie more than 1 m from the sensor, so the estimated normals face it like the generator's
    keep_true = _surface_keep(d["source_points"], d["source_normals"], delta)
    share = (keep & keep_true).sum() / keep_true.sum()
    print(f"[normals_ref] gate with estimated normals keeps {share:.4%} of what the gate with the generator's normals keeps ({keep.sum()} / {keep_true.sum()})")
    assert share >= SHARE_OF_TRUE_GATE


SHARE_OF_TRUE_GATE = 0.99  # (the numpy reference -- oracle covariances, eigh, the sign rule -- reaches 100 % on this scene)


# ---- 6. the factor's cached pointers ---------------------------------------------------------------------------------------------------------------------
def test_estimating_again_does_not_leave_a_factor_with_a_stale_pointer(gpu):
    """a factor caches the device pointers of its source and re-reads them when source.generation moved.  Both calls replace frame.normals_gpu (the fused one
    frame.covs_gpu too, under a live packed mirror); the freed block is handed out again at once -- here to a tensor of sevens.  The live factor must linearise
    exactly as a freshly built one."""
    import torch

    from gtsam_points_amd import synthetic

    d = synthetic.make_pair(70_013, 100_000, seed=5)
    tgt = gpu.PointCloudGPU(d["target_points"], d["target_covs"])
    vm = gpu.GaussianVoxelMapGPU(0.5, target_points_drop_rate=0.0)
    vm.insert(tgt)
    src = gpu.PointCloudGPU(d["source_points"])
    gpu.estimate_normals_covariances_gpu(src, 10)
    delta = d["T_true"]
    f = gpu.IntegratedVGICPFactorGPU(0, 1, vm, src)
    f.set_enable_surface_validation(True)
    L0 = _lin(gpu, f, delta)
    assert 0 < L0.num_inliers < src.size()
    src.add_points((d["source_points"] + np.float32(0.05)).astype(np.float32))  # the cloud moved: a new points tensor
    f.touch_points()
    junk = []

    def check(what):
        n = src.size()
        junk.append((torch.full((n, 3), 7.0, dtype=torch.float32, device=src.device), torch.full((n, 9), 7.0, dtype=torch.float32, device=src.device)))
        torch.cuda.synchronize()
        f.touch_points()
        L = _lin(gpu, f, delta)
        fresh = gpu.IntegratedVGICPFactorGPU(0, 1, vm, src)
        fresh.set_enable_surface_validation(True)
        Lf = _lin(gpu, fresh, delta)
        for k in BLOCKS:
            assert np.array_equal(getattr(L, k), getattr(Lf, k)), (what, k)
        assert L.num_inliers == Lf.num_inliers > 0 and L.error == Lf.error, what
        return L

    gen = src.generation
    gpu.estimate_normals_gpu(src)  # covariances present: from them, with the moved points' signs
    assert src.generation > gen and "normals" not in src._host
    check("estimate_normals_gpu")
    gen = src.generation
    gpu.estimate_normals_covariances_gpu(src, 5)
    assert src.generation > gen and "covs" not in src._host
    L5 = check("estimate_normals_covariances_gpu")
    assert not np.array_equal(L5.H_source, L0.H_source)


# ---- 7. argument checks ----------------------------------------------------------------------------------------------------------------------------------
def test_argument_checks_come_before_device_work(gpu):
    import torch

    lib = gpu.load()
    pts = torch.zeros((100, 3), dtype=torch.float32, device="cuda:0")
    nrm = torch.full((100, 3), 5.0, dtype=torch.float32, device="cuda:0")
    cov = torch.full((100, 9), 5.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    p, n, c = (C.c_void_p(t.data_ptr()) for t in (pts, nrm, cov))
    short = C.c_int(0)
    for k, nn, cc in [(0, n, c), (33, n, c), (10, None, None)]:
        assert lib.gp_estimate_normals_covariances(p, 100, k, 0.0, nn, cc, C.byref(short), None) == 1  # GP_ERROR_INVALID_ARGUMENT
    assert lib.gp_estimate_normals_covariances(p, 0, 10, 0.0, n, c, C.byref(short), None) == 0
    assert lib.gp_estimate_normals_from_covs(p, None, 100, n, None) == 1 and lib.gp_estimate_normals_from_covs(p, c, 0, n, None) == 0
    torch.cuda.synchronize()
    assert bool((nrm == 5.0).all()) and bool((cov == 5.0).all())  # nothing was written
    fr = gpu.PointCloudGPU(np.zeros((50, 3), np.float32))
    with pytest.raises(gpu.GPError):
        gpu.estimate_normals_gpu(fr, 0)
    with pytest.raises(gpu.GPError):
        gpu.estimate_normals_covariances_gpu(fr, 33)
    assert fr.normals_gpu is None and fr.covs_gpu is None

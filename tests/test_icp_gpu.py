"""GPU tests of IntegratedICPFactorGPU (gp_icp_factor_*: point-to-point and point-to-plane ICP on a shared KdTreeGPU) against tests/icp_ref.py, the numpy f64
restatement of impl/integrated_icp_factor_impl.hpp.  Parity at the GICP test's tolerance: both sides compute in f64 on the same f32 inputs and differ by the
order of ~15,000-term sums (about 1e-13 relative); 1e-7 is the project's gate for an f64 factor.

Condition on the inputs: the device search and the brute-force reference must pick the same target for every source point, which two correct f64
implementations only do when no point sits on a tie or on the cut-off.  Every parity test asserts that from icp_ref's margins (> 1e-9 relative) before it compares.

The target normals are normals_ref.reference_normals (host, numpy eigh), rounded to f32 once and given to both sides."""
import ctypes as C

import numpy as np
import pytest

import icp_ref
import normals_ref
from helpers import BLOCKS, assert_linearized_close, expmap, lm_optimize, pose_error

pytestmark = pytest.mark.gpu
PARITY_TOL = 1e-7  # PARITY_TOL of test_knn_gicp_gpu.py
MARGIN = 1e-9
XI = np.array([0.01, -0.02, 0.015, 0.10, -0.05, 0.03])
NEARBY = np.array([0.002, -0.001, 0.003, 0.01, 0.02, -0.01])
G = np.random.default_rng(11).normal(size=(3, 3))


@pytest.fixture(scope="module")
def scan(kitti00):
    tp, sp = kitti00["target_points"], kitti00["source_points"]
    normals = np.ascontiguousarray(normals_ref.reference_normals(tp, kitti00["target_covs"]).astype(np.float32))
    return tp, sp, normals


@pytest.fixture(scope="module")
def clouds(gpu, scan):
    """the device side, built once: target with normals, source, one search structure"""
    tp, sp, normals = scan
    tgt = gpu.PointCloudGPU(tp, normals=normals)
    return tgt, gpu.PointCloudGPU(sp), gpu.KdTreeGPU(tgt)


def _conditioned(ref, delta, what):
    tie, cut = ref.margins(delta)
    print(f"[icp] {what}: smallest tie gap {tie.min():.3e}, smallest cut-off gap {cut.min():.3e} (relative, squared distances)")
    assert tie.min() > MARGIN and cut.min() > MARGIN, f"{what}: a correspondence two f64 implementations could decide differently (tie {tie.min():.2e}, cut-off {cut.min():.2e})"


def _check(gpu, tp, sp, normals, plane, delta, cutoff=1.0, what="", tree=None, tgt=None, src=None):
    """one factor on the device against icp_ref at `delta`: record, inlier count, error at a nearby pose on the stored correspondences"""
    tgt = tgt if tgt is not None else gpu.PointCloudGPU(tp, normals=normals)
    src = src if src is not None else gpu.PointCloudGPU(sp)
    f = gpu.IntegratedICPFactorGPU(0, 1, tgt, src, target_tree=tree, use_point_to_plane=plane, max_correspondence_distance=cutoff)
    ref = icp_ref.ICPFactorRef(tp, sp, normals, use_point_to_plane=plane, max_correspondence_distance=cutoff)
    _conditioned(ref, delta, what)
    L, Lr = f.linearize_delta(delta), ref.linearize(delta)
    print(f"[icp] {what}: inliers {L.num_inliers} / {Lr['num_inliers']}, error {L.error!r} / {Lr['error']!r}")
    assert_linearized_close(L, Lr, PARITY_TOL, what)
    assert f.num_inliers() == Lr["num_inliers"] == f._lib.gp_icp_factor_num_correspondences(f._h)
    for k in BLOCKS + ["error"]:
        assert np.isfinite(getattr(L, k)).all(), k
    de = delta @ expmap(NEARBY)
    e, er = f.error({0: np.eye(4), 1: de}), ref.error(de)
    assert ref.searches == 1 and abs(e - er) <= PARITY_TOL * max(er, 1e-300), (e, er)
    return f, L, Lr


@pytest.mark.parametrize("cutoff", [1.0, 0.5])
@pytest.mark.parametrize("xi", [np.zeros(6), XI], ids=["identity", "perturbed"])
@pytest.mark.parametrize("plane", [False, True], ids=["point", "plane"])
def test_linearize_matches_reference(gpu, scan, clouds, plane, xi, cutoff):
    tp, sp, normals = scan
    tgt, src, tree = clouds
    delta = expmap(xi)
    f, L, Lr = _check(gpu, tp, sp, normals, plane, delta, cutoff, f"plane={plane} cutoff={cutoff}", tree, tgt, src)
    if cutoff == 1.0 and not plane:
        assert L.num_inliers == (15231 if not np.any(xi) else 14990)  # the fixture's counts at 1 m
    # binary form: the blocks and keys of the HessianFactor (as the GICP test)
    T_t = expmap([0.03, 0.01, -0.02, 0.5, -0.2, 0.1])
    hf = f.linearize({0: T_t, 1: T_t @ delta})
    assert hf.keys == [0, 1] and set(hf.G) == {(0, 0), (0, 1), (1, 1)}
    Lb = {k: Lr[k] for k in BLOCKS}
    for got, want in [(hf.G[(0, 0)], Lb["H_target"]), (hf.G[(0, 1)], Lb["H_target_source"]), (hf.G[(1, 1)], Lb["H_source"]), (hf.g[0], -Lb["b_target"]), (hf.g[1], -Lb["b_source"])]:
        assert np.linalg.norm(got - want) <= PARITY_TOL * np.linalg.norm(want)  # (delta went through T_t^-1 T_t: 1e-16 on the pose)
    assert abs(hf.f - Lr["error"]) <= PARITY_TOL * Lr["error"]
    # fixed-target form: one key, the source blocks
    u = gpu.IntegratedICPFactorGPU(7, 3, tgt, src, target_tree=tree, use_point_to_plane=plane, max_correspondence_distance=cutoff, _fixed_target_pose=np.eye(4))
    hu = u.linearize({3: delta})
    assert u.keys() == [3] and hu.keys == [3] and set(hu.G) == {(0, 0)}
    assert np.array_equal(hu.G[(0, 0)], L.H_source) and np.array_equal(hu.g[0], -L.b_source) and hu.f == L.error  # the same kernels in the same order
    assert u.num_inliers() == Lr["num_inliers"]
    er = icp_ref.ICPFactorRef(tp, sp, normals, plane, cutoff)
    er.linearize(delta)
    de = delta @ expmap(NEARBY)
    assert abs(u.error({3: de}) - er.error(de)) <= PARITY_TOL * er.error(de)


@pytest.mark.parametrize("plane", [False, True], ids=["point", "plane"])
def test_non_orthonormal_pose_uses_the_block_as_given(gpu, scan, clouds, plane):
    tp, sp, normals = scan
    tgt, src, tree = clouds
    delta = expmap(XI)
    delta[:3, :3] = delta[:3, :3] @ (np.eye(3) + 1e-6 * G)  # orthonormal to 1e-6 only
    assert np.abs(delta[:3, :3].T @ delta[:3, :3] - np.eye(3)).max() > 1e-7
    _check(gpu, tp, sp, normals, plane, delta, 1.0, f"non-orthonormal plane={plane}", tree, tgt, src)


@pytest.mark.parametrize("n", [1, 255, 257, 1024, 1025])
def test_source_sizes_at_lane_workgroup_and_tile_edges(gpu, scan, clouds, n):
    tp, sp, normals = scan
    tgt, _, tree = clouds
    for plane in (True, False):
        _check(gpu, tp, sp[100 : 100 + n], normals, plane, expmap(XI), 1.0, f"n={n} plane={plane}", tree, tgt)


def test_target_of_one_point(gpu, scan):
    tp, _, normals = scan
    rng = np.random.default_rng(5)
    sp = (tp[:1].astype(np.float64) + rng.uniform(-0.9, 0.9, (300, 3))).astype(np.float32)  # some within 1 m of the one point, some beyond
    for plane in (False, True):
        _, L, _ = _check(gpu, tp[:1], sp, normals[:1], plane, np.eye(4), 1.0, f"one target point plane={plane}")
        assert 0 < L.num_inliers < 300


def test_every_point_beyond_the_cut_off(gpu, scan, clouds):
    tp, sp, normals = scan
    tgt, _, tree = clouds
    far = expmap([0.0, 0.0, 0.0, 0.0, 0.0, 500.0])  # half a kilometre above the scan
    for plane in (False, True):
        f, L, Lr = _check(gpu, tp, sp[:1025], normals, plane, far, 1.0, f"all beyond plane={plane}", tree, tgt)
        assert Lr["num_inliers"] == 0 and L.num_inliers == 0 and L.error == 0.0
        for k in BLOCKS:
            assert not np.any(getattr(L, k)), k
        assert f.error({0: np.eye(4), 1: far}) == 0.0


def test_duplicated_source_points_and_normals_with_a_zero_component(gpu, scan, clouds):
    tp, sp, normals = scan
    tgt, _, tree = clouds
    whole = icp_ref.ICPFactorRef(tp, sp, normals, True)
    whole.linearize(expmap(XI))
    i = int(np.flatnonzero(whole.correspondences >= 0)[0])  # a source point that has a correspondence
    dup = np.repeat(sp[i : i + 1], 300, axis=0)
    _, L, _ = _check(gpu, tp, dup, normals, True, expmap(XI), 1.0, "300 copies of one point", tree, tgt)
    assert L.num_inliers == 300
    nz = normals.copy()
    nz[::3, 0] = 0.0
    nz[1::3, 2] = 0.0
    nz[::7] = [0.0, 0.0, 1.0]
    _check(gpu, tp, sp[:4000], nz, True, expmap(XI), 1.0, "normals with zero components")


def test_two_linearises_are_bit_identical(gpu, scan, clouds):
    tgt, src, tree = clouds
    for plane in (False, True):
        for delta in (expmap(XI), expmap(XI) @ np.diag([1.0 + 1e-6, 1.0, 1.0, 1.0])):  # the rigid and the general kernels
            f = gpu.IntegratedICPFactorGPU(0, 1, tgt, src, target_tree=tree, use_point_to_plane=plane)
            A, B = f.linearize_delta(delta), f.linearize_delta(delta)
            g = gpu.IntegratedICPFactorGPU(0, 1, tgt, src, target_tree=tree, use_point_to_plane=plane)
            Cc = g.linearize_delta(delta)
            for k in BLOCKS + ["error", "num_inliers"]:
                assert np.array_equal(getattr(A, k), getattr(B, k)) and np.array_equal(getattr(A, k), getattr(Cc, k)), k
            assert A.num_inliers > 14000


def test_correspondence_update_tolerance(gpu, scan, clouds):
    tp, sp, normals = scan
    tgt, src, tree = clouds
    d1 = expmap(XI)
    d2 = d1 @ expmap([0.01, 0.0, -0.01, 0.05, 0.0, 0.02])  # 0.014 rad / 0.054 m from d1: inside (0.05 rad, 0.5 m)
    d3 = d1 @ expmap([0.06, 0.0, 0.0, 0.0, 0.0, 0.0])       # 0.06 rad from d1: outside
    f = gpu.IntegratedICPFactorGPU(0, 1, tgt, src, target_tree=tree, use_point_to_plane=True)
    ref = icp_ref.ICPFactorRef(tp, sp, normals, True)
    for h in (f, ref):
        h.set_correspondence_update_tolerance(0.05, 0.5)
    for d in (d1, d2, d3):
        _conditioned(icp_ref.ICPFactorRef(tp, sp, normals, True), d, "tolerance poses")
    assert_linearized_close(f.linearize_delta(d1), ref.linearize(d1), PARITY_TOL, "first linearise")
    L2, R2 = f.linearize_delta(d2), ref.linearize(d2)
    assert ref.searches == 1  # kept
    assert_linearized_close(L2, R2, PARITY_TOL, "inside the tolerance: the correspondences of the first pose")
    fresh = icp_ref.ICPFactorRef(tp, sp, normals, True).linearize(d2)
    assert fresh["num_inliers"] != R2["num_inliers"] and abs(fresh["error"] - R2["error"]) > 1e3 * PARITY_TOL * fresh["error"]  # the fixture tells the two apart
    assert L2.num_inliers != fresh["num_inliers"]
    # error() after a linearise that kept the correspondences still evaluates on them
    de = d2 @ expmap(NEARBY)
    assert abs(f.error({0: np.eye(4), 1: de}) - ref.error(de)) <= PARITY_TOL * ref.error(de)
    L3, R3 = f.linearize_delta(d3), ref.linearize(d3)
    assert ref.searches == 2  # searched again
    assert_linearized_close(L3, R3, PARITY_TOL, "outside the tolerance")
    assert_linearized_close(L3, icp_ref.ICPFactorRef(tp, sp, normals, True).linearize(d3), PARITY_TOL, "outside the tolerance = a fresh search")
    # only one tolerance set: the other's strict '<' fails, the search runs
    g = gpu.IntegratedICPFactorGPU(0, 1, tgt, src, target_tree=tree, use_point_to_plane=True)
    g.set_correspondence_update_tolerance(0.05, 0.0)
    g.linearize_delta(d1)
    assert_linearized_close(g.linearize_delta(d2), fresh, PARITY_TOL, "one tolerance only")
    # zero tolerances (the default): every linearise is a fresh search
    z = gpu.IntegratedICPFactorGPU(0, 1, tgt, src, target_tree=tree, use_point_to_plane=True)
    z.linearize_delta(d1)
    assert_linearized_close(z.linearize_delta(d2), fresh, PARITY_TOL, "zero tolerances")


def test_factors_share_one_tree(gpu, scan):
    tp, sp, normals = scan
    tgt = gpu.PointCloudGPU(tp, normals=normals)
    srcs = [gpu.PointCloudGPU(sp), gpu.PointCloudGPU(sp[::2].copy())]
    tree = gpu.KdTreeGPU(tgt)
    delta = expmap(XI)
    shared = [gpu.IntegratedICPFactorGPU(0, 1, tgt, s, target_tree=tree, use_point_to_plane=True) for s in srcs]
    own = [gpu.IntegratedICPFactorGPU(0, 1, tgt, s, use_point_to_plane=True) for s in srcs]
    assert shared[0].target_tree is tree and shared[1].target_tree is tree and own[0].target_tree is not own[1].target_tree
    recs = [f.linearize_delta(delta) for f in shared]
    for a, f in zip(recs, own):
        b = f.linearize_delta(delta)
        for k in BLOCKS + ["error", "num_inliers"]:
            assert np.array_equal(getattr(a, k), getattr(b, k)), k
    del shared[0]
    again = shared[0].linearize_delta(delta)  # the other factor and the tree live on
    for k in BLOCKS + ["error", "num_inliers"]:
        assert np.array_equal(getattr(again, k), getattr(recs[1], k)), k
    idx, _, nf = tree.knn_search(sp[:10], 1)
    assert (nf == 1).all() and (idx >= 0).all()
    with pytest.raises(gpu.GPError, match="target_tree was not built over the target frame's points"):
        gpu.IntegratedICPFactorGPU(0, 1, gpu.PointCloudGPU(tp[:100]), srcs[0], target_tree=tree)


def test_missing_attributes_and_null_grid(gpu, scan):
    tp, sp, _ = scan
    tgt, src = gpu.PointCloudGPU(tp), gpu.PointCloudGPU(sp)
    with pytest.raises(gpu.GPError, match="error: target frame doesn't have required attributes for icp"):
        gpu.IntegratedICPFactorGPU(0, 1, tgt, src, use_point_to_plane=True)
    with pytest.raises(gpu.GPError, match="error: target frame doesn't have required attributes for icp"):
        gpu.IntegratedPointToPlaneICPFactorGPU(0, 1, tgt, src)
    with pytest.raises(gpu.GPError, match="error: source frame doesn't have required attributes for icp"):
        gpu.IntegratedICPFactorGPU(0, 1, tgt, gpu.PointCloudGPU())
    lib = gpu.load()
    h = C.c_void_p()
    args = (tgt.ptr(tgt.points_gpu), None, tgt.size(), src.ptr(src.points_gpu), src.size(), 1.0)
    assert lib.gp_icp_factor_create(None, *args, 0, None, C.byref(h)) == 1 and not h.value  # GP_ERROR_INVALID_ARGUMENT
    tree = gpu.KdTreeGPU(tgt)
    assert lib.gp_icp_factor_create(tree._h, *args, 1, None, C.byref(h)) == 1 and not h.value  # point-to-plane without normals
    assert lib.gp_icp_factor_destroy(None) == 0 and lib.gp_icp_factor_num_correspondences(None) == 0
    assert lib.gp_icp_factor_linearize(None, None, None) == 1 and lib.gp_icp_factor_set_correspondence_update_tolerance(None, 0.1, 0.1) == 1


def test_point_to_plane_aligns_a_moved_copy(gpu, scan):
    """End to end: the source is T_gt^-1 applied to the target points (rounded to f32); a fixed-target point-to-plane factor driven by helpers.lm_optimize from
    T_gt Expmap(xi_0) must end within the alignment gate of the LM tests (0.015 rad / 0.15 m).  xi_0 = [0.02, -0.015, 0.02, 0.2, -0.1, 0.1] was chosen so that the SAME loop
    driven by icp_ref on the CPU meets the gate: run before this test was written, it ended 2.1e-8 rad / 5.1e-9 m from T_gt after 6 linearisations."""
    tp, _, normals = scan
    T_gt = expmap(XI)
    sp = ((tp.astype(np.float64) - T_gt[:3, 3]) @ T_gt[:3, :3]).astype(np.float32)
    tgt = gpu.PointCloudGPU(tp, normals=normals)
    f = gpu.IntegratedPointToPlaneICPFactorGPU(0, 1, tgt, gpu.PointCloudGPU(sp), _fixed_target_pose=np.eye(4))
    v = lm_optimize(lambda values: [f.linearize(values)], lambda values: f.error(values), {1: T_gt @ expmap([0.02, -0.015, 0.02, 0.2, -0.1, 0.1])}, [1])
    ang, trans = pose_error(v[1], T_gt)
    print(f"[icp] end to end: {ang:.3e} rad, {trans:.3e} m from the truth, {f.num_inliers()} inliers")
    assert ang < 0.015 and trans < 0.15

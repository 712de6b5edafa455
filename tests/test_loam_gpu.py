"""GPU tests of IntegratedPointToEdgeFactorGPU / IntegratedPointToPlaneFactorGPU / IntegratedLOAMFactorGPU (gp_loam_factor_*) against tests/loam_ref.py, the numpy
f64 restatement of impl/integrated_loam_factor_impl.hpp.  Parity at 1e-7, the project's gate for an f64 factor: both sides compute in f64 on the same f32 inputs.

Inputs from kitti00_dec8.npz: edge target tp[0::2], plane target tp[1::2], source sp for both parts.

Condition on the inputs, asserted before every comparison: the device search and the brute-force reference keep the same K neighbours in the same order only
when no point sits on a tie or on the cut-off, the residuals are only well conditioned when the neighbours are apart and not collinear, and the validation only
decides alike away from its threshold: every tie / cut-off gap > 1e-9 relative, |x_j - x_l| > 1e-9, the sine > 1e-6, the validation margin > 1e-9 rad."""
import ctypes as C

import numpy as np
import pytest

import loam_ref
from helpers import BLOCKS, assert_linearized_close, expmap, lm_optimize, pose_error

pytestmark = pytest.mark.gpu
PARITY_TOL = 1e-7
MARGIN = 1e-9
SINE = 1e-6
XI = np.array([0.01, -0.02, 0.015, 0.10, -0.05, 0.03])  # the XI of test_icp_gpu.py
NEARBY = np.array([0.002, -0.001, 0.003, 0.01, 0.02, -0.01])
G = np.random.default_rng(11).normal(size=(3, 3))
KINDS = ["edge", "plane", "loam"]
INLIERS = {("edge", False): 14414, ("edge", True): 14201, ("plane", False): 13898, ("plane", True): 13713}  # at 1 m, identity / XI
EDGES_REJECTED = {False: 2138, True: 1671}


@pytest.fixture(scope="module")
def scan(kitti00):
    tp, sp = kitti00["target_points"], kitti00["source_points"]
    return np.ascontiguousarray(tp[0::2]), np.ascontiguousarray(tp[1::2]), sp


@pytest.fixture(scope="module")
def clouds(gpu, scan):
    """the device side, built once: both targets with a search structure each, the source"""
    te, tpl, sp = scan
    ce, cp = gpu.PointCloudGPU(te), gpu.PointCloudGPU(tpl)
    return ce, cp, gpu.PointCloudGPU(sp), gpu.KdTreeGPU(ce), gpu.KdTreeGPU(cp)


def make_ref(kind, te, tpl, se, spl, cutoff=1.0):
    if kind == "edge":
        return loam_ref.EdgeFactorRef(te, se, cutoff)
    if kind == "plane":
        return loam_ref.PlaneFactorRef(tpl, spl, cutoff)
    return loam_ref.LOAMFactorRef(te, tpl, se, spl, cutoff)


def make_gpu(gpu, kind, ce, cp, se, spl, tree_e=None, tree_p=None, cutoff=1.0, fixed=None, keys=(0, 1)):
    if kind == "edge":
        return gpu.IntegratedPointToEdgeFactorGPU(*keys, ce, se, target_tree=tree_e, max_correspondence_distance=cutoff, _fixed_target_pose=fixed)
    if kind == "plane":
        return gpu.IntegratedPointToPlaneFactorGPU(*keys, cp, spl, target_tree=tree_p, max_correspondence_distance=cutoff, _fixed_target_pose=fixed)
    return gpu.IntegratedLOAMFactorGPU(*keys, ce, cp, se, spl, target_edges_tree=tree_e, target_planes_tree=tree_p, max_correspondence_distance=cutoff, _fixed_target_pose=fixed)


def _conditioned(ref, delta, what, validation=False):
    for part in ref.parts:
        m = part.margins(delta, validation)
        low = {k: (float(v.min()) if len(v) else np.inf) for k, v in m.items()}
        print(f"[loam] {what} K={part.K}: smallest margins {low}")
        assert low["tie"] > MARGIN and low["cut"] > MARGIN and low["length"] > MARGIN, f"{what}: a correspondence two f64 implementations could decide differently {low}"
        assert low.get("sine", 1.0) > SINE and low.get("theta", 1.0) > MARGIN, f"{what}: {low}"


def _check(gpu, kind, scan_, sp, delta, cutoff=1.0, what="", clouds_=None, validation=False):
    """one factor on the device against loam_ref at `delta`: record, inlier counts, error at a nearby pose on the stored correspondences"""
    te, tpl = scan_[0], scan_[1]
    if clouds_ is None:
        clouds_ = (gpu.PointCloudGPU(te), gpu.PointCloudGPU(tpl), None, None, None)
    ce, cp, _, tree_e, tree_p = clouds_
    src = gpu.PointCloudGPU(sp)
    f = make_gpu(gpu, kind, ce, cp, src, src, tree_e, tree_p, cutoff)
    ref = make_ref(kind, te, tpl, sp, sp, cutoff)
    if validation:
        f.set_enable_correspondence_validation(True)
        ref.set_enable_correspondence_validation(True)
    _conditioned(ref, delta, what, validation)
    L, Lr = f.linearize_delta(delta), ref.linearize(delta)
    print(f"[loam] {what}: inliers {L.num_inliers} / {Lr['num_inliers']}, error {L.error!r} / {Lr['error']!r}")
    assert_linearized_close(L, Lr, PARITY_TOL, what)
    ne, npl = f.num_correspondences()
    assert f.num_inliers() == Lr["num_inliers"] == ne + npl
    if kind == "loam":
        assert (ne, npl) == (ref.edge.evaluate(delta, False)["num_inliers"], ref.plane.evaluate(delta, False)["num_inliers"])
    for k in BLOCKS + ["error"]:
        assert np.isfinite(getattr(L, k)).all(), k
    de = delta @ expmap(NEARBY)
    e, er = f.error({0: np.eye(4), 1: de}), ref.error(de)
    assert ref.searches == 1 and abs(e - er) <= PARITY_TOL * max(er, 1e-300), (e, er)
    return f, L, Lr, ref


@pytest.mark.parametrize("cutoff", [1.0, 0.5])
@pytest.mark.parametrize("xi", [np.zeros(6), XI], ids=["identity", "perturbed"])
@pytest.mark.parametrize("kind", KINDS)
def test_linearize_matches_reference(gpu, scan, clouds, kind, xi, cutoff):
    te, tpl, sp = scan
    ce, cp, src, tree_e, tree_p = clouds
    delta = expmap(xi)
    f, L, Lr, ref = _check(gpu, kind, scan, sp, delta, cutoff, f"{kind} cutoff={cutoff}", clouds)
    if cutoff == 1.0:
        moved = bool(np.any(xi))
        want = INLIERS[("edge", moved)] + INLIERS[("plane", moved)] if kind == "loam" else INLIERS[(kind, moved)]
        assert L.num_inliers == want  # the fixture's counts at 1 m
    # binary form: the blocks and keys of the HessianFactor
    T_t = expmap([0.03, 0.01, -0.02, 0.5, -0.2, 0.1])
    hf = f.linearize({0: T_t, 1: T_t @ delta})
    assert hf.keys == [0, 1] and set(hf.G) == {(0, 0), (0, 1), (1, 1)}
    for got, want in [(hf.G[(0, 0)], Lr["H_target"]), (hf.G[(0, 1)], Lr["H_target_source"]), (hf.G[(1, 1)], Lr["H_source"]), (hf.g[0], -Lr["b_target"]), (hf.g[1], -Lr["b_source"])]:
        assert np.linalg.norm(got - want) <= PARITY_TOL * np.linalg.norm(want)  # (delta went through T_t^-1 T_t: 1e-16 on the pose)
    assert abs(hf.f - Lr["error"]) <= PARITY_TOL * Lr["error"]
    # fixed-target form: one key, the source blocks
    u = make_gpu(gpu, kind, ce, cp, src, src, tree_e, tree_p, cutoff, fixed=np.eye(4), keys=(7, 3))
    hu = u.linearize({3: delta})
    assert u.keys() == [3] and hu.keys == [3] and set(hu.G) == {(0, 0)}
    assert np.array_equal(hu.G[(0, 0)], L.H_source) and np.array_equal(hu.g[0], -L.b_source) and hu.f == L.error  # the same kernels in the same order
    assert u.num_inliers() == Lr["num_inliers"]
    de = delta @ expmap(NEARBY)
    assert abs(u.error({3: de}) - ref.error(de)) <= PARITY_TOL * ref.error(de)


@pytest.mark.parametrize("kind", KINDS)
def test_non_orthonormal_pose_uses_the_block_as_given(gpu, scan, clouds, kind):
    delta = expmap(XI)
    delta[:3, :3] = delta[:3, :3] @ (np.eye(3) + 1e-6 * G)  # orthonormal to 1e-6 only: the general kernels
    assert np.abs(delta[:3, :3].T @ delta[:3, :3] - np.eye(3)).max() > 1e-7
    _check(gpu, kind, scan, scan[2], delta, 1.0, f"non-orthonormal {kind}", clouds)


@pytest.mark.parametrize("n", [1, 255, 257, 1024, 1025])
def test_source_sizes_at_lane_workgroup_and_tile_edges(gpu, scan, clouds, n):
    for kind in KINDS:
        _check(gpu, kind, scan, scan[2][100 : 100 + n], expmap(XI), 1.0, f"n={n} {kind}", clouds)


@pytest.mark.parametrize("m", [1, 2, 3])
def test_targets_of_one_two_and_three_points(gpu, scan, m):
    """fewer than K target points: no correspondence at all, an all-zero record, error 0; exactly K: the factor works"""
    te, tpl, _ = scan
    rng = np.random.default_rng(5)
    sp = (te[:1].astype(np.float64) + rng.uniform(-0.4, 0.4, (300, 3))).astype(np.float32)
    tgt = np.ascontiguousarray(te[:1] + np.array([[0.0, 0.0, 0.0], [0.31, 0.05, 0.02], [0.04, 0.29, -0.03]], np.float32)[:m])  # three points apart, not collinear
    for kind, K in [("edge", 2), ("plane", 3)]:
        f, L, Lr, _ = _check(gpu, kind, (tgt, tgt), sp, np.eye(4), 1.0, f"{m} target points {kind}")
        if m < K:
            assert Lr["num_inliers"] == 0 and L.num_inliers == 0 and L.error == 0.0
            for k in BLOCKS:
                assert not np.any(getattr(L, k)), k
            assert f.error({0: np.eye(4), 1: np.eye(4)}) == 0.0
        else:
            assert L.num_inliers == 300


def test_every_point_beyond_the_cut_off(gpu, scan, clouds):
    far = expmap([0.0, 0.0, 0.0, 0.0, 0.0, 500.0])  # half a kilometre above the scan
    for kind in KINDS:
        f, L, Lr, _ = _check(gpu, kind, scan, scan[2][:1025], far, 1.0, f"all beyond {kind}", clouds)
        assert Lr["num_inliers"] == 0 and L.num_inliers == 0 and L.error == 0.0
        for k in BLOCKS:
            assert not np.any(getattr(L, k)), k
        assert f.error({0: np.eye(4), 1: far}) == 0.0


def test_duplicated_source_points(gpu, scan, clouds):
    te, tpl, sp = scan
    whole = loam_ref.LOAMFactorRef(te, tpl, sp, sp)
    whole.linearize(expmap(XI))
    i = int(np.flatnonzero((whole.edge.correspondences[:, 0] >= 0) & (whole.plane.correspondences[:, 0] >= 0))[0])
    dup = np.repeat(sp[i : i + 1], 300, axis=0)
    _, L, _, _ = _check(gpu, "loam", scan, dup, expmap(XI), 1.0, "300 copies of one point", clouds)
    assert L.num_inliers == 600


def test_a_duplicated_target_point_gives_a_non_finite_error_on_both_sides(gpu, scan):
    """x_j = x_l (edge) and a degenerate triple (plane) are not guarded in the reference: the division yields non-finite values.  The condition above cannot hold
    here (the duplicate IS a tie), so only the non-finiteness and the return code are compared."""
    te = scan[0][:200]
    tgt = np.ascontiguousarray(np.concatenate([te, te[17:18], te[17:18] + np.array([[0.05, 0.02, 0.01]], np.float32)]))  # (and a third point well within the cut-off)
    sp = (te[17:18].astype(np.float64) + np.array([[0.001, 0.002, -0.001]])).astype(np.float32)  # beside the duplicated point: its two nearest are the copies
    for kind in ("edge", "plane"):
        ref = make_ref(kind, tgt, tgt, sp, sp)
        Lr = ref.linearize(np.eye(4))
        c = gpu.PointCloudGPU(tgt)
        f = make_gpu(gpu, kind, c, c, gpu.PointCloudGPU(sp), gpu.PointCloudGPU(sp))
        L = f.linearize_delta(np.eye(4))  # (GP_OK: a failure would raise)
        assert Lr["num_inliers"] == 1 == L.num_inliers
        assert not np.isfinite(Lr["error"]) and not np.isfinite(L.error), (kind, Lr["error"], L.error)
        assert not np.isfinite(f.error({0: np.eye(4), 1: expmap(NEARBY)}))


@pytest.mark.parametrize("xi", [np.zeros(6), XI], ids=["identity", "perturbed"])
def test_correspondence_validation(gpu, scan, clouds, xi):
    te, tpl, sp = scan
    delta = expmap(xi)
    f, L_on, R_on, ref = _check(gpu, "loam", scan, sp, delta, 1.0, "validation on", clouds, validation=True)
    assert ref.rejected[0] == EDGES_REJECTED[bool(np.any(xi))]
    _, L_off, R_off, _ = _check(gpu, "loam", scan, sp, delta, 1.0, "validation off", clouds)
    assert L_off.num_inliers - L_on.num_inliers == sum(ref.rejected)
    assert abs(R_on["error"] - R_off["error"]) > 1e3 * PARITY_TOL * R_off["error"]  # the fixture tells the two apart
    # idempotent, and switched off again the next linearise searches afresh
    assert f.linearize_delta(delta).error == L_on.error
    f.set_enable_correspondence_validation(False)
    assert f.linearize_delta(delta).error == L_off.error


def test_correspondence_update_tolerance(gpu, scan, clouds):
    te, tpl, sp = scan
    ce, cp, src, tree_e, tree_p = clouds
    d1 = expmap(XI)
    d2 = d1 @ expmap([0.01, 0.0, -0.01, 0.05, 0.0, 0.02])  # 0.014 rad / 0.054 m from d1: inside (0.05 rad, 0.5 m)
    d3 = d1 @ expmap([0.06, 0.0, 0.0, 0.0, 0.0, 0.0])       # 0.06 rad from d1: outside
    f = make_gpu(gpu, "loam", ce, cp, src, src, tree_e, tree_p)
    ref = make_ref("loam", te, tpl, sp, sp)
    for h in (f, ref):
        h.set_correspondence_update_tolerance(0.05, 0.5)
        h.set_enable_correspondence_validation(True)  # (runs behind kept correspondences too: idempotent)
    for d in (d1, d2, d3):
        _conditioned(make_ref("loam", te, tpl, sp, sp), d, "tolerance poses", validation=True)
    assert_linearized_close(f.linearize_delta(d1), ref.linearize(d1), PARITY_TOL, "first linearise")
    L2, R2 = f.linearize_delta(d2), ref.linearize(d2)
    assert ref.searches == 1  # kept
    assert_linearized_close(L2, R2, PARITY_TOL, "inside the tolerance: the correspondences of the first pose")
    fresh_ref = make_ref("loam", te, tpl, sp, sp)
    fresh_ref.set_enable_correspondence_validation(True)
    fresh = fresh_ref.linearize(d2)
    assert fresh["num_inliers"] != R2["num_inliers"] and abs(fresh["error"] - R2["error"]) > 1e3 * PARITY_TOL * fresh["error"]  # the fixture tells the two apart
    assert L2.num_inliers != fresh["num_inliers"]
    de = d2 @ expmap(NEARBY)
    assert abs(f.error({0: np.eye(4), 1: de}) - ref.error(de)) <= PARITY_TOL * ref.error(de)  # error() after a linearise that kept them evaluates on them
    L3, R3 = f.linearize_delta(d3), ref.linearize(d3)
    assert ref.searches == 2  # searched again
    assert_linearized_close(L3, R3, PARITY_TOL, "outside the tolerance")
    # only one tolerance set: the other's strict '<' fails, the search runs; zero tolerances (the default) likewise
    for tol in [(0.05, 0.0), (0.0, 0.0)]:
        g = make_gpu(gpu, "loam", ce, cp, src, src, tree_e, tree_p)
        g.set_enable_correspondence_validation(True)
        g.set_correspondence_update_tolerance(*tol)
        g.linearize_delta(d1)
        assert_linearized_close(g.linearize_delta(d2), fresh, PARITY_TOL, f"tolerances {tol}")


def test_two_linearises_are_bit_identical(gpu, clouds):
    ce, cp, src, tree_e, tree_p = clouds
    for kind in KINDS:
        for delta in (expmap(XI), expmap(XI) @ np.diag([1.0 + 1e-6, 1.0, 1.0, 1.0])):  # the rigid and the general kernels
            f = make_gpu(gpu, kind, ce, cp, src, src, tree_e, tree_p)
            A, B = f.linearize_delta(delta), f.linearize_delta(delta)
            Cc = make_gpu(gpu, kind, ce, cp, src, src, tree_e, tree_p).linearize_delta(delta)
            for k in BLOCKS + ["error", "num_inliers"]:
                assert np.array_equal(getattr(A, k), getattr(B, k)) and np.array_equal(getattr(A, k), getattr(Cc, k)), k
            assert A.num_inliers > 13000


def test_combined_record_is_the_edge_record_plus_the_plane_record(gpu, clouds):
    ce, cp, src, tree_e, tree_p = clouds
    delta = expmap(XI)
    e, p, l = (make_gpu(gpu, k, ce, cp, src, src, tree_e, tree_p).linearize_delta(delta) for k in KINDS)
    for k in BLOCKS + ["error", "num_inliers"]:
        assert np.array_equal(getattr(l, k), getattr(e, k) + getattr(p, k)), k  # added in that order in f64


def test_factors_share_one_tree(gpu, scan):
    te, tpl, sp = scan
    ce, cp = gpu.PointCloudGPU(te), gpu.PointCloudGPU(tpl)
    srcs = [gpu.PointCloudGPU(sp), gpu.PointCloudGPU(sp[::2].copy())]
    tree_e, tree_p = gpu.KdTreeGPU(ce), gpu.KdTreeGPU(cp)
    delta = expmap(XI)
    shared = [make_gpu(gpu, "loam", ce, cp, s, s, tree_e, tree_p) for s in srcs]
    own = [make_gpu(gpu, "loam", ce, cp, s, s) for s in srcs]
    assert shared[0].target_edges_tree is tree_e and shared[1].target_planes_tree is tree_p and own[0].target_edges_tree is not own[1].target_edges_tree
    recs = [f.linearize_delta(delta) for f in shared]
    for a, f in zip(recs, own):
        b = f.linearize_delta(delta)
        for k in BLOCKS + ["error", "num_inliers"]:
            assert np.array_equal(getattr(a, k), getattr(b, k)), k
    del shared[0]
    again = shared[0].linearize_delta(delta)  # the other factor and the trees live on
    for k in BLOCKS + ["error", "num_inliers"]:
        assert np.array_equal(getattr(again, k), getattr(recs[1], k)), k
    idx, _, nf = tree_e.knn_search(sp[:10], 1)
    assert (nf == 1).all() and (idx >= 0).all()
    with pytest.raises(gpu.GPError, match="target_tree was not built over the target frame's points"):
        gpu.IntegratedPointToEdgeFactorGPU(0, 1, gpu.PointCloudGPU(te[:100]), srcs[0], target_tree=tree_e)
    with pytest.raises(gpu.GPError, match="target_tree was not built over the target frame's points"):
        gpu.IntegratedLOAMFactorGPU(0, 1, ce, cp, srcs[0], srcs[0], target_edges_tree=tree_e, target_planes_tree=tree_e)


def test_missing_attributes_and_null_handles(gpu, scan):
    te, tpl, sp = scan
    tgt, src, empty = gpu.PointCloudGPU(tpl), gpu.PointCloudGPU(sp), gpu.PointCloudGPU()
    with pytest.raises(gpu.GPError, match="error: target frame doesn't have required attributes for loam"):
        gpu.IntegratedPointToPlaneFactorGPU(0, 1, empty, src)
    with pytest.raises(gpu.GPError, match="error: source frame doesn't have required attributes for loam"):
        gpu.IntegratedPointToPlaneFactorGPU(0, 1, tgt, empty)
    for a, b in [(empty, src), (tgt, empty)]:
        with pytest.raises(gpu.GPError, match="error: target or source points has not been allocated!!"):
            gpu.IntegratedPointToEdgeFactorGPU(0, 1, a, b)
    with pytest.raises(gpu.GPError, match="error: target or source points has not been allocated!!"):
        gpu.IntegratedLOAMFactorGPU(0, 1, empty, tgt, src, src)
    with pytest.raises(gpu.GPError, match="error: source frame doesn't have required attributes for loam"):
        gpu.IntegratedLOAMFactorGPU(0, 1, tgt, tgt, src, empty)
    lib = gpu.load()
    h = C.c_void_p()
    tree = gpu.KdTreeGPU(tgt)
    assert lib.gp_loam_factor_create(tree._h, None, tgt.size(), src.ptr(src.points_gpu), src.size(), None, None, 0, None, 0, None, C.byref(h)) == 1 and not h.value
    assert lib.gp_loam_factor_create(None, None, 0, None, 0, None, None, 0, None, 0, None, C.byref(h)) == 1 and not h.value
    f = gpu.IntegratedPointToPlaneFactorGPU(0, 1, tgt, src, target_tree=tree)
    with pytest.raises(gpu.GPError):
        f.set_max_correspondence_distance(1.0, 0.0)
    assert lib.gp_loam_factor_linearize(None, None, None) == 1 and lib.gp_loam_factor_destroy(None) == 0


def test_loam_aligns_a_moved_copy(gpu, scan):
    """End to end: the sources are T_gt^-1 applied to the target points (rounded to f32), even points as edges and odd ones as planes; a fixed-target combined
    factor driven by helpers.lm_optimize from T_gt Expmap(xi_0) must end within the alignment gate of the LM tests (0.015 rad / 0.15 m).
    xi_0 = [0.02, -0.015, 0.02, 0.2, -0.1, 0.1] was chosen so that the SAME loop driven by loam_ref on the CPU meets the gate: run before this test was written, it
    ended 0.0 rad (below the arccos resolution) / 5.4e-9 m from T_gt after 7 linearisations."""
    te, tpl, _ = scan
    T_gt = expmap(XI)
    se, spl = (((t.astype(np.float64) - T_gt[:3, 3]) @ T_gt[:3, :3]).astype(np.float32) for t in (te, tpl))
    f = gpu.IntegratedLOAMFactorGPU(0, 1, gpu.PointCloudGPU(te), gpu.PointCloudGPU(tpl), gpu.PointCloudGPU(se), gpu.PointCloudGPU(spl), _fixed_target_pose=np.eye(4))
    v = lm_optimize(lambda values: [f.linearize(values)], lambda values: f.error(values), {1: T_gt @ expmap([0.02, -0.015, 0.02, 0.2, -0.1, 0.1])}, [1])
    ang, trans = pose_error(v[1], T_gt)
    print(f"[loam] end to end: {ang:.3e} rad, {trans:.3e} m from the truth, {f.num_inliers()} inliers")
    assert ang < 0.015 and trans < 0.15

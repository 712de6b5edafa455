"""GPU sweep of the three factor families (VGICP, GICP, ICP) over the part of the input domain the scan-pair tests never enter: a sensor hundreds to thousands of
metres from the map's origin, rotations near pi, both clouds far from the origin, and other units of length.  Inputs and f64 references: tests/factor_domain_ref.py
(self-checked on the CPU by tests/test_factor_domain_ref_cpu.py).

Contract: for a rigid relative pose with |t| <= 10 km and f32 source coordinates within 200 m every family meets the 1e-5 north-star gate on
every block; the default family meets PARITY_TOL wherever it takes its fast path (the 29 f32 sums + adjoint expansion).  The library sends a pose whose translation
exceeds GP_TUNE_FAR_POSE_RATIO times the source cloud's extent to the explicit-J_s sums instead, because the expansion H_s = Ad^T H_t Ad cancels about (|t| / |p|)^2
of the f32 rounding in H_t; gp_vgicp_factor_takes_rigid_path says which path a pose takes.  Asserted: the project's own tolerance (PARITY_TOL / MIXED_TOL for the
families with f32 outer products, F64_TOL for the all-f64 ones, the GICP / ICP tests' 1e-7) at |t| = 0, in the controls and wherever the fast path runs, the gate
everywhere else.  The metric is helpers.assert_linearized_close: every block norm-wise, the error, the inlier count.  Each test prints its worst block figure.

Measured on one MI355X (worst block, H_source): the rigid sums held at every distance read 3.2e-8 at 0 m, 3.1e-6 at 100 m, 3.1e-4 at 1000 m and 2.6e-2 at 10 km for
the default family (families 2 and 8: 1.3e-4 and 1.6e-2 at 1 and 10 km) -- what case (a) would report without the routing; routed, every family stays below 3e-8,
and GICP / ICP below 4e-10."""
import ctypes as C

import numpy as np
import pytest

import factor_domain_ref as fd
import icp_ref
import oracle
from helpers import assert_linearized_close, expmap

pytestmark = pytest.mark.gpu
PARITY_TOL = MIXED_TOL = 1e-6  # tests/test_vgicp_gpu.py
F64_TOL = 1e-7                 # tests/test_vgicp_gpu.py; also PARITY_TOL of test_knn_gicp_gpu.py and test_icp_gpu.py
GATE = 1e-5                    # the north-star gate
KERNEL, FAR_POSE_RATIO = 0, 25  # GP_TUNE_KERNEL, GP_TUNE_FAR_POSE_RATIO
FAMILIES = [(0, F64_TOL), (2, MIXED_TOL), (3, F64_TOL), (8, MIXED_TOL), (12, MIXED_TOL)]
CASES_A = [(t, r) for t in fd.DISTANCES for r in fd.ROTATIONS]
_CACHE = {}


def _case(kind, *args):
    """inputs, poses and the f64 VGICP reference of one case, computed once and shared"""
    key = (kind,) + args
    if key not in _CACHE:
        d, delta, delta_eval, dropped = getattr(fd, kind)(*args)
        assert dropped <= fd.DROP_CAP
        ref, err_eval = fd.vgicp_reference(d, delta, delta_eval)
        assert ref["num_inliers"] > 2000
        _CACHE[key] = (d, delta, delta_eval, ref, err_eval)
    return _CACHE[key]


_DEVICE = {}


def _device(gpu, key, d):
    """target cloud (with normals), source cloud and voxel map of placed inputs on the device, built once per case"""
    if key not in _DEVICE:
        tgt = gpu.PointCloudGPU(d["target_points"], d["target_covs"], normals=d["target_normals"])
        src = gpu.PointCloudGPU(d["source_points"], d["source_covs"])
        vm = gpu.GaussianVoxelMapGPU(d["leaf"], target_points_drop_rate=0.0)
        vm.insert(tgt)
        _DEVICE[key] = (tgt, src, vm)
    return _DEVICE[key]


def _factor(gpu, vm, src, family):
    f = gpu.IntegratedVGICPFactorGPU(0, 1, vm, src)
    f.set_tuning(KERNEL, family)
    return f


def _fast_path(gpu, f, delta):
    out = C.c_int(-1)
    gpu._capi.check(f._lib.gp_vgicp_factor_takes_rigid_path(f._h, gpu.types._pose16(delta), C.byref(out)), "takes_rigid_path")
    return out.value == 1


def _linearize(gpu, f, delta):
    rec = gpu._capi.Linearized6()
    gpu._capi.check(f._lib.gp_vgicp_factor_linearize(f._h, gpu.types._pose16(delta), C.byref(rec)), "linearize")
    return gpu.LinearizedSystem6(rec)


def _error(gpu, f, delta, delta_eval):
    out = C.c_double()
    gpu._capi.check(f._lib.gp_vgicp_factor_compute_error(f._h, gpu.types._pose16(delta), gpu.types._pose16(delta_eval), C.byref(out)), "compute_error")
    return out.value


def _report(what, L, ref, tol, path):
    worst, block, errs = fd.worst_block(L, ref)
    print(f"[domain] {what}: path {path}, worst block {block} {worst:.3e} (H_source {errs['H_source']:.3e}, b_source {errs['b_source']:.3e}, H_target {errs['H_target']:.3e}), "
          f"error {abs(L.error - ref['error']) / ref['error']:.3e}, inliers {L.num_inliers} / {ref['num_inliers']}, asserted at {tol:.0e}")


def _check_vgicp(gpu, f, case, family_tol, far, what):
    d, delta, delta_eval, ref, err_eval = case
    fast = _fast_path(gpu, f, delta)
    tol = family_tol if (fast or not far) else GATE
    L = _linearize(gpu, f, delta)
    _report(what, L, ref, tol, "rigid sums + adjoint" if fast else "explicit J_s")
    assert_linearized_close(L, ref, tol, what)
    e = _error(gpu, f, delta, delta_eval)
    print(f"[domain] {what}: error at the evaluation pose {abs(e - err_eval) / err_eval:.3e}")
    assert abs(e - err_eval) <= tol * err_eval, (e, err_eval)
    return fast


@pytest.mark.parametrize("family,tol", FAMILIES)
@pytest.mark.parametrize("distance,rotation", CASES_A)
def test_scan_to_map(gpu, distance, rotation, family, tol):
    """(a) the target in a world frame, the source in its sensor frame: every kernel family, linearise and error evaluation"""
    case = _case("scan_to_map", distance, rotation)
    _, src, vm = _device(gpu, ("a", distance, rotation), case[0])
    fast = _check_vgicp(gpu, _factor(gpu, vm, src, family), case, tol, distance > 0, f"(a) {distance:g} m {rotation} family {family}")
    assert fast or distance > 0, "a pose at the origin leaves the fast path"


@pytest.mark.parametrize("distance,rotation", CASES_A)
def test_scan_to_map_rigid_sums_figures(gpu, distance, rotation):
    """the default family held on its rigid sums at every distance (GP_TUNE_FAR_POSE_RATIO = 0: no pose counts as far): the figures behind DESIGN.md section 2's
    table, printed.  Asserted: the project tolerance at the origin only -- what the 29 f32 sums lose further out is what the routing exists for."""
    d, delta, _, ref, _ = _case("scan_to_map", distance, rotation)
    _, src, vm = _device(gpu, ("a", distance, rotation), d)
    f = _factor(gpu, vm, src, 12)
    f.set_tuning(FAR_POSE_RATIO, 0)
    assert _fast_path(gpu, f, delta)
    L = _linearize(gpu, f, delta)
    _report(f"(a) rigid sums held, {distance:g} m {rotation}", L, ref, MIXED_TOL if distance == 0 else float("inf"), "rigid sums + adjoint")
    assert L.num_inliers == ref["num_inliers"]
    if distance == 0:
        assert_linearized_close(L, ref, MIXED_TOL, "rigid sums at the origin")


@pytest.mark.parametrize("first,second", [((0.0, "0.4rad"), (100.0, "pi-1e-3")), ((1000.0, "0.4rad"), (10000.0, "pi-1e-3"))])
def test_scan_to_map_batch(gpu, first, second):
    """(a) two factors with different W in one synchronous batch call (default family; the fused finalize where the batch takes its fast path)"""
    cases = [_case("scan_to_map", *first), _case("scan_to_map", *second)]
    factors = []
    for (t, r), c in zip((first, second), cases):
        _, src, vm = _device(gpu, ("a", t, r), c[0])
        factors.append(gpu.IntegratedVGICPFactorGPU(0, 1, vm, src))
    lib = gpu.load()
    arr = (C.c_void_p * 2)(*[f._h.value for f in factors])
    batch = C.c_void_p()
    gpu._capi.check(lib.gp_vgicp_batch_create(arr, 2, None, C.byref(batch)), "batch")
    try:
        P = np.ascontiguousarray(np.stack([c[1].T.reshape(16) for c in cases]))
        fast = C.c_int(-1)
        gpu._capi.check(lib.gp_vgicp_batch_takes_rigid_path(batch, P.ctypes.data, C.byref(fast)), "takes_rigid_path")
        assert fast.value == int(all(_fast_path(gpu, f, c[1]) for f, c in zip(factors, cases)))  # one far pose sends the whole batch to the explicit sums
        out = np.zeros((2, 122))
        gpu._capi.check(lib.gp_vgicp_batch_linearize(batch, P.ctypes.data, out.ctypes.data), "linearize")
        for k, ((t, r), c) in enumerate(zip((first, second), cases)):
            tol = MIXED_TOL if (fast.value == 1 or t == 0) else GATE
            L = gpu.LinearizedSystem6.from_doubles(out[k])
            _report(f"(a) batch, factor {k}: {t:g} m {r}", L, c[3], tol, "rigid sums + adjoint, fused finalize" if fast.value == 1 else "explicit J_s")
            assert_linearized_close(L, c[3], tol, f"batch factor {k}")
    finally:
        lib.gp_vgicp_batch_destroy(batch)


@pytest.mark.parametrize("distance,rotation", CASES_A)
def test_scan_to_map_general_pose(gpu, distance, rotation):
    """(a) a rotation block off by 1e-6 (as test_rigid_and_general_pose_paths): the explicit-J_s sums, against the reference on the block as given"""
    d, delta, _, _, _ = _case("scan_to_map", distance, rotation)
    skew = delta.copy()
    skew[:3, :3] = skew[:3, :3] @ (np.eye(3) + 1e-6 * np.array([[1.0, 0.3, 0.0], [0.0, -0.5, 0.2], [0.1, 0.0, 0.7]]))
    d2, dropped = fd.with_margin(d, skew)
    assert dropped <= fd.DROP_CAP
    ref, _ = fd.vgicp_reference(d2, skew)
    src = gpu.PointCloudGPU(d2["source_points"], d2["source_covs"])
    _, _, vm = _device(gpu, ("a", distance, rotation), d)
    f = _factor(gpu, vm, src, 12)
    assert not _fast_path(gpu, f, skew)
    L = _linearize(gpu, f, skew)
    tol = MIXED_TOL if distance == 0 else GATE
    _report(f"(a) general pose {distance:g} m {rotation}", L, ref, tol, "explicit J_s")
    assert_linearized_close(L, ref, tol, "general pose")


@pytest.mark.parametrize("distance,rotation", CASES_A)
def test_scan_to_map_device_poses(gpu, distance, rotation):
    """(a) the values in device memory: set_values and linearize on a two-pose graph, the record read out of gp_lm_graph_records"""
    d, delta, _, ref, _ = _case("scan_to_map", distance, rotation)
    _, src, vm = _device(gpu, ("a", distance, rotation), d)
    f = gpu.IntegratedVGICPFactorGPU(0, 1, vm, src)
    fast = _fast_path(gpu, f, delta)
    lm = gpu.LevenbergMarquardtGraphGPU([f], [(0, 1)], 2, fixed=(0,))
    try:
        lm.set_values(np.stack([np.eye(4), delta]))  # (the relative pose is delta to the last bit: the inverse of the identity)
        lm.linearize()
        L = gpu.LinearizedSystem6.from_doubles(lm.records().cpu().numpy()[0])
    finally:
        lm.close()
    tol = MIXED_TOL if (fast or distance == 0) else GATE
    _report(f"(a) device poses {distance:g} m {rotation}", L, ref, tol, "rigid sums + adjoint" if fast else "explicit J_s")
    assert_linearized_close(L, ref, tol, "device poses")
    # the graph chooses as the host-pose entry points do: the same kernels on the same operands, the same record
    Lh = gpu.LinearizedSystem6.from_doubles(_issue(gpu, f, delta))
    for k in ("H_target", "H_source", "H_target_source", "b_target", "b_source"):
        assert np.array_equal(getattr(L, k), getattr(Lh, k)), k


def _issue(gpu, f, delta):
    """the asynchronous host-pose entry point of a batch of one (no fused finalize, as the graph's launches)"""
    import torch

    lib = gpu.load()
    batch = C.c_void_p()
    gpu._capi.check(lib.gp_vgicp_batch_create((C.c_void_p * 1)(f._h.value), 1, None, C.byref(batch)), "batch")
    try:
        dev = torch.zeros(122, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        P = np.ascontiguousarray(delta.T.reshape(16))
        gpu._capi.check(lib.gp_vgicp_batch_issue_linearize(batch, P.ctypes.data, C.c_void_p(dev.data_ptr())), "issue")
        gpu._capi.check(lib.gp_vgicp_batch_sync(batch), "sync")
        return dev.cpu().numpy()
    finally:
        lib.gp_vgicp_batch_destroy(batch)


@pytest.mark.parametrize("family,tol", FAMILIES)
def test_both_clouds_far(gpu, family, tol):
    """(b) control: source and target both 1000 m out, the relative pose near identity -- H_source is legitimately large, nothing cancels, the fast path runs and
    meets the project tolerance"""
    case = _case("both_far")
    _, src, vm = _device(gpu, ("b",), case[0])
    fast = _check_vgicp(gpu, _factor(gpu, vm, src, family), case, tol, False, f"(b) both far, family {family}")
    assert fast


@pytest.mark.parametrize("family,tol", [(12, MIXED_TOL), (3, F64_TOL)])
@pytest.mark.parametrize("scale", fd.SCALES)
def test_units(gpu, scale, family, tol):
    """(c) the whole scene in centimetres, metres and hundreds of metres at the origin"""
    case = _case("scaled", scale)
    _, src, vm = _device(gpu, ("c", scale), case[0])
    fast = _check_vgicp(gpu, _factor(gpu, vm, src, family), case, tol, False, f"(c) scale {scale:g}, family {family}")
    assert fast


# ---- (d) GICP and ICP: the shared core of gp_corr_factors.hip -------------------------------------------------------------------------------------------------------
CASES_D = [(t, r) for t in (0.0, 1000.0, 10000.0) for r in fd.ROTATIONS]
NEARBY = np.array([0.002, -0.001, 0.003, 0.01, 0.02, -0.01])


def _conditioned(d, delta, what):
    """test_icp_gpu.py's condition: no source point on a tie or on the cut-off of the 1-NN search"""
    tie, cut = icp_ref.ICPFactorRef(d["target_points"], d["source_points"]).margins(delta)
    assert tie.min() > fd.MARGIN and cut.min() > fd.MARGIN, f"{what}: tie {tie.min():.2e}, cut-off {cut.min():.2e}"


@pytest.mark.parametrize("distance,rotation", CASES_D)
def test_gicp_scan_to_map(gpu, distance, rotation):
    d, delta, _, _, _ = _case("scan_to_map", distance, rotation)
    what = f"(d) gicp {distance:g} m {rotation}"
    _conditioned(d, delta, what)
    tgt, src, _ = _device(gpu, ("a", distance, rotation), d)
    f = gpu.IntegratedGICPFactorGPU(0, 1, tgt, src)
    fo = oracle.OracleGICPFactor(d["target_points"], d["target_covs"], d["source_points"], d["source_covs"], 4)
    L, Lo = f.linearize_delta(delta), fo.linearize(delta)
    tol = F64_TOL if distance == 0 else GATE
    ref = {k: getattr(Lo, k) for k in ("H_target", "H_source", "H_target_source", "b_target", "b_source", "error", "num_inliers")}
    _report(what, L, ref, tol, "f64 sums + adjoint")
    assert Lo.num_inliers > 2000
    assert_linearized_close(L, Lo, tol, what)
    de = delta @ expmap(NEARBY)
    e, eo = f.error({0: np.eye(4), 1: de}), fo.evaluate(de).error
    assert abs(e - eo) <= tol * eo, (e, eo)


@pytest.mark.parametrize("plane", [False, True], ids=["point", "plane"])
@pytest.mark.parametrize("distance,rotation", CASES_D)
def test_icp_scan_to_map(gpu, distance, rotation, plane):
    d, delta, _, _, _ = _case("scan_to_map", distance, rotation)
    what = f"(d) icp plane={plane} {distance:g} m {rotation}"
    _conditioned(d, delta, what)
    tgt, src, _ = _device(gpu, ("a", distance, rotation), d)
    f = gpu.IntegratedICPFactorGPU(0, 1, tgt, src, use_point_to_plane=plane)
    ref = icp_ref.ICPFactorRef(d["target_points"], d["source_points"], d["target_normals"], use_point_to_plane=plane)
    L, Lr = f.linearize_delta(delta), ref.linearize(delta)
    tol = F64_TOL if distance == 0 else GATE
    _report(what, L, Lr, tol, "f64 sums + adjoint")
    assert Lr["num_inliers"] > 2000
    assert_linearized_close(L, Lr, tol, what)
    de = delta @ expmap(NEARBY)
    e, er = f.error({0: np.eye(4), 1: de}), ref.error(de)
    assert abs(e - er) <= tol * er, (e, er)

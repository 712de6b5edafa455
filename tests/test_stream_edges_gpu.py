"""vgicp_stream_kernel (csrc/gp_vgicp_stream.hpp, family 12) held to an f64 reference at every plan geometry and per-wave stream length of
tests/stream_plan_ref.py's case table: waves of 0, 1, 2, 3 chunks beside longer ones inside a planned launch, streams of 16, 32 and 64 chunks through the same 32 f32
per-lane sums (an 8 M-point source streams ~30), skewed plans of two and three rounds (at the default cap and under a cap; the smallest, gx = 33), refused skews, XCD shares of a half and one and a half, tails of 0 / 1 / 63
points, and GP_TUNE_TILE_CHUNKS 1 .. 16 on fixed tiles.  tests/test_stream_plan_ref_cpu.py asserts that the table contains all of that.

The plan changes only WHICH points a wave adds up, so one reference per (cloud, pose) serves every geometry of that cloud: oracle/vgicp_oracle_np.py (all f64, numpy; through
factor_domain_ref.vgicp_reference), computed once per n and kept.  Inputs: synthetic.make_c2_workload(n, 64 000, seed 7) at 0.5 m -- 79 % of the source are inliers (asserted
on the reference) -- and ONE voxel map for the whole file (the target does not depend on n).  Pose: T_true o expmap of the perturbation of tests/test_vgicp_gpu.py.

Asserted per geometry: linearise and error evaluation inside MIXED_TOL = 1e-6 of the reference on every block (the project's contract), the
reference's inlier count, identical bits on a second call.  Printed per geometry ("[stream] ..."): the worst block.

Measured on an MI355X (this file's own output):
  planned launches, worst block of the linearise (error evaluation <= 3.1e-9 everywhere, inlier counts equal everywhere):
    65,535 points, fixed tiles (control)                                       5.8e-9 (H_target)
    65,536 / 65,537 / 65,599 points, 8 workgroups, 31 - 33 chunks per wave     1.7e-8 / 7.0e-9 / 1.4e-8 (b_source)
    the same, 16 workgroups, 15 - 17 chunks per wave                           9.2e-9 / 8.7e-9 / 9.6e-9
    the same, 64 workgroups, 3 - 5 chunks per wave                             6.8e-9 / 6.2e-9 / 7.6e-9
    the same, 256 = 1024 workgroups (the plan needs no more), 0 - 2 chunks     6.4e-9 / 6.0e-9 / 6.1e-9
    131,072 points, 8 workgroups, 63 - 65 chunks per wave                      5.3e-9 (b_target)
    140,011 / 163,903 / 196,607 points, 256 workgroups, 1 - 4 chunks per wave  7.4e-9 / 6.3e-9 / 5.6e-9
    default cap, the balance sweep:
      120,925 points, gx = 60: 0 / 50 / 150 / 400 (skewed) / 1000 (refused)    6.9e-9 / 6.9e-9 / 7.0e-9 / 7.1e-9 / 6.9e-9
      196,607 points, gx = 96, three rounds: 0 / 50 / 150 (skewed) / 400       6.3e-9 / 6.6e-9 / 6.5e-9 / 6.3e-9
      67,429 points, gx = 33, every balance (all refused: one flat plan)       6.9e-9
      198,719 points, gx = 97, every balance (all refused: one flat plan)      5.6e-9
    198,719 points, 264 workgroups at 40: the smallest skewed plan, gx = 33    6.5e-9 (H_source)
    198,719 points, skewed: 304 / 728 / 768 workgroups, 512 at 0 ... 1000      5.5e-9 - 6.6e-9
    XCD weights 500 / 1500 (four geometries)                                   6.0e-9 - 7.1e-9
  plan against plan, 198,719 points, 16 cases = 12 different plans: largest difference 2.5e-9 (H_source, 768 workgroups at 50 against 512 at 1000)
  surface validation (41,255 of 65,599 and 103,033 of 163,903 points kept; packed and unpacked the same bits): 6.4e-9, 6.3e-9, and 1.3e-8 at 31 - 33 chunks per wave
  fixed tiles of a batch, 1 / 2 / 4 / 8 / 16 chunks per wave: worst factor 8.1e-9 / 1.5e-8 / 1.9e-8 / 2.4e-8 / 3.1e-8 (the 5000-point factor, b_target), error <= 1.5e-8
  the whole file: 62 tests (52 planned cases = 39 different plans) in 13 s, the slowest 1.3 s
"""
import ctypes as C

import numpy as np
import pytest

import factor_domain_ref as fdr
import stream_plan_ref as spr
from helpers import BLOCKS, assert_linearized_close, expmap, rel_err

pytestmark = pytest.mark.gpu
MIXED_TOL = 1e-6  # tests/test_vgicp_gpu.py's: f64 geometry and covariance inverse, f32 outer products and per-lane sums
KERNEL, SOURCE_POLICY, BALANCE, XCD_WEIGHT_0, FUSED, TILE_CHUNKS, MAX_WORKGROUPS, MIRROR = 0, 1, 5, 8, 17, 18, 19, 21
N_TARGET, SEED, LEAF = 64_000, 7, 0.5
PERTURBATION = [2e-4, -1e-4, 1.5e-4, 0.02, -0.01, 0.015]
EVAL_STEP = [0.002, -0.001, 0.003, 0.01, 0.02, -0.01]

_WORK = {}  # n (or (n, "sv")) -> inputs and f64 reference, computed once and left alone
_SEEN = {}  # n -> {geometry: record}, for the plan-against-plan figure


def _work(n):
    if n not in _WORK:
        from gtsam_points_amd import synthetic

        d = synthetic.make_c2_workload(n, N_TARGET, seed=SEED)
        d["leaf"] = LEAF
        delta = d["T_true"] @ expmap(PERTURBATION)
        de = delta @ expmap(EVAL_STEP)
        ref, err = fdr.vgicp_reference(d, delta, de)
        assert len(d["source_points"]) == n and ref["num_inliers"] > n // 2, (n, ref["num_inliers"])
        _WORK[n] = dict(d=d, delta=delta, de=de, ref=ref, err=err)
    return _WORK[n]


def _surface_keep(points, normals, delta):
    """lookup_voxels.cuh:41-50 in f64: a point is rejected when normalized(T p) . (R n) > 0.174 = cos(80 deg)"""
    p, n = points.astype(np.float64), normals.astype(np.float64)
    q = p @ delta[:3, :3].T + delta[:3, 3]
    return ~(((q / np.linalg.norm(q, axis=1, keepdims=True)) * (n @ delta[:3, :3].T)).sum(1) > 0.174)


def _work_sv(n):
    """the same cloud with every third normal turned away from the sensor, and the reference on the points the validation keeps"""
    if (n, "sv") not in _WORK:
        w = _work(n)
        normals = w["d"]["source_normals"].copy()
        normals[::3] *= -1.0
        keep = _surface_keep(w["d"]["source_points"], normals, w["delta"])
        assert 0.02 < 1.0 - keep.mean() < 0.98
        d = dict(w["d"], source_points=w["d"]["source_points"][keep], source_covs=w["d"]["source_covs"][keep])
        ref, err = fdr.vgicp_reference(d, w["delta"], w["de"])
        _WORK[(n, "sv")] = dict(normals=normals, ref=ref, err=err)
    return _WORK[(n, "sv")]


@pytest.fixture(scope="module")
def dev(gpu):
    """device side, shared by the file: ONE voxel map, one source cloud per n"""
    state = dict(clouds={})

    def get(n, normals=None):
        w = _work(n)
        if "vm" not in state:
            state["target"] = w["d"]["target_points"]
            vm = gpu.GaussianVoxelMapGPU(LEAF, target_points_drop_rate=0.0)
            vm.insert(gpu.PointCloudGPU(w["d"]["target_points"], w["d"]["target_covs"]))
            state["vm"] = vm
        assert np.array_equal(state["target"], w["d"]["target_points"])  # (same seed, same target size: the map is every n's)
        key = (n, normals is not None)
        if key not in state["clouds"]:
            state["clouds"][key] = gpu.PointCloudGPU(w["d"]["source_points"], w["d"]["source_covs"], normals=normals)
        return state["vm"], state["clouds"][key]

    yield get
    state.clear()


def _factor(gpu, vm, src, cap=1024, balance=-1, weights=None, **tuning):
    f = gpu.IntegratedVGICPFactorGPU(0, 1, vm, src).set_tuning(KERNEL, 12).set_tuning(MAX_WORKGROUPS, cap).set_tuning(BALANCE, balance)
    for x, v in enumerate(weights or ()):
        f.set_tuning(XCD_WEIGHT_0 + x, v)
    for key, value in tuning.items():
        f.set_tuning(int(key[1:]), value)
    return f


def _lin(gpu, f, delta):
    rec = gpu._capi.Linearized6()
    gpu._capi.check(f._lib.gp_vgicp_factor_linearize(f._h, gpu.types._pose16(delta), C.byref(rec)), "linearize")
    return gpu.LinearizedSystem6(rec)


def _err(gpu, f, delta, de):
    e = C.c_double()
    gpu._capi.check(f._lib.gp_vgicp_factor_compute_error(f._h, gpu.types._pose16(delta), gpu.types._pose16(de), C.byref(e)), "compute_error")
    return e.value


def _same_bits(a, b, what):
    for k in BLOCKS:
        assert np.array_equal(getattr(a, k), getattr(b, k)), (what, k)
    assert a.error == b.error and a.num_inliers == b.num_inliers, what


def _check(gpu, f, w, ref, err_ref, what):
    """twice the same bits; linearise and error evaluation against the reference at the contract; the worst block printed first"""
    L, e = _lin(gpu, f, w["delta"]), _err(gpu, f, w["delta"], w["de"])
    worst, block, errs = fdr.worst_block(L, ref)
    e_rel = abs(e - err_ref) / abs(err_ref)
    print(f"[stream] {what}: worst block {block} {worst:.3e} (H_source {errs['H_source']:.3e}, b_source {errs['b_source']:.3e}, b_target {errs['b_target']:.3e}), "
          f"error at the evaluation pose {e_rel:.3e}, inliers {L.num_inliers} / {ref['num_inliers']}")
    _same_bits(L, _lin(gpu, f, w["delta"]), what + ", second call")
    assert e == _err(gpu, f, w["delta"], w["de"]), what
    assert_linearized_close(L, ref, MIXED_TOL, what)
    assert e_rel <= MIXED_TOL, (what, e, err_ref)
    return L, e


def _lengths(n, cap, balance, weights):
    wv = spr.launch_waves(n, cap, balance, weights)[1][:, 1]
    return f"{wv.min()}-{wv.max()} chunks per wave"


def _id(case):
    n, cap, balance, weights = case
    return f"{n}-cap{cap}-bal{'auto' if balance < 0 else balance}-" + ("table" if weights is None else "w" + "_".join(str(v) for v in weights))


def test_control_below_the_threshold_runs_on_fixed_tiles(gpu, dev):
    n = spr.N_CONTROL
    w = _work(n)
    vm, src = dev(n)
    _check(gpu, _factor(gpu, vm, src), w, w["ref"], w["err"], f"n={n} (fixed tiles)")


@pytest.mark.parametrize("case", spr.CASES, ids=_id)
def test_planned_geometry(gpu, dev, case):
    n, cap, balance, weights = case
    w = _work(n)
    vm, src = dev(n)
    what = f"n={n} cap={cap} balance={balance} weights={'table' if weights is None else list(weights)}: {_lengths(*case)}"
    L, _ = _check(gpu, _factor(gpu, vm, src, cap, balance, weights), w, w["ref"], w["err"], what)
    _SEEN.setdefault(n, {})[case] = L


def test_plan_against_plan(gpu, dev):
    """printed, not asserted against a figure of its own (the assertion is the reference, at the contract): how far two geometries of one cloud are apart"""
    n = spr.N_SKEW
    w = _work(n)
    vm, src = dev(n)
    recs = _SEEN.setdefault(n, {})
    for case in spr.CASES:  # (what test_planned_geometry has not left here, when this test runs alone)
        if case[0] == n and case not in recs:
            recs[case] = _lin(gpu, _factor(gpu, vm, src, *case[1:]), w["delta"])
    worst = (0.0, None)
    cases = list(recs)
    for i, a in enumerate(cases):
        for b in cases[i + 1:]:
            for k in BLOCKS:
                worst = max(worst, (rel_err(getattr(recs[a], k), getattr(recs[b], k)), (k, _id(a), _id(b))), key=lambda t: t[0])
            assert recs[a].num_inliers == recs[b].num_inliers
    plans = len({spr.launch_waves(*c)[1].tobytes() for c in cases})
    print(f"[stream] plan against plan, n={n}, {len(cases)} cases = {plans} different plans: largest difference {worst[0]:.3e} ({worst[1]})")


INSTANTIATIONS = [(65_599, 1024), (spr.N_MID[1], 256), (65_599, 8)]  # shortest waves (0 - 2 chunks), 2 - 3 chunks per wave, 32 per wave (tail 63 both)


@pytest.mark.parametrize("n,cap", INSTANTIATIONS, ids=lambda v: str(v))
def test_instantiations_agree_bit_for_bit(gpu, dev, n, cap):
    """the kernel's template axes on three geometries: packed mirror / caller's arrays (PK), default / non-temporal source stream (NT), fused / two-kernel finalize
    (parts at >= 256 workgroups, by factor below), an unaligned view of the same points -- identical bits; surface validation (SV) against the reference"""
    import torch

    w = _work(n)
    vm, src = dev(n)
    what = f"n={n} cap={cap}: {_lengths(n, cap, -1, None)}"
    f = _factor(gpu, vm, src, cap)
    L, e = _lin(gpu, f, w["delta"]), _err(gpu, f, w["delta"], w["de"])
    assert_linearized_close(L, w["ref"], MIXED_TOL, what)
    for name, tuning in [("mirror off", dict(k21=0)), ("policy 1", dict(k1=1)), ("policy 2", dict(k1=2)), ("two-kernel finalize", dict(k17=0)),
                         ("mirror off, policy 2, two-kernel", dict(k21=0, k1=2, k17=0))]:
        g = _factor(gpu, vm, src, cap, **tuning)
        _same_bits(L, _lin(gpu, g, w["delta"]), f"{what}, {name}")
        assert _err(gpu, g, w["delta"], w["de"]) == e, (what, name)
    # a view that starts 12 / 36 bytes into its allocation
    d = w["d"]
    whole = gpu.PointCloudGPU(np.concatenate([d["source_points"][:1], d["source_points"]]), np.concatenate([d["source_covs"][:1], d["source_covs"]]))
    view = gpu.PointCloudGPU.from_device(whole.points_gpu[1:], whole.covs_gpu[1:])
    assert view.points_gpu.data_ptr() % 16 == 12 and view.size() == n
    g = _factor(gpu, vm, view, cap)
    _same_bits(L, _lin(gpu, g, w["delta"]), what + ", unaligned view")
    assert _err(gpu, g, w["delta"], w["de"]) == e
    del g, view, whole
    torch.cuda.synchronize()
    # surface validation rides in the ring (a fourth / fifth request per chunk): against the f64 reference on the points the same rule keeps
    sv = _work_sv(n)
    _, src_n = dev(n, sv["normals"])
    for name, tuning in [("", {}), (", mirror off", dict(k21=0))]:
        g = _factor(gpu, vm, src_n, cap, **tuning)
        g.set_enable_surface_validation(True)
        Ls, _ = _check(gpu, g, w, sv["ref"], sv["err"], f"{what}, surface validation{name}")
        assert Ls.num_inliers < L.num_inliers


@pytest.mark.parametrize("tile_chunks", spr.TILE_CHUNKS)
def test_fixed_tiles_of_a_batch(gpu, dev, tile_chunks):
    """three small factors in one batch, GP_TUNE_TILE_CHUNKS chunks per wave of a tile (256 x value points): every factor's record and error against the reference"""
    lib = gpu.load()
    w = _work(spr.N_CONTROL)
    vm, _ = dev(spr.N_CONTROL)
    d = w["d"]
    key = ("batch", spr.FIXED_BATCH)
    if key not in _WORK:
        parts, at = [], 0
        for n in spr.FIXED_BATCH:
            sub = dict(d, source_points=d["source_points"][at:at + n], source_covs=d["source_covs"][at:at + n])
            ref, err = fdr.vgicp_reference(sub, w["delta"], w["de"])
            assert ref["num_inliers"] > n // 2
            parts.append(dict(points=sub["source_points"], covs=sub["source_covs"], ref=ref, err=err))
            at += n
        _WORK[key] = parts
    parts = _WORK[key]
    clouds = [gpu.PointCloudGPU(p["points"], p["covs"]) for p in parts]
    factors = [gpu.IntegratedVGICPFactorGPU(0, 1, vm, c) for c in clouds]
    arr = (C.c_void_p * len(factors))(*[f._h.value for f in factors])
    batch = C.c_void_p()
    gpu._capi.check(lib.gp_vgicp_batch_create(arr, len(factors), None, C.byref(batch)), "batch")
    try:
        gpu._capi.check(lib.gp_vgicp_batch_set_tuning(batch, KERNEL, 12), "kernel")
        gpu._capi.check(lib.gp_vgicp_batch_set_tuning(batch, TILE_CHUNKS, tile_chunks), "tile chunks")
        pose = np.tile(np.ascontiguousarray(w["delta"].T).reshape(1, 16), (len(factors), 1)).copy()
        pose_e = np.tile(np.ascontiguousarray(w["de"].T).reshape(1, 16), (len(factors), 1)).copy()
        out, out2, e, e2 = np.zeros((len(factors), 122)), np.zeros((len(factors), 122)), np.zeros(len(factors)), np.zeros(len(factors))
        gpu._capi.check(lib.gp_vgicp_batch_linearize(batch, pose.ctypes.data, out.ctypes.data), "linearize")
        gpu._capi.check(lib.gp_vgicp_batch_linearize(batch, pose.ctypes.data, out2.ctypes.data), "linearize")
        gpu._capi.check(lib.gp_vgicp_batch_compute_error(batch, pose.ctypes.data, pose_e.ctypes.data, e.ctypes.data), "compute_error")
        gpu._capi.check(lib.gp_vgicp_batch_compute_error(batch, pose.ctypes.data, pose_e.ctypes.data, e2.ctypes.data), "compute_error")
        v = C.c_int()
        gpu._capi.check(lib.gp_vgicp_batch_get_tuning(batch, 6, C.byref(v)), "effective kernel")
        assert v.value == 12
    finally:
        lib.gp_vgicp_batch_destroy(batch)
    assert np.array_equal(out, out2) and np.array_equal(e, e2)
    for i, (n, p) in enumerate(zip(spr.FIXED_BATCH, parts)):
        L = gpu.LinearizedSystem6.from_doubles(out[i])
        worst, block, errs = fdr.worst_block(L, p["ref"])
        e_rel = abs(e[i] - p["err"]) / abs(p["err"])
        print(f"[stream] fixed tiles, {tile_chunks} chunks per wave, factor of {n}: worst block {block} {worst:.3e} (b_source {errs['b_source']:.3e}), error {e_rel:.3e}")
        assert_linearized_close(L, p["ref"], MIXED_TOL, f"tile chunks {tile_chunks}, factor of {n}")
        assert e_rel <= MIXED_TOL

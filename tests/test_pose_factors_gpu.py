"""gtsam::BetweenFactor<Pose3> / PriorFactor<Pose3> on the device (csrc/gp_pose_factors.hip) and in the device-resident LM graph (gp_lm_graph_create_with_pose_factors):
records against the numpy statement of GTSAM's formulas (tests/pose3_ref.py), the Jacobians against central differences, the dense and sparse systems over them, a
pure pose graph and a mixed VGICP + pose graph optimised on the device against bench_lm.run_lm over host graphs, and the C3 graph through the new entry point."""
import ctypes as C

import numpy as np
import pytest

import bench_lm
import pose3_ref
from helpers import assert_linearized_close, kitti_graph, rigid

pytestmark = pytest.mark.gpu


class _Rec:
    """a [122] record as the named blocks assert_linearized_close reads"""

    def __init__(self, r):
        self.num_inliers, self.error = r[0], r[1]
        self.H_target, self.H_source, self.H_target_source = r[2:38].reshape(6, 6).T, r[38:74].reshape(6, 6).T, r[74:110].reshape(6, 6).T
        self.b_target, self.b_source = r[110:116], r[116:122]


def _random_information(rng, form):
    if form == "full":
        A = rng.normal(size=(6, 6))
        L = A @ A.T + 0.5 * np.eye(6)
        return 0.5 * (L + L.T)
    if form == "diagonal":
        return np.diag(rng.uniform(0.5, 50.0, 6))
    return 1e6 * np.eye(6)


def _rot(axis, th):
    axis = np.asarray(axis, dtype=np.float64)
    return pose3_ref.expmap(np.concatenate([th * axis / np.linalg.norm(axis), np.zeros(3)]))


def _pi_pose(axis, t):
    """a rotation of EXACTLY pi about `axis` (R = 2 n n^T - I: no sin / cos rounding)"""
    n = np.asarray(axis, dtype=np.float64)
    n = n / np.linalg.norm(n)
    T = np.eye(4)
    T[:3, :3] = 2.0 * np.outer(n, n) - np.eye(3)
    T[:3, 3] = t
    return rigid(T[None])[0] if np.count_nonzero(n) > 1 else T


def _check(gpu, factors, values, tol):
    pf = gpu.PoseFactorsGPU(factors, len(values))
    got = pf.linearize(values)
    err = pf.error(values)
    dev = pf.linearize_on_device(values).cpu().numpy()
    assert np.array_equal(dev, got)  # the device-tensor form = the synchronous one, bit for bit
    assert np.array_equal(err, got[:, 1])  # the error pass = the records' word 1, bit for bit
    for k, f in enumerate(factors):
        ref = pose3_ref.factor_record(f, values)
        assert_linearized_close(_Rec(got[k]), _Rec(ref).__dict__ | {"num_inliers": 0.0}, tol, f"factor {k}")
    pf.close()
    return got


@pytest.mark.parametrize("form", ["full", "diagonal", "isotropic"])
def test_records_match_the_numpy_statement(gpu, form):
    rng = np.random.default_rng({"full": 1, "diagonal": 2, "isotropic": 3}[form])
    N = 12
    values = bench_lm.expmap_many(rng.normal(scale=[1.0] * 3 + [5.0] * 3, size=(N, 6)))
    factors = []
    for k in range(N - 1):
        Z = pose3_ref.inverse(values[k]) @ values[k + 1] @ pose3_ref.expmap(rng.normal(scale=0.2, size=6))
        factors.append(gpu.BetweenFactorPose3(k, k + 1, Z, information=_random_information(rng, form)))
    for k in range(0, N, 3):
        factors.append(gpu.BetweenFactorPose3(k, (k + 5) % N, bench_lm.expmap_many(rng.normal(size=(1, 6)))[0], information=_random_information(rng, form)))
        factors.append(gpu.PriorFactorPose3(k, values[k] @ pose3_ref.expmap(rng.normal(scale=0.5, size=6)), information=_random_information(rng, form)))
    _check(gpu, factors, values, 1e-12)


@pytest.mark.parametrize("th", [0.0, 1e-12, 1e-7, 0.4, np.pi - 1e-7])
def test_records_at_small_and_large_angles(gpu, th):
    """theta = 0, 1e-12, 1e-7 take the series branches of SO3::Logmap and Pose3::Logmap's small-angle return; pi - 1e-7 the near-pi branch"""
    rng = np.random.default_rng(11)
    Lam = _random_information(rng, "full")
    values = np.stack([np.eye(4), np.eye(4), np.eye(4)])
    values[0] = pose3_ref.expmap(rng.normal(size=6))
    factors = []
    for axis in ([1, 0, 0], [0, 1, 0], [0, 0, 1], [0.3, -0.5, 0.8]):
        D = _rot(axis, th)
        D[:3, 3] = [0.4, -1.2, 2.0]
        values[1] = values[0] @ D
        Z = pose3_ref.expmap(1e-3 * rng.normal(size=6)) if th > 0.1 else np.eye(4)
        v = values.copy()
        factors = [gpu.BetweenFactorPose3(0, 1, np.eye(4), information=Lam), gpu.PriorFactorPose3(2, pose3_ref.inverse(D), information=Lam),
                   gpu.BetweenFactorPose3(1, 0, Z, information=np.eye(6))]
        tol = 1e-9 if th > 3 else 1e-12
        got = _check(gpu, factors, v, tol)
        if th > 3:  # the two near-pi formula variants are both accurate there, not bit-equal: Expmap(Logmap(T)) = T
            pf = gpu.PoseFactorsGPU([gpu.BetweenFactorPose3(0, 1, np.eye(4))], 3)
            e = pf.linearize(v)[0, 116:122]  # b_source = Lambda e = e
            assert np.allclose(pose3_ref.expmap(e), D, atol=1e-9)
            pf.close()


@pytest.mark.parametrize("axis", [[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 2, -2]])
def test_records_at_exactly_pi(gpu, axis):
    """the relative pose is D itself, bit for bit, on both sides (T_a = Z = I): at exactly pi the sign of omega follows the rounding of R32 - R23, so the operands must
    not differ by a rounding"""
    rng = np.random.default_rng(5)
    D = _pi_pose(axis, [0.3, 0.7, -1.1])
    values = np.stack([np.eye(4), D])
    Lam = _random_information(rng, "full")
    factors = [gpu.BetweenFactorPose3(0, 1, np.eye(4), information=Lam), gpu.PriorFactorPose3(1, np.eye(4), information=Lam),
               gpu.PriorFactorPose3(0, D, information=np.eye(6))]
    _check(gpu, factors, values, 1e-9)
    pf = gpu.PoseFactorsGPU([gpu.PriorFactorPose3(0, np.eye(4))], 1)  # e = Logmap(D) itself
    e = pf.linearize(np.stack([D]))[0, 116:122]
    assert abs(np.linalg.norm(e[:3]) - np.pi) < 1e-9
    assert np.allclose(pose3_ref.expmap(e), D, atol=1e-9)
    pf.close()


def _numeric_jacobians(Ta, Tb, Z, h=1e-6):
    """central differences of the numpy error along the retracts of a and b"""
    J = np.zeros((6, 12))
    for k in range(12):
        d = np.zeros(6)
        d[k % 6] = h
        if k < 6:
            ep, em = pose3_ref.between_error(Ta @ pose3_ref.expmap(d), Tb, Z), pose3_ref.between_error(Ta @ pose3_ref.expmap(-d), Tb, Z)
        else:
            ep, em = pose3_ref.between_error(Ta, Tb @ pose3_ref.expmap(d), Z), pose3_ref.between_error(Ta, Tb @ pose3_ref.expmap(-d), Z)
        J[:, k] = (ep - em) / (2 * h)
    return J


def test_jacobians_against_central_differences(gpu):
    """at e = 0 (Z = hx) the records are J^T Lambda J of the true derivative; away from it they differ from it by the omitted LogmapDerivative(e) -- GTSAM's default"""
    rng = np.random.default_rng(21)
    Lam = _random_information(rng, "full")
    Ta, Tb = pose3_ref.expmap(rng.normal(size=6)), pose3_ref.expmap(rng.normal(size=6))
    hx = pose3_ref.inverse(Ta) @ Tb
    values = rigid(np.stack([Ta, Tb]))
    for Z, exact in ((hx, True), (hx @ pose3_ref.expmap([0.3, -0.2, 0.25, 0.5, 0.1, -0.4]), False)):
        Z = rigid(Z[None])[0]
        pf = gpu.PoseFactorsGPU([gpu.BetweenFactorPose3(0, 1, Z, information=Lam)], 2)
        r = _Rec(pf.linearize(values)[0])
        pf.close()
        J = _numeric_jacobians(values[0], values[1], Z)
        H = J.T @ Lam @ J
        dev = np.block([[r.H_target, r.H_target_source], [r.H_target_source.T, r.H_source]])
        rel = np.linalg.norm(dev - H) / np.linalg.norm(H)
        if exact:
            assert rel < 1e-7, rel
        else:
            assert rel > 1e-2, rel  # the true derivative carries LogmapDerivative(e); GTSAM's BetweenFactor does not


@pytest.mark.parametrize("kind", ["dense", "sparse"])
def test_standalone_records_feed_the_systems(gpu, kind):
    rng = np.random.default_rng(31)
    N = 10
    values = bench_lm.expmap_many(rng.normal(size=(N, 6)))
    factors = [gpu.BetweenFactorPose3(k, k + 1, pose3_ref.inverse(values[k]) @ values[k + 1] @ pose3_ref.expmap(0.1 * rng.normal(size=6)),
                                      information=_random_information(rng, "full")) for k in range(N - 1)]
    factors += [gpu.BetweenFactorPose3(0, 7, pose3_ref.expmap(rng.normal(size=6))), gpu.PriorFactorPose3(3, values[3] @ pose3_ref.expmap(0.01 * rng.normal(size=6)), information=1e6 * np.eye(6)),
                gpu.PriorFactorPose3(0, values[0] @ pose3_ref.expmap(0.1 * rng.normal(size=6)), sigmas=[0.1] * 3 + [0.3] * 3)]
    slot = np.full(N, -1)
    free = [k for k in range(N) if k != 5]  # pose 5 held: its factors drop that side
    slot[free] = np.arange(len(free))
    pf = gpu.PoseFactorsGPU(factors, N)
    fs = pf.factor_slots(slot)
    rec = pf.linearize_on_device(values)
    sys = gpu.DenseLinearSystemGPU(len(free), fs) if kind == "dense" else gpu.SparseLinearSystemGPU(len(free), fs)
    A, b, c = sys.build(rec).download()
    ref = np.stack([pose3_ref.factor_record(f, values) for f in factors])
    A0, b0, c0 = bench_lm.host_system(ref, fs, len(free))
    assert np.linalg.norm(A - A0) <= 1e-12 * np.linalg.norm(A0)
    assert np.linalg.norm(b - b0) <= 1e-12 * np.linalg.norm(b0)
    assert abs(c - c0) <= 1e-12 * c0
    pf.close()


def _pose_graph(gpu, N=300, seed=41):
    """a chain of N poses with loop closures every 25 poses, noisy measurements, one soft prior on pose 0; the start = the chain's odometry composed with noise"""
    rng = np.random.default_rng(seed)
    truth = [np.eye(4)]
    for k in range(1, N):
        truth.append(truth[-1] @ pose3_ref.expmap([0.0, 0.0, 0.05, 1.0, 0.0, 0.0]))
    truth = np.stack(truth)
    sig = np.array([0.01] * 3 + [0.05] * 3)
    factors = [gpu.PriorFactorPose3(0, truth[0], information=1e6 * np.eye(6))]
    edges = [(k, k + 1) for k in range(N - 1)] + [(k, k + 20) for k in range(0, N - 20, 25)]
    for a, b in edges:
        Z = pose3_ref.inverse(truth[a]) @ truth[b] @ pose3_ref.expmap(sig * rng.normal(size=6))
        factors.append(gpu.BetweenFactorPose3(a, b, Z, sigmas=sig))
    v0 = rigid(truth @ bench_lm.expmap_many(rng.normal(scale=[0.02] * 3 + [0.2] * 3, size=(N, 6))))
    return factors, truth, v0


def test_pure_pose_graph_follows_the_host_loop(gpu):
    N = 300
    factors, truth, v0 = _pose_graph(gpu, N)
    host = pose3_ref.HostPoseGraph(factors, N)
    ref = bench_lm.run_lm(host, v0, max_iterations=30)
    g = gpu.LevenbergMarquardtGraphGPU([], [], N, fixed=(), pose_factors=factors)
    assert g.n == 6 * N
    runs = {}
    for one_launch in (True, False):
        for spec in (True, False):
            g.set_one_launch(one_launch)
            g.set_speculation(spec)
            runs[(one_launch, spec)] = g.optimize(v0, max_iterations=30)
    again = g.optimize(v0, max_iterations=30)
    vals, s = runs[(True, True)]
    assert s["iterations"] == ref["iterations"] and s["inner_iterations"] == ref["inner_iterations"], (s, ref["iterations"], ref["inner_iterations"])
    assert np.abs(vals - ref["values"]).max() < 1e-9
    assert abs(s["final_error"] - ref["final_error"]) <= 1e-9 * ref["final_error"]
    for key, (v, ss) in list(runs.items()) + [("again", again)]:
        assert np.array_equal(v, vals) and ss == s, key  # bit-identical across one-launch / speculation and runs
    # the trial piece by piece: the device's c and new_error against the host graph's
    g.set_values(v0)
    g.linearize()
    dx, b, c, e, vt = g.try_lambda(1e-3, want_values=True)
    c0 = host.linearize(v0)
    dx0, b0, _ = host.solve(1e-3)
    assert abs(c - c0) <= 1e-9 * c0  # (relative poses of 300 m apart values: their rounding differs between the two statements at ~1e-13 m)
    np.testing.assert_allclose(dx, dx0, rtol=1e-7, atol=1e-10)
    assert abs(e - host.error(vt)) <= 1e-9 * e
    assert abs(float(g.records()[:, 1].sum()) - c) <= 1e-12 * c  # c = the sum of the records' errors
    g.close()


class _TrialGraph(bench_lm.GpuTrialGraph):
    """bench_lm's device-trial back end over a graph with pose factors, nothing held"""

    def __init__(self, gpa, factors, pairs, num_poses, pose_factors):
        bench_lm._Graph.__init__(self, pairs, num_poses, fixed=-1)
        self.g = gpa.LevenbergMarquardtGraphGPU(factors, self.pairs, num_poses, fixed=(), pose_factors=pose_factors)
        self.sync_phases = False
        self._trial = None
        self._trial_error = None


def test_mixed_graph_on_kitti07(gpu, kitti07):
    factors, pairs, truth, v0, keep = kitti_graph(gpu, kitti07)
    truth, v0 = rigid(truth), rigid(v0)
    n = len(truth)
    rng = np.random.default_rng(77)
    sig = np.array([0.005] * 3 + [0.05] * 3)
    pose_factors = [gpu.PriorFactorPose3(0, truth[0], information=1e6 * np.eye(6))]
    for k in range(n - 1):
        Z = rigid((pose3_ref.inverse(truth[k]) @ truth[k + 1] @ pose3_ref.expmap(0.2 * sig * rng.normal(size=6)))[None])[0]
        pose_factors.append(gpu.BetweenFactorPose3(k, k + 1, Z, sigmas=sig))
    host = pose3_ref.HostPoseGraph(pose_factors, n, vgicp=bench_lm.GpuGraph(gpu, factors, pairs, n, fixed=0, solver="host"))
    ref = bench_lm.run_lm(host, v0, max_iterations=30)
    tg = _TrialGraph(gpu, factors, pairs, n, pose_factors)
    res = bench_lm.run_lm(tg, v0, max_iterations=30)
    assert res["iterations"] == ref["iterations"] and res["inner_iterations"] == ref["inner_iterations"]  # the same accept / reject decisions
    np.testing.assert_allclose(res["errors"], ref["errors"], rtol=1e-9)
    np.testing.assert_allclose(res["values"], ref["values"], atol=1e-9)
    base_v, base_t = pose3_ref.inverse(res["values"][0]), pose3_ref.inverse(truth[0])
    for k in range(n):
        ang, tr = bench_lm.pose_error(base_v @ res["values"][k], base_t @ truth[k])
        assert ang < 0.015 and tr < 0.15, (k, ang, tr)  # the reference's gate
    tg.g.set_values(v0)
    tg.g.linearize()
    _, _, c, _ = tg.g.try_lambda(1e-3)
    recs = tg.g.records()
    assert recs.shape == (len(factors) + len(pose_factors), 122)
    assert abs(float(recs[:, 1].sum()) - c) <= 1e-12 * c
    nat_v, nat = tg.g.optimize(v0, max_iterations=30)
    assert nat["iterations"] == res["iterations"] and nat["inner_iterations"] == res["inner_iterations"]
    assert np.array_equal(nat_v, res["values"])  # the library's loop = the interpreter driving its three calls
    tg.close()
    host.close()


def _c3(gpu):
    from gtsam_points_amd import synthetic

    g = synthetic.make_c3_graph()
    clouds = [gpu.PointCloudGPU(p, c) for p, c in g["clouds"]]
    maps = []
    for c in clouds:
        m = gpu.GaussianVoxelMapGPU(1.0, target_points_drop_rate=0.0)
        m.insert(c)
        maps.append(m)
    factors = [gpu.IntegratedVGICPFactorGPU(t, s, maps[t], clouds[s]) for t, s in g["pairs"]]
    n = len(g["clouds"])
    truth = rigid(np.stack(g["stations"][:n]))
    v0 = rigid(truth @ bench_lm.expmap_many(np.random.default_rng(8191).uniform(-0.1, 0.1, (n, 6))))
    v0[0] = truth[0]
    return factors, g["pairs"], truth, v0, (clouds, maps)


def _trial_sequence(gpu, lib, h, n, N, v0):
    """set_values, linearize, records, two trials (the first dropped), accept, linearize, a trial: every output as bytes"""
    x, b, c, e, v = np.zeros(n), np.zeros(n), np.zeros(1), np.zeros(1), np.zeros((N, 16))
    out = []
    vals = np.ascontiguousarray(v0.transpose(0, 2, 1)).reshape(N, 16)
    assert lib.gp_lm_graph_set_values(h, vals.ctypes.data) == 0
    for step in ("lin", 1e-5, 1e-1, "accept", "lin", 1e-3):
        if step == "lin":
            assert lib.gp_lm_graph_linearize(h) == 0
        elif step == "accept":
            assert lib.gp_lm_graph_accept(h) == 0
        else:
            assert lib.gp_lm_graph_try_lambda(h, step, 0, 1e-6, 1e32, x.ctypes.data, b.ctypes.data, c.ctypes.data, e.ctypes.data, v.ctypes.data) == 0
            out += [x.tobytes(), b.tobytes(), c.tobytes(), e.tobytes(), v.tobytes()]
    p = C.c_void_p()
    assert lib.gp_lm_graph_records(h, C.byref(p), None) == 0
    import torch

    torch.cuda.synchronize()
    F = 256
    rec = torch.zeros(F * 122, dtype=torch.float64, device="cuda")
    assert lib.gp_stream_synchronize(None) == 0 and lib.gp_memcpy_d2d(C.c_void_p(rec.data_ptr()), p, 8 * F * 122, None) == 0 and lib.gp_stream_synchronize(None) == 0
    return out + [rec.cpu().numpy().tobytes()]


def test_c3_through_the_new_entry_point(gpu):
    """P = 0 through gp_lm_graph_create_with_pose_factors = gp_lm_graph_create, bit for bit; C3 + 63 odometry factors + a prior keeps the one-launch sparse step"""
    from gtsam_points_amd import _capi

    factors, pairs, truth, v0, keep = _c3(gpu)
    lib = gpu.load()
    F, N = len(factors), len(truth)
    pp = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32))
    held = np.zeros(N, np.uint8)
    held[0] = 1
    batch = C.c_void_p()
    _capi.check(lib.gp_vgicp_batch_create((C.c_void_p * F)(*[f._h.value for f in factors]), F, None, C.byref(batch)), "batch")
    seqs = []
    for new in (False, True):
        h = C.c_void_p()
        if new:
            _capi.check(lib.gp_lm_graph_create_with_pose_factors(batch, pp.ctypes.data, None, 0, N, held.ctypes.data, 4, None, C.byref(h)), "create_with_pose_factors")
        else:
            _capi.check(lib.gp_lm_graph_create(batch, pp.ctypes.data, N, held.ctypes.data, 4, C.byref(h)), "create")
        seqs.append(_trial_sequence(gpu, lib, h, lib.gp_lm_graph_num_variables(h), N, v0))
        lib.gp_lm_graph_destroy(h)
    assert seqs[0] == seqs[1]
    lib.gp_vgicp_batch_destroy(batch)
    # C3 plus odometry along the chain and a prior on pose 0, nothing held
    rng = np.random.default_rng(99)
    sig = np.array([0.01] * 3 + [0.1] * 3)
    pose_factors = [gpu.PriorFactorPose3(0, truth[0], information=1e6 * np.eye(6))]
    for k in range(N - 1):
        Z = rigid((pose3_ref.inverse(truth[k]) @ truth[k + 1] @ pose3_ref.expmap(0.2 * sig * rng.normal(size=6)))[None])[0]
        pose_factors.append(gpu.BetweenFactorPose3(k, k + 1, Z, sigmas=sig))
    assert len(pose_factors) == 64
    g = gpu.LevenbergMarquardtGraphGPU(factors, pairs, N, fixed=(), pose_factors=pose_factors)
    assert g.set_one_launch(True) == 1  # the chain edges are already blocks of A: the system still fits one compute unit
    vals, s = g.optimize(v0, max_iterations=30)
    g.set_one_launch(False)
    vals2, s2 = g.optimize(v0, max_iterations=30)
    assert np.array_equal(vals, vals2) and s == s2 and s["iterations"] > 1
    g.close()

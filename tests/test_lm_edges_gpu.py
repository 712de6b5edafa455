"""The device LM's error-evaluation recovery path and its pose algebra.

C. When the completion words of a fused error evaluation are missing, gp_vgicp_batch_compute_error_dev_end recovers on the host.  The LM trial queues the speculative
   linearise into the batch's partials buffer between _begin and _end, so the recovery must not re-sum those rows.  gp_debug_drop_error_words sends evaluations down
   that path; the errors, and a whole optimize(), must be the bits of the ordinary path.
D. The relative poses the LM graph evaluates its factors at, and the trial values, against an independent f64/mpmath statement of gtsam::Pose3 (inverse = (R^T, -R^T t),
   compose, the closed-form Expmap in the (omega, v) order, retract = T Expmap(xi)) -- for orthonormal values and values 1e-7 / 1e-4 off orthonormality."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench_lm  # noqa: E402
from helpers import kitti_graph, rigid  # noqa: E402

pytestmark = pytest.mark.gpu

mpmath = pytest.importorskip("mpmath")
mp = mpmath.mp


# ---- C: the recovery path of the fused error evaluation -------------------------------------------------------------------------------------------------------------------
def test_error_recovery_with_a_linearise_queued_behind_the_evaluation(gpu, kitti07):
    """_begin, a linearise into a second record buffer on the batch stream (what try_lambda's speculation does), then _end with the words dropped: the same errors, bit for bit,
    as without the hook; the synchronous call's recovery too"""
    import torch
    from gtsam_points_amd import _capi

    factors, pairs, truth, v0, keep = kitti_graph(gpu, kitti07)
    truth, v0 = rigid(truth), rigid(v0)
    lib = gpu.load()
    F = len(factors)
    g = bench_lm._Graph(pairs, 5)
    p_lin, p_eval = bench_lm._poses16(g.deltas(v0)), bench_lm._poses16(g.deltas(truth))
    batch = C.c_void_p()
    _capi.check(lib.gp_vgicp_batch_create((C.c_void_p * F)(*[f._h.value for f in factors]), F, None, C.byref(batch)), "batch")
    try:
        d_lin, d_eval = torch.from_numpy(p_lin).cuda(), torch.from_numpy(p_eval).cuda()
        spec = torch.zeros((F, 122), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()

        def trial(drop, speculate=True):
            out = np.full(F, np.nan)
            _capi.check(lib.gp_debug_drop_error_words(batch, int(drop)), "drop")
            _capi.check(lib.gp_vgicp_batch_issue_compute_error_dev_begin(batch, C.c_void_p(d_lin.data_ptr()), C.c_void_p(d_eval.data_ptr())), "begin")
            if speculate:
                _capi.check(lib.gp_vgicp_batch_issue_linearize_dev(batch, C.c_void_p(d_eval.data_ptr()), 1, C.c_void_p(spec.data_ptr())), "linearize behind")
            _capi.check(lib.gp_vgicp_batch_compute_error_dev_end(batch, out.ctypes.data), "end")
            _capi.check(lib.gp_vgicp_batch_sync(batch), "sync")
            return out

        plain = trial(0)
        assert np.isfinite(plain).all() and plain.min() > 0
        for speculate in (True, False):
            assert np.array_equal(trial(1, speculate), plain), speculate
        assert np.array_equal(trial(0), plain)  # (the hook was used up)
        # the records the linearise behind the evaluation wrote are the ordinary ones
        rec = torch.zeros_like(spec)
        _capi.check(lib.gp_vgicp_batch_issue_linearize_dev(batch, C.c_void_p(d_eval.data_ptr()), 1, C.c_void_p(rec.data_ptr())), "linearize")
        _capi.check(lib.gp_vgicp_batch_sync(batch), "sync")
        trial(1)
        assert torch.equal(spec, rec)
        # the synchronous host-pose call: its recovery re-sums its own rows
        e0, e1 = np.zeros(F), np.zeros(F)
        _capi.check(lib.gp_vgicp_batch_compute_error(batch, p_lin.ctypes.data, p_eval.ctypes.data, e0.ctypes.data), "error")
        _capi.check(lib.gp_debug_drop_error_words(batch, 1), "drop")
        _capi.check(lib.gp_vgicp_batch_compute_error(batch, p_lin.ctypes.data, p_eval.ctypes.data, e1.ctypes.data), "error, words dropped")
        assert np.array_equal(e0, e1) and np.array_equal(e0, plain)
        assert lib.gp_debug_drop_error_words(None, 1) == 1 and lib.gp_debug_drop_error_words(batch, -1) == 1
    finally:
        lib.gp_debug_drop_error_words(batch, 0)
        lib.gp_vgicp_batch_destroy(batch)


def test_optimize_with_every_error_evaluation_recovered(gpu, kitti07):
    """gp_lm_graph_optimize with the words of every trial's evaluation dropped (speculation on): the same iterations, lambdas, costs and values, bit for bit"""
    factors, pairs, truth, v0, keep = kitti_graph(gpu, kitti07)
    truth, v0 = rigid(truth), rigid(v0)
    lib = gpu.load()
    lm = gpu.LevenbergMarquardtGraphGPU(factors, pairs, 5, fixed=(0,))
    try:
        assert lm.set_speculation(True) is True
        ref_values, ref = lm.optimize(v0, max_iterations=30)
        assert ref["iterations"] >= 2 and ref["inner_iterations"] > ref["iterations"] - 1
        gpu._capi.check(lib.gp_debug_drop_error_words(lm._batch, 1 << 30), "drop")
        values, s = lm.optimize(v0, max_iterations=30)
        assert s == ref, (s, ref)
        assert np.array_equal(values, ref_values)
        # one trial at a time, too: the cost at the trial values and the trial values themselves
        lm.set_values(v0)
        lm.linearize()
        got = [np.array(a, copy=True) for a in lm.try_lambda(1e-3, want_values=True)]
        gpu._capi.check(lib.gp_debug_drop_error_words(lm._batch, 0), "disarm")
        lm.set_values(v0)
        lm.linearize()
        want = [np.array(a, copy=True) for a in lm.try_lambda(1e-3, want_values=True)]
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
    finally:
        lib.gp_debug_drop_error_words(lm._batch, 0)
        lm.close()


# ---- D: the pose algebra of the LM graph -----------------------------------------------------------------------------------------------------------------------------------
def _mp(T):
    return mp.matrix([[mp.mpf(float(v)) for v in row] for row in np.asarray(T)])


def _np(M):
    return np.array([[float(M[i, j]) for j in range(M.cols)] for i in range(M.rows)])


def pose3_inverse(T):
    """gtsam::Pose3::inverse: (R^T, -R^T t) -- whatever R is"""
    R = T[0:3, 0:3]
    t = T[0:3, 3]
    Rt = R.T
    out = mp.eye(4)
    out[0:3, 0:3] = Rt
    out[0:3, 3] = -(Rt * t)
    return out


def pose3_expmap(xi):
    """gtsam::Pose3::Expmap, xi = (omega, v): R = I + sin(th)/th W + (1 - cos th)/th^2 W^2, t = (I + (1 - cos th)/th^2 W + (th - sin th)/th^3 W^2) v"""
    w = [mp.mpf(float(v)) for v in xi[:3]]
    v = mp.matrix([mp.mpf(float(u)) for u in xi[3:]])
    W = mp.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    th = mp.sqrt(w[0] ** 2 + w[1] ** 2 + w[2] ** 2)
    I3 = mp.eye(3)
    if th == 0:
        R, V = I3, I3
    else:
        A, B, Cc = mp.sin(th) / th, (1 - mp.cos(th)) / th**2, (th - mp.sin(th)) / th**3
        R = I3 + A * W + B * W * W
        V = I3 + B * W + Cc * W * W
    out = mp.eye(4)
    out[0:3, 0:3] = R
    out[0:3, 3] = V * v
    return out


def _off_orthonormal(values, eps, seed):
    rng = np.random.default_rng(seed)
    out = np.array(values, dtype=np.float64)
    if eps > 0:
        out[:, :3, :3] += eps * rng.uniform(-1.0, 1.0, (len(out), 3, 3))
    return out


def _download(lib, ptr, count):
    from gtsam_points_amd import _capi

    out = np.zeros(count)
    import torch

    _capi.check(lib.gp_memcpy_d2h(out.ctypes.data, ptr, 8 * count, None), "d2h")
    torch.cuda.synchronize()  # (the copy is asynchronous)
    return out


@pytest.mark.parametrize("eps", [0.0, 1e-7, 1e-4])
def test_relative_poses_and_retract_follow_pose3(gpu, kitti07, eps):
    """set_values -> the device's relative poses = inverse(T_t) T_s with inverse = (R^T, -R^T t), to 1e-13; try_lambda's trial values = T Expmap(x_slot), to 1e-13; and the
    records the graph linearises at those relative poses = gp_vgicp_batch_issue_linearize given the same poses from the host, bit for bit"""
    import torch
    from gtsam_points_amd import _capi

    mp.dps = 40
    factors, pairs, truth, v0, keep = kitti_graph(gpu, kitti07)
    values = _off_orthonormal(rigid(v0), eps, 7)
    lib = gpu.load()
    F, N = len(factors), 5
    lm = gpu.LevenbergMarquardtGraphGPU(factors, pairs, N, fixed=(0,))
    try:
        lm.set_values(values)
        lm.linearize()
        lm.sync()
        rec_p, rel_p = C.c_void_p(), C.c_void_p()
        _capi.check(lib.gp_lm_graph_records(lm._h, C.byref(rec_p), C.byref(rel_p)), "records")
        rel = _download(lib, rel_p, 16 * F).reshape(F, 4, 4).transpose(0, 2, 1)  # column-major 4x4 per factor
        records = _download(lib, rec_p, 122 * F).reshape(F, 122)
        scale = max(1.0, float(np.abs(values).max()))
        for f, (i, j) in enumerate(pairs):
            want = _np(pose3_inverse(_mp(values[i])) * _mp(values[j]))
            assert np.abs(rel[f] - want).max() <= 1e-13 * scale, (eps, f, np.abs(rel[f] - want).max())
        # the host-pose entry point at the same relative poses: the same kernels (rigid or general, as the poses are), the same records
        host = torch.zeros((F, 122), dtype=torch.float64, device="cuda:0")
        p16 = np.ascontiguousarray(rel.transpose(0, 2, 1)).reshape(F, 16)
        _capi.check(lib.gp_vgicp_batch_issue_linearize(lm._batch, p16.ctypes.data, C.c_void_p(host.data_ptr())), "host poses")
        _capi.check(lib.gp_vgicp_batch_sync(lm._batch), "sync")
        assert records[:, 0].min() > 100
        assert np.array_equal(host.cpu().numpy(), records), eps
        # the trial: T Expmap(x of the pose's slot) for the free poses, the held pose as it was
        dx, b, c, e, trial = lm.try_lambda(1e-3, want_values=True)
        dx = np.array(dx, copy=True)
        assert np.isfinite(dx).all() and np.abs(dx).max() > 1e-6
        assert np.array_equal(trial[0], values[0])
        for k in range(1, N):
            want = _np(_mp(values[k]) * pose3_expmap(dx[6 * (k - 1) : 6 * k]))
            assert np.abs(trial[k] - want).max() <= 1e-13 * scale, (eps, k, np.abs(trial[k] - want).max())
    finally:
        lm.close()

"""GICP and ICP factors in the device-resident LM graph (gp_lm_graph_create_with_factors, LevenbergMarquardtGraphGPU(corr_factors=...)): the trials against the loop
driven from the host over the single-factor calls (tests/corr_graph_ref.py), the correspondence sets under speculation, a graph that mixes VGICP, GICP / ICP and
pose factors, and the one-free-pose (dense) path."""
import numpy as np
import pytest

import bench_lm
import corr_graph_ref
import normals_ref
import pose3_ref
from helpers import kitti_graph, lm_optimize, rigid

pytestmark = pytest.mark.gpu
N = 5
PAIRS = [(i, j) for i in range(N) for j in range(i + 1, N)]
PLANE_EDGE, POINT_EDGE = (1, 2), (3, 4)


@pytest.fixture(scope="module")
def submaps(gpu, kitti07):
    """the five kitti07 submaps with their covariances (and normals read off them, for the point-to-plane targets), one search structure each, the truth and a
    perturbed start (pose 0 = truth)"""
    clouds, trees = [], []
    for i in range(N):
        p, c = kitti07[f"points_{i}"], kitti07[f"covs_{i}"]
        normals = np.ascontiguousarray(normals_ref.reference_normals(p, c).astype(np.float32))
        clouds.append(gpu.PointCloudGPU(p, c, normals=normals))
        trees.append(gpu.KdTreeGPU(clouds[-1]))
    truth = rigid(np.stack([np.asarray(T, dtype=np.float64) for T in kitti07["poses"][:N]]))
    v0 = truth @ bench_lm.expmap_many(np.random.default_rng(8191).uniform(-0.02, 0.02, (N, 6)))
    v0[0] = truth[0]
    return clouds, trees, truth, rigid(v0)


def _factor(gpu, submaps, i, j):
    clouds, trees = submaps[0], submaps[1]
    if (i, j) == PLANE_EDGE:
        return gpu.IntegratedICPFactorGPU(i, j, clouds[i], clouds[j], target_tree=trees[i], use_point_to_plane=True)
    if (i, j) == POINT_EDGE:
        return gpu.IntegratedICPFactorGPU(i, j, clouds[i], clouds[j], target_tree=trees[i])
    return gpu.IntegratedGICPFactorGPU(i, j, clouds[i], clouds[j])


@pytest.fixture(scope="module")
def chain(gpu, submaps):
    """point-to-plane on (1, 2), point-to-point on (3, 4), GICP on every other edge; the host graph over the same factor objects"""
    factors = [_factor(gpu, submaps, i, j) for i, j in PAIRS]
    host = corr_graph_ref.HostCorrGraph([corr_graph_ref.DeviceFactor(f) for f in factors], PAIRS, N, fixed=0)
    return factors, host


class _TrialGraph(bench_lm.GpuTrialGraph):
    """bench_lm's device-trial back end over a graph of correspondence factors, pose 0 held"""

    def __init__(self, gpa, corr_factors, corr_pairs, num_poses):
        bench_lm._Graph.__init__(self, corr_pairs, num_poses, fixed=0)
        self.g = gpa.LevenbergMarquardtGraphGPU([], [], num_poses, fixed=(0,), corr_factors=corr_factors, corr_pairs=corr_pairs)
        self.sync_phases = False
        self._trial = None
        self._trial_error = None


def test_trial_follows_the_host_driven_loop(gpu, submaps, chain):
    _, _, truth, v0 = submaps
    factors, host = chain
    ref = bench_lm.run_lm(host, v0, max_iterations=30)
    base_r, base_t = pose3_ref.inverse(ref["values"][0]), pose3_ref.inverse(truth[0])
    for k in range(N):  # the HOST loop decides that the start is fair: it reaches the reference's gate (test_matching_cost_factors.cpp:227-228) on its own
        ang, tr = bench_lm.pose_error(base_r @ ref["values"][k], base_t @ truth[k])
        print(f"[corr-lm] host loop, pose {k}: {ang:.3e} rad, {tr:.3e} m from the truth")
        assert ang < 0.015 and tr < 0.15, ("host loop", k, ang, tr)
    tg = _TrialGraph(gpu, factors, PAIRS, N)
    res = bench_lm.run_lm(tg, v0, max_iterations=30)
    print(f"[corr-lm] iterations {res['iterations']} / {ref['iterations']}, trials {res['inner_iterations']} / {ref['inner_iterations']}, errors {res['errors']} / {ref['errors']}")
    print(f"[corr-lm] largest value difference {np.abs(res['values'] - ref['values']).max():.3e}")
    assert res["iterations"] == ref["iterations"] and res["inner_iterations"] == ref["inner_iterations"]
    np.testing.assert_allclose(res["errors"], ref["errors"], rtol=1e-9)
    np.testing.assert_allclose(res["values"], ref["values"], atol=1e-9)
    base_v = pose3_ref.inverse(res["values"][0])
    for k in range(N):
        ang, tr = bench_lm.pose_error(base_v @ res["values"][k], base_t @ truth[k])
        assert ang < 0.015 and tr < 0.15, (k, ang, tr)
    nat_v, nat = tg.g.optimize(v0, max_iterations=30)
    assert nat["iterations"] == res["iterations"] and nat["inner_iterations"] == res["inner_iterations"]
    assert np.array_equal(nat_v, res["values"])  # the library's loop = the interpreter driving its three calls
    tg.close()


def test_rejected_trial_keeps_its_correspondences(gpu, submaps, chain):
    """linearize, a trial that is NOT accepted, another trial: with speculation the first trial queues a linearise at its values, which must search into the other
    correspondence set -- the second trial's error is still the host graph's error on the correspondences of the linearisation point"""
    _, _, _, v0 = submaps
    factors, host = chain
    got = {}
    for spec in (True, False):
        g = gpu.LevenbergMarquardtGraphGPU([], [], N, fixed=(0,), corr_factors=factors, corr_pairs=PAIRS)
        g.set_speculation(spec)
        g.set_values(v0)
        g.linearize()
        out = []
        for lam in (1e-12, 1e3):
            dx, b, c, e, v = g.try_lambda(lam, want_values=True)
            out.append((dx.copy(), b.copy(), c, e, v))
        got[spec] = out
        g.close()
    for (dx1, b1, c1, e1, v1), (dx2, b2, c2, e2, v2) in zip(got[True], got[False]):
        assert np.array_equal(dx1, dx2) and np.array_equal(b1, b2) and c1 == c2 and e1 == e2 and np.array_equal(v1, v2)
    host.linearize(v0)
    v_first, v_second = got[True][0][4], got[True][1][4]
    e_host = host.error(v_second)
    e_dev = got[True][1][3]
    # what the second trial would have returned had the speculative linearise overwritten the stored correspondences: the error on those of the FIRST trial's values
    host.linearize(v_first)
    e_wrong = host.error(v_second)
    print(f"[corr-lm] second trial: device {e_dev!r}, host on the linearisation point's correspondences {e_host!r}, on the first trial's {e_wrong!r}")
    assert abs(e_wrong - e_host) > 1e-6 * e_host  # the fixture tells the two apart
    assert abs(e_dev - e_host) <= 1e-9 * e_host


def test_mixed_graph(gpu, kitti07, submaps):
    vg_factors, vg_pairs, truth, v0, keep = kitti_graph(gpu, kitti07)
    truth, v0 = rigid(truth), rigid(v0)
    corr_pairs = [(0, 1), PLANE_EDGE]
    corr = [_factor(gpu, submaps, *p) for p in corr_pairs]
    sig = np.array([0.005] * 3 + [0.05] * 3)
    pose_factors = [gpu.PriorFactorPose3(0, truth[0], information=1e6 * np.eye(6)),
                    gpu.BetweenFactorPose3(0, 1, rigid((pose3_ref.inverse(truth[0]) @ truth[1])[None])[0], sigmas=sig)]
    F, Gc, P = len(vg_factors), len(corr), len(pose_factors)

    def make():
        return gpu.LevenbergMarquardtGraphGPU(vg_factors, vg_pairs, N, fixed=(), pose_factors=pose_factors, corr_factors=corr, corr_pairs=corr_pairs)

    g = make()
    g.set_values(v0)
    g.linearize()
    _, _, c, _ = g.try_lambda(1e-3)
    recs = g.records().cpu().numpy()
    assert recs.shape == (F + Gc + P, 122)
    assert abs(recs[:, 1].sum() - c) <= 1e-12 * c
    # the documented order: VGICP, then the correspondence factors (GICP before ICP), then the pose factors
    assert g.corr_order == [0, 1]
    deltas = bench_lm.inv_many(v0[[p[0] for p in corr_pairs]]) @ v0[[p[1] for p in corr_pairs]]
    for k, f in enumerate(corr):
        own = corr_graph_ref.record_of(f.linearize_delta(deltas[k]))
        assert own[0] == recs[F + k, 0] and own[0] > 1000  # the same inliers
        np.testing.assert_allclose(recs[F + k], own, rtol=1e-9, atol=1e-9 * np.abs(own).max())  # (the device's relative pose differs from numpy's by roundings)
    assert np.all(recs[F + Gc :, 0] == 0) and np.all(recs[:F, 0] > 0)  # pose factors carry no inliers, VGICP records do
    ref_v, ref_s = g.optimize(v0, max_iterations=6)
    g.close()
    for one_launch, spec in ((True, True), (False, True), (True, False), (False, False)):
        h = make()
        h.set_one_launch(one_launch)
        h.set_speculation(spec)
        v, s = h.optimize(v0, max_iterations=6)
        h.close()
        assert s == ref_s and np.array_equal(v, ref_v), (one_launch, spec)
    assert ref_s["iterations"] >= 2
    del keep


def test_one_free_pose(gpu, submaps):
    clouds, _, truth, _ = submaps
    f = gpu.IntegratedGICPFactorGPU(0, 1, clouds[0], clouds[1])
    start = np.stack([truth[0], truth[1] @ pose3_ref.expmap(np.array([0.01, -0.01, 0.01, 0.05, -0.05, 0.03]))])
    g = gpu.LevenbergMarquardtGraphGPU([], [], 2, fixed=(0,), corr_factors=[f], corr_pairs=[(0, 1)])
    assert g.n == 6  # one free pose: the dense 6 x 6 step
    v, s = g.optimize(start, max_iterations=60, relative_error_tol=0.0, absolute_error_tol=0.0)
    g.close()
    ref = lm_optimize(lambda values: [f.linearize(values)], lambda values: f.error(values), {0: start[0], 1: start[1]}, [0, 1], fixed=(0,), max_iter=60, rel_tol=-1.0)
    print(f"[corr-lm] one free pose: {s}, largest difference to the host loop {np.abs(v[1] - ref[1]).max():.3e}")
    assert np.array_equal(v[0], start[0])
    np.testing.assert_allclose(v[1], ref[1], atol=1e-9)

"""GPU tests of LOAM members in CorrespondenceFactorBatchGPU (gp_corr_batch_create_ex) and in the device-resident LM graph: every record and error of the batch
against the same factor objects' own single-factor calls, bit for bit (same terms, same 1024-point tiles, same finalize kernels per part, the two part records of
a combined member added in the same order in f64), the GICP / ICP members against a batch without LOAM members, the refusals, and a 3-pose chain in
LevenbergMarquardtGraphGPU against the loop driven from the host over the single-factor calls (tests/corr_graph_ref.py).

One batch of eight factors on kitti00, in the caller's order: combined (validation on), GICP, edge, ICP plane, plane, combined, ICP point, combined with an EMPTY
plane source -- so the record order (GICP, ICP, LOAM) differs from the caller's, two-part members sit between one-part members, and a part without points sits
beside one with."""
import ctypes as C

import numpy as np
import pytest

import bench_lm
import corr_graph_ref
import normals_ref
from helpers import BLOCKS, expmap, rigid

pytestmark = pytest.mark.gpu
XI = np.array([0.01, -0.02, 0.015, 0.10, -0.05, 0.03])
NEARBY = np.array([0.002, -0.001, 0.003, 0.01, 0.02, -0.01])
G = np.random.default_rng(11).normal(size=(3, 3))
KINDS = ["loam-validated", "gicp", "edge", "plane-icp", "plane", "loam", "point-icp", "loam-empty-plane"]
SIZES = [3000, 1025, 257, 1024, 1025, 255, 1, 700]
STARTS = [4000, 100, 500, 800, 2000, 3100, 7000, 9000]
SCALES = [1.0, 0.8, 1.2, 0.6, 1.0, 0.9, 1.1, 0.7]
FIELDS = BLOCKS + ["error", "num_inliers"]


def _same(a, b, what):
    for k in FIELDS:
        assert np.array_equal(getattr(a, k), getattr(b, k)), f"{what}: {k} differs"


@pytest.fixture(scope="module")
def scene(gpu, kitti00):
    tp, tc, sp, sc = kitti00["target_points"], kitti00["target_covs"], kitti00["source_points"], kitti00["source_covs"]
    normals = np.ascontiguousarray(normals_ref.reference_normals(tp, tc).astype(np.float32))
    tgt = gpu.PointCloudGPU(tp, tc, normals=normals)
    te, tpl = gpu.PointCloudGPU(np.ascontiguousarray(tp[0::2])), gpu.PointCloudGPU(np.ascontiguousarray(tp[1::2]))
    tree, tree_e, tree_p = gpu.KdTreeGPU(tgt), gpu.KdTreeGPU(te), gpu.KdTreeGPU(tpl)
    factors, keep = [], []
    for kind, n, a in zip(KINDS, SIZES, STARTS):
        src = gpu.PointCloudGPU(sp[a : a + n], sc[a : a + n])
        keep.append(src)
        if kind == "gicp":
            f = gpu.IntegratedGICPFactorGPU(0, 1, tgt, src)
        elif kind.endswith("-icp"):
            f = gpu.IntegratedICPFactorGPU(0, 1, tgt, src, target_tree=tree, use_point_to_plane=kind == "plane-icp")
        elif kind == "edge":
            f = gpu.IntegratedPointToEdgeFactorGPU(0, 1, te, src, target_tree=tree_e)
        elif kind == "plane":
            f = gpu.IntegratedPointToPlaneFactorGPU(0, 1, tpl, src, target_tree=tree_p, max_correspondence_distance=0.7)
        else:
            planes = src
            if kind == "loam-empty-plane":
                planes = gpu.PointCloudGPU(sp[:1])
                planes.num_points = 0  # an EMPTY source whose device pointer is valid: the plane part is created over zero points
                keep.append(planes)
            f = gpu.IntegratedLOAMFactorGPU(0, 1, te, tpl, src, planes, target_edges_tree=tree_e, target_planes_tree=tree_p)
            if kind == "loam-validated":
                f.set_enable_correspondence_validation(True)
        factors.append(f)
    deltas = np.stack([expmap(XI * s) for s in SCALES])
    near = deltas @ expmap(NEARBY)
    single = [f.linearize_delta(d) for f, d in zip(factors, deltas)]
    single_err = np.array([f.error({0: np.eye(4), 1: e}) for f, e in zip(factors, near)])
    batch = gpu.CorrespondenceFactorBatchGPU(factors)
    yield dict(factors=factors, keep=(keep, tgt, te, tpl, tree, tree_e, tree_p), deltas=deltas, near=near, single=single, single_err=single_err, batch=batch)
    batch.close()


def test_batch_equals_the_single_factor_calls(gpu, scene):
    b = scene["batch"]
    assert b.order == [1, 3, 6, 0, 2, 4, 5, 7] and b._lib.gp_corr_batch_size(b._h) == 8
    for corr_set in (None, 0, 1):  # the synchronous host-pose forms (set 0), the device-pose entry points into either set
        recs = b.linearize_deltas(scene["deltas"], corr_set=corr_set)
        errs = b.errors(scene["deltas"], scene["near"], corr_set=corr_set)
        for k, (L, S) in enumerate(zip(recs, scene["single"])):
            print(f"[loam-batch] set {corr_set} factor {k} ({KINDS[k]}, n={SIZES[k]}): inliers {L.num_inliers} / {S.num_inliers}, error {L.error!r} / {S.error!r}, "
                  f"error nearby {errs[k]!r} / {scene['single_err'][k]!r}")
        for k, (L, S) in enumerate(zip(recs, scene["single"])):
            _same(L, S, f"factor {k} ({KINDS[k]}), set {corr_set}")
        assert np.array_equal(errs, scene["single_err"])
    assert sum(S.num_inliers for S in scene["single"]) > 4000  # (the comparison is not one of empty records)
    # the validated member differs from the same factor without validation: the batch ran the validation kernel
    f = scene["factors"][0]
    f.set_enable_correspondence_validation(False)
    off = f.linearize_delta(scene["deltas"][0])
    f.set_enable_correspondence_validation(True)
    assert off.num_inliers > scene["single"][0].num_inliers and f.linearize_delta(scene["deltas"][0]).error == scene["single"][0].error


def test_general_path_equals_the_single_factor_calls(gpu, scene):
    deltas = scene["deltas"].copy()
    deltas[:, :3, :3] = deltas[:, :3, :3] @ (np.eye(3) + 1e-6 * G)  # orthonormal to 1e-6 only: rigid=False, the 92 explicit sums
    for corr_set in (None, 1):
        recs = scene["batch"].linearize_deltas(deltas, rigid=False, corr_set=corr_set)
        for k, (f, d, L) in enumerate(zip(scene["factors"], deltas, recs)):
            _same(L, f.linearize_delta(d), f"factor {k} ({KINDS[k]}), general path, set {corr_set}")


def test_gicp_and_icp_members_equal_a_batch_without_loam_members(gpu, scene):
    plain_idx = [k for k, kind in enumerate(KINDS) if kind == "gicp" or kind.endswith("-icp")]
    plain = gpu.CorrespondenceFactorBatchGPU([scene["factors"][k] for k in plain_idx])
    for rigid_, deltas in ((True, scene["deltas"]), (False, scene["deltas"] @ np.diag([1.0 + 1e-6, 1.0, 1.0, 1.0]))):
        full = scene["batch"].linearize_deltas(deltas, rigid=rigid_)
        part = plain.linearize_deltas(deltas[plain_idx], rigid=rigid_)
        for k, L in zip(plain_idx, part):
            _same(L, full[k], f"factor {k} ({KINDS[k]})")
    assert np.array_equal(plain.errors(scene["deltas"][plain_idx], scene["near"][plain_idx]), scene["batch"].errors(scene["deltas"], scene["near"])[plain_idx])
    plain.close()


def test_sets_keep_their_correspondences(gpu, scene):
    b = scene["batch"]
    A = scene["deltas"]
    B = A @ expmap([0.03, -0.02, 0.02, 0.3, -0.2, 0.1])  # far enough from A that the correspondences differ
    b.linearize_deltas(A, corr_set=0)
    before = b.errors(A, scene["near"], corr_set=0)
    b.linearize_deltas(B, corr_set=1)
    assert np.array_equal(before, b.errors(A, scene["near"], corr_set=0)) and np.array_equal(before, scene["single_err"])
    on_b = b.errors(B, scene["near"], corr_set=1)
    assert all(on_b[k] != before[k] for k in (0, 2, 4, 5))  # the fixture tells the two sets apart, for every kind of LOAM member


def test_refusals(gpu, scene):
    lib = gpu.load()
    keep, tgt, te, tpl, tree, tree_e, tree_p = scene["keep"]
    loam_only = [scene["factors"][k] for k in (0, 2, 4)]
    fresh = gpu.CorrespondenceFactorBatchGPU(loam_only)
    poses = np.ascontiguousarray(np.tile(np.eye(4).reshape(1, 16), (3, 1)))
    out = np.zeros(3)
    assert lib.gp_corr_batch_compute_error(fresh._h, poses.ctypes.data, poses.ctypes.data, out.ctypes.data) == 1  # GP_ERROR_INVALID_ARGUMENT: set 0 never linearised
    assert b"never linearised" in lib.gp_last_error()
    fresh.linearize_deltas(scene["deltas"][[0, 2, 4]], corr_set=0)
    with pytest.raises(gpu.GPError, match="never linearised"):
        fresh.errors(scene["deltas"][[0, 2, 4]], scene["near"][[0, 2, 4]], corr_set=1)
    fresh.close()
    tol = gpu.IntegratedPointToEdgeFactorGPU(0, 1, te, keep[2], target_tree=tree_e)
    tol.set_correspondence_update_tolerance(0.1, 0.1)
    with pytest.raises(gpu.GPError, match="tolerances"):
        gpu.CorrespondenceFactorBatchGPU([scene["factors"][1], tol])
    with pytest.raises(TypeError):
        gpu.CorrespondenceFactorBatchGPU([scene["factors"][0], object()])
    h = C.c_void_p()
    null = (C.c_void_p * 1)(None)
    assert lib.gp_corr_batch_create_ex(None, 0, None, 0, null, 1, None, C.byref(h)) == 1 and not h.value  # a NULL handle
    stream = C.c_void_p()
    gpu._capi.check(lib.gp_stream_create(C.byref(stream)), "gp_stream_create")
    with pytest.raises(gpu.GPError, match="stream"):
        gpu.CorrespondenceFactorBatchGPU(loam_only, stream=stream)  # the factors live on the NULL stream
    gpu._capi.check(lib.gp_stream_destroy(stream), "gp_stream_destroy")


# ---- a 3-pose chain in the device-resident LM graph ----
N = 3
PAIRS = [(0, 1), (1, 2), (0, 2)]


@pytest.fixture(scope="module")
def chain(gpu, kitti07):
    """the first three kitti07 submaps, even points as edge features and odd ones as plane features; a combined factor (validation on) on (0, 1), an edge factor on
    (1, 2), a combined factor on (0, 2); the host graph over the same factor objects"""
    edges, planes, te, tp_ = [], [], [], []
    for i in range(N):
        p = kitti07[f"points_{i}"]
        edges.append(gpu.PointCloudGPU(np.ascontiguousarray(p[0::2])))
        planes.append(gpu.PointCloudGPU(np.ascontiguousarray(p[1::2])))
        te.append(gpu.KdTreeGPU(edges[-1]))
        tp_.append(gpu.KdTreeGPU(planes[-1]))
    truth = rigid(np.stack([np.asarray(T, dtype=np.float64) for T in kitti07["poses"][:N]]))
    v0 = truth @ bench_lm.expmap_many(np.random.default_rng(8191).uniform(-0.02, 0.02, (N, 6)))
    v0[0] = truth[0]
    factors = []
    for k, (i, j) in enumerate(PAIRS):
        if k == 1:
            factors.append(gpu.IntegratedPointToEdgeFactorGPU(i, j, edges[i], edges[j], target_tree=te[i]))
        else:
            factors.append(gpu.IntegratedLOAMFactorGPU(i, j, edges[i], planes[i], edges[j], planes[j], target_edges_tree=te[i], target_planes_tree=tp_[i]))
    factors[0].set_enable_correspondence_validation(True)
    host = corr_graph_ref.HostCorrGraph([corr_graph_ref.DeviceFactor(f) for f in factors], PAIRS, N, fixed=0)
    return factors, host, rigid(v0), (edges, planes, te, tp_)


class _TrialGraph(bench_lm.GpuTrialGraph):
    """bench_lm's device-trial back end over a graph of correspondence factors, pose 0 held (as in test_corr_lm_gpu.py)"""

    def __init__(self, gpa, corr_factors, corr_pairs, num_poses):
        bench_lm._Graph.__init__(self, corr_pairs, num_poses, fixed=0)
        self.g = gpa.LevenbergMarquardtGraphGPU([], [], num_poses, fixed=(0,), corr_factors=corr_factors, corr_pairs=corr_pairs)
        self.sync_phases = False
        self._trial = None
        self._trial_error = None


def test_trial_follows_the_host_driven_loop(gpu, chain):
    """the tolerances of test_corr_lm_gpu.py::test_trial_follows_the_host_driven_loop: the same iterations and trials, errors to 1e-9 relative, values to 1e-9"""
    factors, host, v0, _ = chain
    ref = bench_lm.run_lm(host, v0, max_iterations=30)
    tg = _TrialGraph(gpu, factors, PAIRS, N)
    res = bench_lm.run_lm(tg, v0, max_iterations=30)
    print(f"[loam-lm] iterations {res['iterations']} / {ref['iterations']}, trials {res['inner_iterations']} / {ref['inner_iterations']}, errors {res['errors']} / {ref['errors']}")
    print(f"[loam-lm] largest value difference {np.abs(res['values'] - ref['values']).max():.3e}")
    assert res["iterations"] == ref["iterations"] and res["inner_iterations"] == ref["inner_iterations"] and ref["iterations"] >= 2
    np.testing.assert_allclose(res["errors"], ref["errors"], rtol=1e-9)
    np.testing.assert_allclose(res["values"], ref["values"], atol=1e-9)
    nat_v, nat = tg.g.optimize(v0, max_iterations=30)
    assert nat["iterations"] == res["iterations"] and nat["inner_iterations"] == res["inner_iterations"]
    assert np.array_equal(nat_v, res["values"])  # the library's loop = the interpreter driving its three calls
    tg.close()


def test_rejected_trial_keeps_its_correspondences(gpu, chain):
    """linearize, a trial that is NOT accepted, another trial: with speculation the first trial queues a linearise at its values, which must search (and validate) into
    the other correspondence set -- the second trial's error is still the host graph's error on the correspondences of the linearisation point"""
    factors, host, v0, _ = chain
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
    host.linearize(v_first)  # what the second trial would have returned had the speculative linearise overwritten the stored correspondences
    e_wrong = host.error(v_second)
    print(f"[loam-lm] second trial: device {e_dev!r}, host on the linearisation point's correspondences {e_host!r}, on the first trial's {e_wrong!r}")
    assert abs(e_wrong - e_host) > 1e-6 * e_host  # the fixture tells the two apart
    assert abs(e_dev - e_host) <= 1e-9 * e_host

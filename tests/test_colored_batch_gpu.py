"""GPU tests of colored GICP members in CorrespondenceFactorBatchGPU (gp_corr_batch_create_ex2) and in the device-resident LM graph: every record and error of the
batch against the same factor objects' own single-factor calls, bit for bit (the same term on the same operands, the same 1024-point tiles, the same finalize
kernels over a part's rows), the GICP / ICP members against a batch without colored members, the two correspondence sets, the creation-time reads, the refusals,
and a 3-pose graph in LevenbergMarquardtGraphGPU against the loop driven from the host over the single-factor calls (tests/corr_graph_ref.py).

The clouds are those of test_colored_gicp_gpu.py: colored_ref.two_plane_cloud() (4,000 points) with device-estimated covariances, normals and gradients as the
target, slices of colored_ref.moved_copy() (2,500 points, every 20th pushed 0.15 .. 0.8 m off) as the sources.  One batch of eight factors, in the caller's order:
colored 2500, GICP 1025, colored 1024, point-to-plane ICP 700, colored 1025, colored 1, colored over an EMPTY source, colored 257 with weight 0.6 and a 0.3 m
cut-off -- so the record order (GICP, ICP, colored) differs from the caller's, colored members sit between the other kinds, 1024 / 1025 / 1 are the tile
boundaries, a part without rows sits beside parts with rows, and one member's cut-off in the search table differs from the others'."""
import ctypes as C

import numpy as np
import pytest

import bench_lm
import colored_ref
import corr_graph_ref
from helpers import BLOCKS, expmap, rigid

pytestmark = pytest.mark.gpu
MARGIN = 1e-9
XI = np.array([0.01, -0.02, 0.015, 0.10, -0.05, 0.03])
NEARBY = np.array([0.002, -0.001, 0.003, 0.01, 0.02, -0.01])
G = np.random.default_rng(11).normal(size=(3, 3))
T_GT = expmap(XI)
KINDS = ["colored", "gicp", "colored", "plane-icp", "colored", "colored", "colored-empty", "colored-0.3m"]
SIZES = [2500, 1025, 1024, 700, 1025, 1, 0, 257]
STARTS = [0, 100, 1000, 800, 1400, 2401, 0, 2000]  # slices of the moved copy
SCALES = [1.0, 0.8, 1.2, 0.6, 1.1, 0.9, 1.0, 0.7]  # member k is linearised at Expmap(SCALES[k] XI): up to 0.4 |XI| from the aligned pose
COLORED = [k for k, kind in enumerate(KINDS) if kind.startswith("colored")]
FIELDS = BLOCKS + ["error", "num_inliers"]


def _same(a, b, what):
    for k in FIELDS:
        assert np.array_equal(getattr(a, k), getattr(b, k)), f"{what}: {k} differs"


def _cloud(gpu, points, intensities):
    """a cloud on the device with its estimated covariances and normals, its search structure and its intensity gradients"""
    frame = gpu.PointCloudGPU(points, intensities=intensities)
    assert gpu.estimate_normals_covariances_gpu(frame, 10) == 0
    tree = gpu.KdTreeGPU(frame)
    grads = gpu.estimate_intensity_gradients_gpu(frame, 10)
    assert grads.num_short == 0
    return frame, tree, grads


def _colored(gpu, scene, src, cutoff=1.0, weight=0.25, **kw):
    return gpu.IntegratedColoredGICPFactorGPU(0, 1, scene["tgt"], src, target_tree=scene["tree"], target_gradients=scene["grads"], max_correspondence_distance=cutoff,
                                              photometric_term_weight=weight, **kw)


def _slice(gpu, scene, k, kind):
    a, n = STARTS[k], SIZES[k]
    sp, sI, scov = scene["sp"], scene["sI"], scene["scov"]
    if kind == "colored-empty":
        src = gpu.PointCloudGPU(sp[:1], covs=scov[:1], intensities=sI[:1])
        src.num_points = 0  # an EMPTY source whose device pointers are valid: the factor is created over zero points
        return src
    if kind.startswith("colored"):
        return gpu.PointCloudGPU(sp[a : a + n], covs=scov[a : a + n], intensities=sI[a : a + n])
    return gpu.PointCloudGPU(sp[a : a + n], covs=scov[a : a + n])  # (covariances only, as the GICP factor needs; the ICP factor reads the points)


@pytest.fixture(scope="module")
def scene(gpu):
    tp, tI = colored_ref.two_plane_cloud()
    tgt, tree, grads = _cloud(gpu, tp, tI)
    sp, sI = colored_ref.moved_copy(tp, tI, T_GT)
    whole = gpu.PointCloudGPU(sp)
    assert gpu.estimate_covariances_gpu(whole, 10) == 0
    s = dict(tgt=tgt, tree=tree, grads=grads, sp=sp, sI=sI, scov=whole.download("covs"))
    factors, keep = [], []
    for k, kind in enumerate(KINDS):
        src = _slice(gpu, s, k, kind)
        keep.append(src)
        if kind == "gicp":
            f = gpu.IntegratedGICPFactorGPU(0, 1, tgt, src)
        elif kind == "plane-icp":
            f = gpu.IntegratedICPFactorGPU(0, 1, tgt, src, target_tree=tree, use_point_to_plane=True)
        elif kind == "colored-0.3m":
            f = _colored(gpu, s, src, cutoff=0.3, weight=0.6)
        else:
            f = _colored(gpu, s, src)
        factors.append(f)
    deltas = np.stack([expmap(XI * c) for c in SCALES])
    near = deltas @ expmap(NEARBY)
    single = [f.linearize_delta(d) for f, d in zip(factors, deltas)]
    single_err = np.array([f.error({0: np.eye(4), 1: e}) for f, e in zip(factors, near)])
    batch = gpu.CorrespondenceFactorBatchGPU(factors)
    s.update(factors=factors, keep=keep, deltas=deltas, near=near, single=single, single_err=single_err, batch=batch)
    yield s
    batch.close()


def test_batch_equals_the_single_factor_calls(gpu, scene):
    b = scene["batch"]
    assert b.order == [1, 3, 0, 2, 4, 5, 6, 7] and b._lib.gp_corr_batch_size(b._h) == 8
    for corr_set in (None, 0, 1):  # the synchronous host-pose forms (set 0), the device-pose entry points into either set
        recs = b.linearize_deltas(scene["deltas"], corr_set=corr_set)
        errs = b.errors(scene["deltas"], scene["near"], corr_set=corr_set)
        for k, (L, S) in enumerate(zip(recs, scene["single"])):
            print(f"[colored-batch] set {corr_set} factor {k} ({KINDS[k]}, n={SIZES[k]}): inliers {L.num_inliers} / {S.num_inliers}, error {L.error!r} / {S.error!r}, "
                  f"error nearby {errs[k]!r} / {scene['single_err'][k]!r}")
        for k, (L, S) in enumerate(zip(recs, scene["single"])):
            _same(L, S, f"factor {k} ({KINDS[k]}), set {corr_set}")
        assert np.array_equal(errs, scene["single_err"])
    assert sum(S.num_inliers for S in scene["single"]) > 4000  # (the comparison is not one of empty records)
    assert all(scene["single"][k].num_inliers > 0 for k in COLORED if SIZES[k] > 0) and scene["single"][6].num_inliers == 0
    # the per-member cut-off in the search table: 0.3 m drops points of the slice that 1 m keeps
    wide = _colored(gpu, scene, scene["keep"][7], cutoff=1.0, weight=0.6).linearize_delta(scene["deltas"][7])
    print(f"[colored-batch] the 257-point slice: {scene['single'][7].num_inliers} inliers at 0.3 m, {wide.num_inliers} at 1 m")
    assert scene["single"][7].num_inliers < wide.num_inliers


def test_general_path_equals_the_single_factor_calls(gpu, scene):
    deltas = scene["deltas"].copy()
    deltas[:, :3, :3] = deltas[:, :3, :3] @ (np.eye(3) + 1e-6 * G)  # orthonormal to 1e-6 only: rigid=False, the 92 explicit sums
    for corr_set in (None, 1):
        recs = scene["batch"].linearize_deltas(deltas, rigid=False, corr_set=corr_set)
        for k, (f, d, L) in enumerate(zip(scene["factors"], deltas, recs)):
            _same(L, f.linearize_delta(d), f"factor {k} ({KINDS[k]}), general path, set {corr_set}")
    assert sum(L.num_inliers for L in recs) > 4000


def test_gicp_and_icp_members_equal_a_batch_without_colored_members(gpu, scene):
    plain_idx = [k for k, kind in enumerate(KINDS) if not kind.startswith("colored")]
    plain = gpu.CorrespondenceFactorBatchGPU([scene["factors"][k] for k in plain_idx])
    assert plain.order == [0, 1]
    for rigid_, deltas in ((True, scene["deltas"]), (False, scene["deltas"] @ np.diag([1.0 + 1e-6, 1.0, 1.0, 1.0]))):
        full = scene["batch"].linearize_deltas(deltas, rigid=rigid_)
        part = plain.linearize_deltas(deltas[plain_idx], rigid=rigid_)
        for k, L in zip(plain_idx, part):
            _same(L, full[k], f"factor {k} ({KINDS[k]})")
            assert L.num_inliers > 500
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
    print(f"[colored-batch] errors nearby on set 0 {before}, on set 1 {on_b}")
    assert all(on_b[k] != before[k] for k in COLORED if SIZES[k] > 0)  # the fixture tells the two sets apart, for every colored member that has points


def test_weight_and_cut_off_are_read_at_creation(gpu, scene):
    """a set_* on the factor after the batch exists does not reach it; a batch created afterwards reads the new value (own factor objects: the shared ones stay as they are)"""
    f = _colored(gpu, scene, scene["keep"][2])
    g = gpu.IntegratedGICPFactorGPU(0, 1, scene["tgt"], scene["keep"][1])
    deltas = scene["deltas"][[2, 1]]
    before = f.linearize_delta(deltas[0])
    _same(before, scene["single"][2], "a second factor over the same slice")
    old = gpu.CorrespondenceFactorBatchGPU([f, g])
    f.set_photometric_term_weight(0.1)
    after = f.linearize_delta(deltas[0])
    assert after.error != before.error and after.num_inliers == before.num_inliers
    _same(old.linearize_deltas(deltas)[0], before, "the batch created before the change")
    new = gpu.CorrespondenceFactorBatchGPU([f, g])
    _same(new.linearize_deltas(deltas)[0], after, "a batch created after the change")
    f.set_max_correspondence_distance(0.05)
    narrow = f.linearize_delta(deltas[0])
    assert 0 < narrow.num_inliers < before.num_inliers
    _same(new.linearize_deltas(deltas)[0], after, "the cut-off of an existing batch")
    newest = gpu.CorrespondenceFactorBatchGPU([f, g])
    _same(newest.linearize_deltas(deltas)[0], narrow, "a batch created after the cut-off changed")
    for b in (old, new, newest):
        b.close()


def test_refusals(gpu, scene):
    lib = gpu.load()
    colored_only = [scene["factors"][k] for k in (0, 2, 7)]
    fresh = gpu.CorrespondenceFactorBatchGPU(colored_only)
    poses = np.ascontiguousarray(np.tile(np.eye(4).reshape(1, 16), (3, 1)))
    out = np.zeros(3)
    assert lib.gp_corr_batch_compute_error(fresh._h, poses.ctypes.data, poses.ctypes.data, out.ctypes.data) == 1  # GP_ERROR_INVALID_ARGUMENT: set 0 never linearised
    assert b"never linearised" in lib.gp_last_error()
    fresh.linearize_deltas(scene["deltas"][[0, 2, 7]], corr_set=0)
    with pytest.raises(gpu.GPError, match="never linearised"):
        fresh.errors(scene["deltas"][[0, 2, 7]], scene["near"][[0, 2, 7]], corr_set=1)
    fresh.close()
    tol = _colored(gpu, scene, scene["keep"][2])
    tol.set_correspondence_update_tolerance(0.1, 0.1)
    with pytest.raises(gpu.GPError, match="tolerances"):
        gpu.CorrespondenceFactorBatchGPU([scene["factors"][1], tol])
    with pytest.raises(TypeError):
        gpu.CorrespondenceFactorBatchGPU([scene["factors"][0], object()])
    h = C.c_void_p()
    null = (C.c_void_p * 1)(None)
    assert lib.gp_corr_batch_create_ex2(None, 0, None, 0, None, 0, null, 1, None, C.byref(h)) == 1 and not h.value  # a NULL handle
    stream = C.c_void_p()
    gpu._capi.check(lib.gp_stream_create(C.byref(stream)), "gp_stream_create")
    with pytest.raises(gpu.GPError, match="stream"):
        gpu.CorrespondenceFactorBatchGPU(colored_only, stream=stream)  # the factors live on the NULL stream
    gpu._capi.check(lib.gp_stream_destroy(stream), "gp_stream_destroy")


# ---- a 3-pose graph in the device-resident LM graph ----
N = 3
PAIRS = [(0, 1), (1, 2), (0, 2)]
TRUTH = np.stack([np.eye(4), T_GT, expmap([-0.015, 0.01, 0.02, -0.06, 0.08, 0.04])])
COPY_SEEDS = (21, 22)
START_SEED = 8191


def chain_clouds():
    """(points, intensities) of the three clouds -- the two-plane cloud as pose 0, two moved copies of it (different seeds, 2,500 points each) at TRUTH[1] and
    TRUTH[2] -- and the start: the truth perturbed by uniform(-0.02, 0.02) per coordinate, pose 0 held"""
    tp, tI = colored_ref.two_plane_cloud()
    clouds = [(tp, tI)] + [colored_ref.moved_copy(tp, tI, TRUTH[k + 1], seed=s) for k, s in enumerate(COPY_SEEDS)]
    v0 = TRUTH @ bench_lm.expmap_many(np.random.default_rng(START_SEED).uniform(-0.02, 0.02, (N, 6)))
    v0[0] = TRUTH[0]
    return clouds, rigid(v0)


def chain_margins(clouds, v0):
    """per pair, the smallest relative tie gap and cut-off gap (squared distances) of the brute-force search at the start"""
    out = []
    for i, j in PAIRS:
        (tp, tI), (sp, sI) = clouds[i], clouds[j]
        eye = np.tile(np.eye(3, dtype=np.float32), (len(tp), 1, 1))
        ref = colored_ref.ColoredGICPFactorRef(tp, eye, np.zeros_like(tp), tI, np.zeros_like(tp), sp, eye[: len(sp)], sI)  # (the margins read the points alone)
        tie, cut = ref.margins(np.linalg.inv(v0[i]) @ v0[j])
        out.append((float(tie.min()), float(cut.min())))
    return out


@pytest.fixture(scope="module")
def chain(gpu):
    """colored factors on (0, 1), (1, 2) and (0, 2), every cloud with its own covariances, normals, intensities and gradients; the host graph over the same objects"""
    clouds, v0 = chain_clouds()
    for (i, j), (tie, cut) in zip(PAIRS, chain_margins(clouds, v0)):
        print(f"[colored-lm] pair ({i}, {j}) at the start: smallest tie gap {tie:.3e}, smallest cut-off gap {cut:.3e} (relative, squared distances)")
        assert tie > MARGIN and cut > MARGIN, f"pair ({i}, {j}): a correspondence two searches could decide differently (tie {tie:.2e}, cut-off {cut:.2e})"
    dev = [_cloud(gpu, p, I) for p, I in clouds]
    factors = [gpu.IntegratedColoredGICPFactorGPU(i, j, dev[i][0], dev[j][0], target_tree=dev[i][1], target_gradients=dev[i][2]) for i, j in PAIRS]
    host = corr_graph_ref.HostCorrGraph([corr_graph_ref.DeviceFactor(f) for f in factors], PAIRS, N, fixed=0)
    return factors, host, v0, dev


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
    assert tg.g.corr_order == [0, 1, 2]
    res = bench_lm.run_lm(tg, v0, max_iterations=30)
    print(f"[colored-lm] iterations {res['iterations']} / {ref['iterations']}, trials {res['inner_iterations']} / {ref['inner_iterations']}, errors {res['errors']} / {ref['errors']}")
    print(f"[colored-lm] largest value difference {np.abs(res['values'] - ref['values']).max():.3e}")
    assert res["iterations"] == ref["iterations"] and res["inner_iterations"] == ref["inner_iterations"] and ref["iterations"] >= 2
    np.testing.assert_allclose(res["errors"], ref["errors"], rtol=1e-9)
    np.testing.assert_allclose(res["values"], ref["values"], atol=1e-9)
    nat_v, nat = tg.g.optimize(v0, max_iterations=30)
    assert nat["iterations"] == res["iterations"] and nat["inner_iterations"] == res["inner_iterations"]
    assert np.array_equal(nat_v, res["values"])  # the library's loop = the interpreter driving its three calls
    tg.close()


def test_rejected_trial_keeps_its_correspondences(gpu, chain):
    """linearize, a trial that is NOT accepted, another trial: with speculation the first trial queues a linearise at its values, which must search into the other
    correspondence set -- the second trial's error is still the host graph's error on the correspondences of the linearisation point"""
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
    print(f"[colored-lm] second trial: device {e_dev!r}, host on the linearisation point's correspondences {e_host!r}, on the first trial's {e_wrong!r}")
    assert abs(e_wrong - e_host) > 1e-6 * e_host  # the fixture tells the two apart
    assert abs(e_dev - e_host) <= 1e-9 * e_host

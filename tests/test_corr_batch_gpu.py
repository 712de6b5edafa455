"""GPU tests of CorrespondenceFactorBatchGPU (gp_corr_batch_*, csrc/gp_corr_batch.hip): GICP and ICP factors linearised and evaluated together with their poses in
device memory, against (a) the same factor objects' own single-factor calls -- bit for bit: the batch runs the single call's terms on the same 1024-point tiles and
the same finalize kernels over each factor's contiguous rows, so no order of sums differs -- and (b) the f64 references of those factors (icp_ref, the oracle's GICP)
at the project's gate for them, 1e-7.

One batch of seven factors on kitti00, in this order: GICP, GICP, ICP point, ICP point, ICP plane, ICP plane, GICP over source slices of 1, 255, 257, 1024, 1025, 0
and 3000 points -- factor and tile boundaries that coincide (1024) and do not, an empty factor, and a GICP factor BEHIND the ICP ones in the caller's list, so the
batch's record order (GICP first) differs from the caller's order."""
import ctypes as C

import numpy as np
import pytest

import icp_ref
import normals_ref
import oracle
from helpers import BLOCKS, assert_linearized_close, expmap

pytestmark = pytest.mark.gpu
PARITY_TOL = 1e-7  # the gate of test_icp_gpu.py / test_knn_gicp_gpu.py
MARGIN = 1e-9
XI = np.array([0.01, -0.02, 0.015, 0.10, -0.05, 0.03])
NEARBY = np.array([0.002, -0.001, 0.003, 0.01, 0.02, -0.01])
G = np.random.default_rng(11).normal(size=(3, 3))
KINDS = ["gicp", "gicp", "point", "point", "plane", "plane", "gicp"]
SIZES = [1, 255, 257, 1024, 1025, 0, 3000]
STARTS = [100, 200, 500, 800, 2000, 3100, 4000]
# a pose of its own per factor: XI scaled and with signs flipped
POSES = [expmap(XI * s * sg) for s, sg in zip([1.0, 0.8, 1.2, 0.6, 1.0, 0.9, 1.1],
                                              [np.ones(6), [1, -1, 1, 1, -1, 1], [-1, 1, 1, -1, 1, 1], np.ones(6), [1, 1, -1, 1, 1, -1], np.ones(6), [-1, -1, 1, 1, 1, -1]])]
FIELDS = BLOCKS + ["error", "num_inliers"]


def _same(a, b, what):
    for k in FIELDS:
        assert np.array_equal(getattr(a, k), getattr(b, k)), f"{what}: {k} differs"
    assert isinstance(a.num_inliers, int) and a.num_inliers == b.num_inliers


@pytest.fixture(scope="module")
def scene(gpu, kitti00):
    """the clouds, the seven factor objects, their batch, and -- computed ONCE with the factors' own calls -- each factor's record at its pose and its error at the
    nearby pose"""
    tp, tc, sp, sc = kitti00["target_points"], kitti00["target_covs"], kitti00["source_points"], kitti00["source_covs"]
    normals = np.ascontiguousarray(normals_ref.reference_normals(tp, tc).astype(np.float32))
    tgt = gpu.PointCloudGPU(tp, tc, normals=normals)
    tree = gpu.KdTreeGPU(tgt)
    factors, srcs, slices = [], [], []
    for kind, n, a in zip(KINDS, SIZES, STARTS):
        sl = slice(a, a + max(n, 1))
        src = gpu.PointCloudGPU(sp[sl], sc[sl])
        if n == 0:
            src.num_points = 0  # an EMPTY source whose device pointers are valid (an empty tensor has none): the factor is created over zero points
        srcs.append(src)
        slices.append(slice(a, a + n))
        if kind == "gicp":
            factors.append(gpu.IntegratedGICPFactorGPU(0, 1, tgt, src))
        else:
            factors.append(gpu.IntegratedICPFactorGPU(0, 1, tgt, src, target_tree=tree, use_point_to_plane=kind == "plane"))
    deltas = np.stack(POSES)
    near = deltas @ expmap(NEARBY)
    single = [f.linearize_delta(d) for f, d in zip(factors, deltas)]
    single_err = np.array([f.error({0: np.eye(4), 1: e}) for f, e in zip(factors, near)])
    batch = gpu.CorrespondenceFactorBatchGPU(factors)
    yield dict(tp=tp, tc=tc, sp=sp, sc=sc, normals=normals, tgt=tgt, tree=tree, factors=factors, srcs=srcs, slices=slices, deltas=deltas, near=near, single=single,
               single_err=single_err, batch=batch)
    batch.close()


def test_batch_equals_the_single_factor_calls(gpu, scene):
    """every record and every error of the batch has the bits of the factor's own call at the same pose (no order of sums differs: see the module docstring)"""
    b = scene["batch"]
    assert b.order == [0, 1, 6, 2, 3, 4, 5] and b._lib.gp_corr_batch_size(b._h) == 7
    recs = b.linearize_deltas(scene["deltas"])
    errs = b.errors(scene["deltas"], scene["near"])
    for k, (L, S) in enumerate(zip(recs, scene["single"])):
        print(f"[corr-batch] factor {k} ({KINDS[k]}, n={SIZES[k]}): inliers {L.num_inliers} / {S.num_inliers}, error {L.error!r} / {S.error!r}, "
              f"error nearby {errs[k]!r} / {scene['single_err'][k]!r}")
    for k, (L, S) in enumerate(zip(recs, scene["single"])):
        _same(L, S, f"factor {k}")
    assert np.array_equal(errs, scene["single_err"])
    assert sum(L.num_inliers for L in recs) > 3000  # (the comparison is not one of empty records)
    # the device-pose entry points into set 1 = the synchronous host-pose forms on set 0
    recs1 = b.linearize_deltas(scene["deltas"], corr_set=1)
    for k, (L, S) in enumerate(zip(recs1, scene["single"])):
        _same(L, S, f"factor {k}, set 1")
    assert np.array_equal(b.errors(scene["deltas"], scene["near"], corr_set=1), scene["single_err"])


@pytest.mark.parametrize("k", [2, 4, 6], ids=["icp-point-257", "icp-plane-1025", "gicp-3000"])
def test_batch_records_against_f64(gpu, scene, k):
    tp, sp = scene["tp"], scene["sp"][scene["slices"][k]]
    delta, near = scene["deltas"][k], scene["near"][k]
    ref = icp_ref.ICPFactorRef(tp, sp, scene["normals"], use_point_to_plane=KINDS[k] == "plane")
    tie, cut = ref.margins(delta)
    print(f"[corr-batch] factor {k}: smallest tie gap {tie.min():.3e}, smallest cut-off gap {cut.min():.3e}")
    assert tie.min() > MARGIN and cut.min() > MARGIN  # a condition on the inputs: no correspondence two f64 searches could decide differently
    L = scene["batch"].linearize_deltas(scene["deltas"])[k]
    e = scene["batch"].errors(scene["deltas"], scene["near"])[k]
    if KINDS[k] == "gicp":
        fo = oracle.OracleGICPFactor(tp, scene["tc"], sp, scene["sc"][scene["slices"][k]], 4)
        assert_linearized_close(L, fo.linearize(delta), PARITY_TOL, f"factor {k}")
        er = fo.evaluate(near).error
    else:
        assert_linearized_close(L, ref.linearize(delta), PARITY_TOL, f"factor {k}")
        er = ref.error(near)
    assert L.num_inliers > 0.5 * SIZES[k]
    assert abs(e - er) <= PARITY_TOL * er, (e, er)


def test_general_path_equals_the_single_factor_calls(gpu, scene):
    """poses whose 3x3 block is orthonormal to 1e-6 only: the batch is told so (rigid=False: the 92 explicit sums), the factors' own calls find out themselves"""
    deltas = scene["deltas"].copy()
    deltas[:, :3, :3] = deltas[:, :3, :3] @ (np.eye(3) + 1e-6 * G)
    assert np.abs(deltas[0, :3, :3].T @ deltas[0, :3, :3] - np.eye(3)).max() > 1e-7
    recs = scene["batch"].linearize_deltas(deltas, rigid=False)
    for k, (f, d, L) in enumerate(zip(scene["factors"], deltas, recs)):
        _same(L, f.linearize_delta(d), f"factor {k}, general path")
    assert sum(L.num_inliers for L in recs) > 3000


def test_empty_and_beyond_cut_off_factors(gpu, scene):
    far = expmap([0.0, 0.0, 0.0, 0.0, 0.0, 500.0])
    deltas = scene["deltas"].copy()
    deltas[3] = far  # the 1024-point factor, between two others
    recs = scene["batch"].linearize_deltas(deltas)
    errs = scene["batch"].errors(deltas, deltas @ expmap(NEARBY))
    for k in (3, 5):  # posed 500 m away / no points
        assert recs[k].num_inliers == 0 and recs[k].error == 0.0 and errs[k] == 0.0
        for name in BLOCKS:
            assert not np.any(getattr(recs[k], name)), (k, name)
    for k in (0, 1, 2, 4, 6):  # the neighbours: the bits of the single-factor calls, as in the first test
        _same(recs[k], scene["single"][k], f"factor {k} beside empty ones")
        assert errs[k] == scene["single_err"][k]


def test_sets_keep_their_correspondences(gpu, scene):
    b = scene["batch"]
    A = scene["deltas"]
    B = A @ expmap([0.03, -0.02, 0.02, 0.3, -0.2, 0.1])  # far enough from A that the correspondences differ
    eval_at = scene["near"]
    b.linearize_deltas(A, corr_set=0)
    before = b.errors(A, eval_at, corr_set=0)
    recs_b = b.linearize_deltas(B, corr_set=1)
    after = b.errors(A, eval_at, corr_set=0)
    assert np.array_equal(before, after) and np.array_equal(before, scene["single_err"])
    on_b = b.errors(B, eval_at, corr_set=1)
    assert not np.array_equal(on_b, before)  # the fixture tells the two sets apart
    assert any(L.num_inliers != S.num_inliers for L, S in zip(recs_b, scene["single"]))


def test_refusals(gpu, scene):
    lib = gpu.load()
    fresh = gpu.CorrespondenceFactorBatchGPU(scene["factors"][:3])
    poses = np.ascontiguousarray(np.tile(np.eye(4).reshape(1, 16), (3, 1)))
    out = np.zeros(3)
    assert lib.gp_corr_batch_compute_error(fresh._h, poses.ctypes.data, poses.ctypes.data, out.ctypes.data) == 1  # GP_ERROR_INVALID_ARGUMENT: set 0 never linearised
    assert b"never linearised" in lib.gp_last_error()
    fresh.linearize_deltas(scene["deltas"][:3], corr_set=0)
    with pytest.raises(gpu.GPError, match="never linearised"):
        fresh.errors(scene["deltas"][:3], scene["near"][:3], corr_set=1)
    fresh.close()
    tol = gpu.IntegratedICPFactorGPU(0, 1, scene["tgt"], scene["srcs"][2], target_tree=scene["tree"])
    tol.set_correspondence_update_tolerance(0.1, 0.1)
    with pytest.raises(gpu.GPError, match="tolerances"):
        gpu.CorrespondenceFactorBatchGPU([scene["factors"][0], tol])
    with pytest.raises(gpu.GPError, match="empty batch"):
        gpu.CorrespondenceFactorBatchGPU([])
    h = C.c_void_p()
    null = (C.c_void_p * 1)(None)
    assert lib.gp_corr_batch_create(null, 1, None, 0, None, C.byref(h)) == 1 and not h.value  # a NULL handle
    stream = C.c_void_p()
    gpu._capi.check(lib.gp_stream_create(C.byref(stream)), "gp_stream_create")
    with pytest.raises(gpu.GPError, match="stream"):
        gpu.CorrespondenceFactorBatchGPU(scene["factors"][:2], stream=stream)  # the factors live on the NULL stream
    gpu._capi.check(lib.gp_stream_destroy(stream), "gp_stream_destroy")


def test_two_linearises_are_bit_identical(gpu, scene):
    for rigid, deltas in ((True, scene["deltas"]), (False, scene["deltas"] @ np.diag([1.0 + 1e-6, 1.0, 1.0, 1.0]))):
        a = scene["batch"].linearize_deltas(deltas, rigid=rigid)
        b = scene["batch"].linearize_deltas(deltas, rigid=rigid)
        other = gpu.CorrespondenceFactorBatchGPU(scene["factors"])
        c = other.linearize_deltas(deltas, rigid=rigid, corr_set=1)
        other.close()
        for k in range(len(a)):
            _same(a[k], b[k], f"factor {k}, second linearise")
            _same(a[k], c[k], f"factor {k}, another batch")

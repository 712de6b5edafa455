"""All six part kinds of CorrespondenceFactorBatchGPU in ONE batch (gp_corr_batch.hip: one tile kernel template over GICP, ICP point, ICP plane, colored GICP, LOAM
edge, LOAM plane), interleaved in the caller's order: every record and error of the batch has the bytes of the member's own linearize_delta / error at the same
poses -- both correspondence sets and the host-pose form, the rigid and the general kernels, and a second pass that gives the same bytes again.  The per-kind
batch tests (test_corr_batch_gpu.py, test_loam_batch_gpu.py, test_colored_batch_gpu.py) hold this kind by kind; none has every kind and both LOAM shapes together.

Slices of kitti00 at the tile boundaries (1, 255, 257, 1024, 1025 points: 1025 straddles two tiles); the colored members read an intensity made up from the
coordinates, with the gradients estimated on the device.  Two combined LOAM members (one with the validation on) make the parts outnumber the members, so the
part-pose and combine launches run; the edge-only member is a one-part LOAM member beside them."""
import numpy as np
import pytest

import normals_ref
from helpers import BLOCKS, expmap

pytestmark = pytest.mark.gpu
XI = np.array([0.01, -0.02, 0.015, 0.10, -0.05, 0.03])
NEARBY = np.array([0.002, -0.001, 0.003, 0.01, 0.02, -0.01])
G = np.random.default_rng(11).normal(size=(3, 3))
KINDS = ["loam", "gicp", "edge", "colored", "point-icp", "loam-validated", "plane-icp", "colored"]
SIZES = [257, 1, 255, 1025, 1024, 1025, 257, 255]
STARTS = [3100, 7000, 500, 2000, 800, 4000, 100, 6000]
SCALES = [1.0, 0.8, 1.2, 0.6, 1.0, 0.9, 1.1, 0.7]
FIELDS = BLOCKS + ["error", "num_inliers"]


def _intensity(p):
    return np.ascontiguousarray((0.5 + 0.25 * np.sin(0.7 * p[:, 0]) * np.cos(0.5 * p[:, 1]) + 0.1 * np.sin(1.3 * p[:, 2])).astype(np.float32))


def _same(a, b, what):
    for k in FIELDS:
        assert np.array_equal(getattr(a, k), getattr(b, k)), f"{what}: {k} differs"


@pytest.fixture(scope="module")
def scene(gpu, kitti00):
    tp, tc, sp, sc = kitti00["target_points"], kitti00["target_covs"], kitti00["source_points"], kitti00["source_covs"]
    normals = np.ascontiguousarray(normals_ref.reference_normals(tp, tc).astype(np.float32))
    tgt = gpu.PointCloudGPU(tp, tc, normals=normals, intensities=_intensity(tp))
    te, tpl = gpu.PointCloudGPU(np.ascontiguousarray(tp[0::2])), gpu.PointCloudGPU(np.ascontiguousarray(tp[1::2]))
    tree, tree_e, tree_p = gpu.KdTreeGPU(tgt), gpu.KdTreeGPU(te), gpu.KdTreeGPU(tpl)
    grads = gpu.estimate_intensity_gradients_gpu(tgt, 10)
    factors, keep = [], [tgt, te, tpl, tree, tree_e, tree_p, grads]
    for kind, n, a in zip(KINDS, SIZES, STARTS):
        src = gpu.PointCloudGPU(sp[a : a + n], sc[a : a + n], intensities=_intensity(sp[a : a + n]))
        keep.append(src)
        if kind == "gicp":
            f = gpu.IntegratedGICPFactorGPU(0, 1, tgt, src)
        elif kind.endswith("-icp"):
            f = gpu.IntegratedICPFactorGPU(0, 1, tgt, src, target_tree=tree, use_point_to_plane=kind == "plane-icp")
        elif kind == "colored":
            f = gpu.IntegratedColoredGICPFactorGPU(0, 1, tgt, src, target_tree=tree, target_gradients=grads)
        elif kind == "edge":
            f = gpu.IntegratedPointToEdgeFactorGPU(0, 1, te, src, target_tree=tree_e)
        else:
            f = gpu.IntegratedLOAMFactorGPU(0, 1, te, tpl, src, src, target_edges_tree=tree_e, target_planes_tree=tree_p)
            if kind == "loam-validated":
                f.set_enable_correspondence_validation(True)
        factors.append(f)
    deltas = np.stack([expmap(XI * s) for s in SCALES])
    general = deltas.copy()
    general[:, :3, :3] = general[:, :3, :3] @ (np.eye(3) + 1e-6 * G)  # orthonormal to 1e-6 only: rigid=False, the 92 explicit sums
    near = deltas @ expmap(NEARBY)
    # the members' own calls, once: rigid record, its error nearby, general record
    single = [f.linearize_delta(d) for f, d in zip(factors, deltas)]
    single_err = np.array([f.error({0: np.eye(4), 1: e}) for f, e in zip(factors, near)])
    single_general = [f.linearize_delta(d) for f, d in zip(factors, general)]
    batch = gpu.CorrespondenceFactorBatchGPU(factors)
    yield dict(factors=factors, keep=keep, deltas=deltas, general=general, near=near, single=single, single_err=single_err, single_general=single_general, batch=batch)
    batch.close()


def test_every_kind_in_one_batch_equals_the_members_own_calls(gpu, scene):
    b = scene["batch"]
    assert b.order == [1, 4, 6, 0, 2, 5, 3, 7] and b._lib.gp_corr_batch_size(b._h) == 8  # GICP, ICP, LOAM, colored: the record order is not the caller's
    for corr_set in (None, 0, 1):  # the synchronous host-pose forms (set 0), the device-pose entry points into either set
        for again in (False, True):  # (a second pass: the same bytes again)
            recs = b.linearize_deltas(scene["deltas"], corr_set=corr_set)
            errs = b.errors(scene["deltas"], scene["near"], corr_set=corr_set)
            if not again:
                for k, (L, S) in enumerate(zip(recs, scene["single"])):
                    print(f"[mixed-batch] set {corr_set} factor {k} ({KINDS[k]}, n={SIZES[k]}): inliers {L.num_inliers} / {S.num_inliers}, error {L.error!r} / {S.error!r}, "
                          f"error nearby {errs[k]!r} / {scene['single_err'][k]!r}")
            for k, (L, S) in enumerate(zip(recs, scene["single"])):
                _same(L, S, f"factor {k} ({KINDS[k]}), set {corr_set}, pass {1 + again}")
            assert errs.tobytes() == scene["single_err"].tobytes(), (corr_set, again)
    assert sum(S.num_inliers for S in scene["single"]) > 2000  # (the comparison is not one of empty records)


def test_every_kind_in_one_batch_on_the_general_path(gpu, scene):
    for corr_set in (None, 0, 1):
        for again in (False, True):
            recs = scene["batch"].linearize_deltas(scene["general"], rigid=False, corr_set=corr_set)
            for k, (L, S) in enumerate(zip(recs, scene["single_general"])):
                _same(L, S, f"factor {k} ({KINDS[k]}), general path, set {corr_set}, pass {1 + again}")
    assert sum(S.num_inliers for S in scene["single_general"]) > 2000

"""Self-check of tests/factor_domain_ref.py, the inputs and f64 statements of the factor-domain sweep (no GPU needed).

For every input of the sweep: the reference is not the weak side (f64 against the same statement in np.longdouble), the face margin removes at most 1 % of the
source, b is not the small remainder of a cancellation (so that a relative figure for it means something), and the margin does not change the inlier count."""
import numpy as np
import pytest

import factor_domain_ref as fd
from helpers import BLOCKS, rel_err

CASES_A = [(t, r) for t in fd.DISTANCES for r in fd.ROTATIONS]


def _sweep_inputs():
    for t, r in CASES_A:
        yield f"a {t:g} m {r}", fd.scan_to_map(t, r)
    yield "b both far", fd.both_far()
    for s in fd.SCALES:
        yield f"c scale {s:g}", fd.scaled(s)


@pytest.fixture(scope="module")
def inputs():
    return list(_sweep_inputs())


def test_scene_shape():
    s = fd.scene()
    assert len(s["target_points"]) == 6000 and len(s["source_points"]) == 4097 == 4096 + 1
    n = np.stack([p[0] / np.linalg.norm(p[0]) for p in fd.PLANES])
    assert np.abs(np.linalg.det(n)) > 0.9  # three planes, mutually far from parallel
    w = np.linalg.eigvalsh(s["source_covs"])
    np.testing.assert_allclose(w, np.broadcast_to([1e-3, 1.0, 1.0], w.shape), atol=1e-12)
    assert abs(np.linalg.norm(fd.DIRECTION) - 1.0) < 1e-12 and (fd.DIRECTION < 0).sum() == 1 and abs(np.linalg.norm(fd.AXIS) - 1.0) < 1e-12
    for t, r in CASES_A:
        W = fd.world_pose(t, r)
        assert np.abs(W[:3, :3].T @ W[:3, :3] - np.eye(3)).max() < 1e-15 and abs(np.linalg.norm(W[:3, 3]) - t) <= 1e-12 * max(t, 1.0)


def test_margin_cap(inputs):
    """the face margin removes at most 1 % of any case's source (and of the target)"""
    for name, (d, delta, _, dropped) in inputs:
        print(f"[domain ref] {name}: {dropped * 100:.4f} % of the source and {d['target_dropped']} target points on a voxel face")
        assert dropped <= fd.DROP_CAP, name
        assert d["target_dropped"] <= fd.DROP_CAP * 6000, name
        assert fd.face_margins(d["source_points"], delta, d["leaf"]).min() > fd.MARGIN


@pytest.mark.parametrize("rotation", list(fd.ROTATIONS))
def test_reference_precision_at_10km(rotation):
    """the f64 reference against np.longdouble on 256 source points, 10 000 m out: 1e-11 norm-wise on every block and on the error"""
    assert np.finfo(np.longdouble).eps < 1e-18, "this platform's long double is no wider than double"
    d, delta, delta_eval, _ = fd.scan_to_map(10000.0, rotation)
    sub = fd.subset_inputs(d, 256)
    for de in (None, delta_eval):
        L, _ = fd.vgicp_reference(sub, delta) if de is None else (fd.onp.vgicp_linearize(_vm(sub), sub["source_points"], sub["source_covs"], delta, de), None)
        X = fd.vgicp_terms(sub, delta, de, dtype=np.longdouble)
        assert L["num_inliers"] == X["num_inliers"] > 150
        worst = max(rel_err(L[k], X[k].astype(np.float64)) for k in BLOCKS)
        # (differences formed in long double: the f64 cast of X alone would hide nothing at 1e-11, but costs nothing to avoid)
        worst = max([worst] + [float(np.linalg.norm(L[k].astype(np.longdouble) - X[k]) / np.linalg.norm(X[k])) for k in BLOCKS])
        e = float(abs(np.longdouble(L["error"]) - X["error"]) / X["error"])
        print(f"[domain ref] 10 km {rotation} eval={'delta' if de is None else 'delta_eval'}: f64 vs long double, worst block {worst:.2e}, error {e:.2e}")
        assert worst <= 1e-11 and e <= 1e-11


def _vm(d):
    vm = fd.onp.VoxelMapNP(d["leaf"])
    vm.insert(d["target_points"], d["target_covs"])
    return vm


def test_f64_restatement_equals_the_oracle(inputs):
    """vgicp_terms in f64 is the oracle's statement (it carries the per-term sums the next test needs)"""
    name, (d, delta, delta_eval, _) = inputs[5]
    L, X = fd.onp.vgicp_linearize(_vm(d), d["source_points"], d["source_covs"], delta, delta_eval), fd.vgicp_terms(d, delta, delta_eval)
    assert L["num_inliers"] == X["num_inliers"]
    assert max(rel_err(X[k], L[k]) for k in BLOCKS) < 1e-10 and abs(X["error"] - L["error"]) < 1e-10 * L["error"]


def test_b_is_not_a_cancellation(inputs):
    """||b|| >= 0.1 * sum_n ||J_n^T M_n r_n|| for b_source and b_target, at the pose the record is taken at and at the evaluation pose"""
    for name, (d, delta, delta_eval, _) in inputs:
        for what, de in (("delta", None), ("delta_eval", delta_eval)):
            X = fd.vgicp_terms(d, delta, de)
            rs, rt = np.linalg.norm(X["b_source"]) / X["term_b_source"], np.linalg.norm(X["b_target"]) / X["term_b_target"]
            print(f"[domain ref] {name} at {what}: ||b_source|| / sum of terms {rs:.3f}, ||b_target|| / sum of terms {rt:.3f}, {X['num_inliers']} inliers")
            assert rs >= 0.1 and rt >= 0.1, (name, what, rs, rt)


def test_margin_keeps_the_inlier_count_at_the_origin():
    for r in fd.ROTATIONS:
        W = fd.world_pose(0.0, r)
        d = fd.place(fd.scene(), W)
        delta = W @ fd.expmap(fd.SMALL)
        filtered, dropped = fd.with_margin(d, delta)
        a, b = fd.vgicp_reference(d, delta)[0]["num_inliers"], fd.vgicp_reference(filtered, delta)[0]["num_inliers"]
        print(f"[domain ref] origin {r}: {a} inliers without the margin filter, {b} with ({dropped * 100:.4f} % removed)")
        assert a == b and a > 2000


def test_icp_inputs_are_conditioned():
    """case (d): no source point on a tie or on the 1 m cut-off of the nearest-neighbour search (what test_icp_gpu.py asks of its inputs)"""
    import icp_ref

    for t in (0.0, 1000.0, 10000.0):
        d, delta, _, _ = fd.scan_to_map(t, "0.4rad")
        ref = icp_ref.ICPFactorRef(d["target_points"], d["source_points"], d["target_normals"], True, 1.0)
        tie, cut = ref.margins(delta)
        L = ref.linearize(delta)
        print(f"[domain ref] icp {t:g} m: tie gap {tie.min():.2e}, cut-off gap {cut.min():.2e}, {L['num_inliers']} inliers")
        assert tie.min() > fd.MARGIN and cut.min() > fd.MARGIN and L["num_inliers"] > 2000

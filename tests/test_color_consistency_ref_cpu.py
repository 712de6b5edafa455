"""CPU checks of tests/color_consistency_ref.py, the restatement the GPU tests of the XYZI search and of IntegratedColorConsistencyFactorGPU compare against.  The
oracle does not compile this factor, so the restatement is held to itself: to finite differences, to the colored GICP restatement at weight 1 (where w_g = 0 and the
Mahalanobis matrix drops out), and -- for the scene -- to the input conditions the GPU tests rest on."""
import numpy as np

import color_consistency_ref as cc
import colored_ref
import icp_ref
from helpers import BLOCKS, expmap, rel_err

XI = cc.XI
MARGIN = 1e-9
POSES = {"identity": np.eye(4), "perturbed": expmap(XI) @ expmap([0.004, -0.003, 0.005, 0.02, -0.03, 0.01])}  # tests/test_colored_gicp_gpu.py's


def _random_inputs(seed, n_target=300, n_source=120):
    rng = np.random.default_rng(seed)
    tp = rng.uniform(-2.0, 2.0, (n_target, 3)).astype(np.float32)
    T = expmap(XI)
    sp = ((tp[:n_source].astype(np.float64) + rng.normal(0.0, 0.02, (n_source, 3)) - T[:3, 3]) @ T[:3, :3]).astype(np.float32)
    normals = rng.normal(size=(n_target, 3))
    normals = (normals / np.linalg.norm(normals, axis=1, keepdims=True)).astype(np.float32)
    return dict(tp=tp, normals=normals, tI=rng.uniform(0, 1, n_target), grads=rng.normal(size=(n_target, 3)), sp=sp, sI=rng.uniform(0, 1, n_source))


def _factor(d, weight, search="3d"):
    return cc.ColorConsistencyFactorRef(d["tp"], d["normals"], d["tI"], d["grads"], d["sp"], d["sI"], max_correspondence_distance=0.5, photometric_term_weight=weight, search=search)


def _general(delta):
    out = delta.copy()
    out[:3, :3] = out[:3, :3] @ (np.eye(3) + 1e-3 * np.random.default_rng(11).normal(size=(3, 3)))
    return out


def test_b_is_half_the_finite_difference_gradient_of_the_error():
    """(a) for a source perturbation delta Expmap(xi) and a target perturbation Expmap(-xi) delta -- the factor's own tangent convention, the one
    tests/test_colored_ref_cpu.py differences the colored restatement in -- b = grad(error) / 2 by central differences with h = 1e-6, at a rigid pose and at one
    whose 3x3 block is not orthonormal; the tolerance is that test's 1e-6"""
    h = 1e-6
    for weight in (1.0, 0.25):
        for delta in (expmap(XI), _general(expmap(XI))):
            ref = _factor(_random_inputs(4), weight)
            L = ref.linearize(delta)
            assert L["num_inliers"] > 60
            moves = dict(source=lambda xi: delta @ expmap(xi), target=lambda xi: expmap(-np.asarray(xi)) @ delta)
            for name, move in moves.items():
                grad = np.array([(ref.error(move(h * e)) - ref.error(move(-h * e))) / (2 * h) for e in np.eye(6)])
                assert rel_err(0.5 * grad, L["b_" + name]) < 1e-6, (weight, name, rel_err(0.5 * grad, L["b_" + name]))
            assert ref.searches == 1  # error() never searches
            for k in ("H_target", "H_source"):
                assert np.allclose(L[k], L[k].T, rtol=1e-13, atol=0.0) and np.linalg.eigvalsh(L[k]).min() >= -1e-9 * np.abs(L[k]).max()


def test_weight_one_is_the_colored_restatement_without_its_geometric_term():
    """(b) on identical correspondences, at photometric_term_weight = 1 (w_g = 0): H, b and the error of the two restatements agree to 1e-12 relative"""
    d = _random_inputs(7)
    rng = np.random.default_rng(8)

    def spd(count):
        A = rng.normal(size=(count, 3, 3))
        return (A @ A.transpose(0, 2, 1) * 0.01 + 1e-3 * np.eye(3)).astype(np.float32)

    for delta in (expmap(XI), _general(expmap(XI))):
        colored = colored_ref.ColoredGICPFactorRef(d["tp"], spd(len(d["tp"])), d["normals"], d["tI"], d["grads"], d["sp"], spd(len(d["sp"])), d["sI"],
                                                   max_correspondence_distance=0.5, photometric_term_weight=1.0)
        Lc = colored.linearize(delta)
        ref = _factor(d, 1.0)
        ref.correspondences = colored.correspondences.copy()  # identical correspondences, whatever either search would say
        L = ref.evaluate(delta)
        assert L["num_inliers"] == Lc["num_inliers"] > 60
        for k in BLOCKS:
            assert rel_err(L[k], Lc[k]) <= 1e-12, (k, rel_err(L[k], Lc[k]))
        assert abs(L["error"] - Lc["error"]) <= 1e-12 * Lc["error"]
        near = delta @ expmap(0.1 * XI)
        assert abs(ref.error(near) - colored.error(near)) <= 1e-12 * colored.error(near)
    # and the weight scales everything linearly, as the reference writes it
    q = _factor(d, 0.25)
    q.correspondences = ref.correspondences.copy()
    Lq = q.evaluate(delta)
    for k in BLOCKS + ["error"]:
        assert rel_err(Lq[k], 0.25 * np.asarray(L[k])) <= 1e-14, k


def test_xyzi_search_reduces_to_the_3d_search_and_honours_the_cut_off():
    rng = np.random.default_rng(3)
    t, q = rng.uniform(-1, 1, (200, 3)), rng.uniform(-1, 1, (50, 3))
    tI, qI = rng.uniform(0, 1, 200), rng.uniform(0, 1, 50)
    i3, d1, _ = icp_ref.nearest_two(t, q)
    i4, d4, _, _ = cc.nearest_xyzi(t, tI, q, qI, scale=0.0)  # the stored side vanishes: d4^2 = d3^2 + I_q^2, the same nearest
    assert np.array_equal(i3, i4) and np.allclose(d4, d1 + qI * qI, rtol=1e-15)
    i4, d4, tie, cut = cc.nearest_xyzi(t, tI, q, qI, scale=1.0, max_sq=0.05)
    brute = ((t[None] - q[:, None]) ** 2).sum(axis=2) + (qI[:, None] - tI[None]) ** 2
    assert np.array_equal(np.where(brute.min(axis=1) < 0.05, brute.argmin(axis=1), -1), i4) and (i4 < 0).any() and (i4 >= 0).any()
    assert (tie > 0).all() and (cut > 0).all()
    # non-finite targets are never returned, non-finite queries get -1; equal distances go to the lowest index
    t2, tI2 = np.vstack([q[:1], t, q[:1]]), np.concatenate([[np.nan], tI, [qI[0]]])
    i, d, _, _ = cc.nearest_xyzi(t2, tI2, q[:1], qI[:1])
    assert i[0] == len(t2) - 1 and d[0] == 0.0
    assert cc.nearest_xyzi(t, tI, np.array([[np.nan, 0, 0], [0, 0, 0]]), np.array([0.5, np.inf]))[0].tolist() == [-1, -1]
    assert cc.nearest_xyzi(np.zeros((3, 3)), np.ones(3), np.zeros((1, 3)), np.ones(1))[0][0] == 0


def test_the_textured_scene_separates_the_4d_from_the_3d_nearest():
    """(c) what the GPU tests need of the scene, at intensity_scale 1, for both of their poses: at least 10 % of the matched source points have a 4-D nearest that is
    not their 3-D nearest; at the 0.3 m cut-off at least one source point has a 3-D nearest inside the cut-off and no 4-D match; no margin is below 1e-9"""
    s = cc.textured_scene()
    t64, tI64, sI64 = s["tp"].astype(np.float64), s["tI"].astype(np.float64), s["sI"].astype(np.float64)
    for name, pose in POSES.items():
        q = icp_ref.transform(pose, s["sp"].astype(np.float64))
        i3, d3, _ = icp_ref.nearest_two(t64, q)
        for cutoff in (1.0, 0.3):
            i4, _, tie, cut = cc.nearest_xyzi(t64, tI64, q, sI64, 1.0, cutoff * cutoff)
            matched = i4 >= 0
            differ = float((i4[matched] != i3[matched]).mean())
            lost = int(((d3 < cutoff * cutoff) & ~matched).sum())
            print(f"[xyzi] {name} cutoff={cutoff}: {int(matched.sum())} matched, {differ:.3f} with another nearest than in 3-D, {lost} inside the cut-off in 3-D only, "
                  f"margins tie {tie.min():.3e} cut-off {cut.min():.3e}")
            assert differ >= 0.10
            assert tie.min() > MARGIN and cut.min() > MARGIN
            if cutoff == 0.3:
                assert lost >= 1

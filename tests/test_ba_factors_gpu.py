"""The BALM plane and edge factors on the device against the longdouble literal restatement (tests/ba_ref.py), everything at ba_ref.GPU_BOUND = 4 x the measured
deviation of the collapsed float64 restatement from the literal longdouble one."""
import numpy as np
import pytest

import ba_ref

pytestmark = pytest.mark.gpu

CASES = ba_ref.single_cases()
KIND_CLASS = {ba_ref.PLANE: "PlaneEVMFactorGPU", ba_ref.EDGE: "EdgeEVMFactorGPU"}


def make_factor(kind, p, pose, scale=1.0):
    import gtsam_points_amd as gpa

    f = getattr(gpa, KIND_CLASS[kind])()
    for x, k in zip(p, pose):
        f.add(x, int(k))
    f.set_scale(scale)
    return f


def dense_of(hf):
    """a HessianFactor's (G, g, f) with the keys in ascending order"""
    order = np.argsort(hf.keys)
    G, g = hf.information(), hf.linear_term()
    idx = np.concatenate([np.arange(6 * i, 6 * i + 6) for i in order])
    return G[np.ix_(idx, idx)], g[idx], hf.f


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_single_factor_against_the_literal_longdouble_form(case):
    kind, p, pose, values, scale, lit, _, scales = ba_ref.reference_single(case)
    f = make_factor(kind, p, pose, scale)
    assert f.num_points() == len(p) and sorted(f.keys()) == sorted(set(int(k) for k in pose)) and f.keys()[0] == int(pose[0])
    hf = f.linearize(values)
    assert hf.keys == f.keys()
    d = ba_ref.deviation(dense_of(hf), lit, scales)
    e = f.error(values)
    de = abs(e - float(lit[2])) / max(abs(float(lit[2])), ba_ref.RESIDUAL_FLOOR * scales[2])
    print(f"{case[0]}: factor {d:.3e}, error {de:.3e}, bound {ba_ref.GPU_BOUND:.3e}")
    assert np.isfinite(d) and d <= ba_ref.GPU_BOUND and de <= ba_ref.GPU_BOUND
    assert e == hf.f  # the error-only kernel is the linearise's first pass


def test_single_pose_feature_far_from_the_origin():
    """all points on one pose 1e3 from the origin: G is what is left of a cancellation of terms ~3e5 and has a measured constant of its own
    (ba_ref.SINGLE_POSE_FAR_DEVIATION, relative to the block's own max-norm like every other); 4 x, as for the common bound"""
    kind, p, pose, values, scale, lit, _, scales = ba_ref.single_pose_far_case()
    d = ba_ref.deviation(dense_of(make_factor(kind, p, pose, scale).linearize(values)), lit, scales)
    print(f"single pose far from the origin: {d:.3e} (bound {4 * ba_ref.SINGLE_POSE_FAR_DEVIATION:.3e})")
    assert d <= 4 * ba_ref.SINGLE_POSE_FAR_DEVIATION


def test_edge_factor_ignores_set_scale():
    case = [c for c in CASES if c[0] == "edge-N65-K3"][0]
    kind, p, pose, values = ba_ref.reference_single(case)[:4]
    a, b = make_factor(kind, p, pose, 1.0).linearize(values), make_factor(kind, p, pose, 7.0).linearize(values)
    assert np.array_equal(a.information(), b.information()) and np.array_equal(a.linear_term(), b.linear_term()) and a.f == b.f


def _batch(cfg):
    import gtsam_points_amd as gpa

    feats, values, lits, _, scales = ba_ref.reference_batch(cfg)
    return gpa.BundleAdjustmentFactorsGPU([make_factor(k, p, pose, sc) for k, p, pose, sc in feats], cfg[1]), feats, values, lits, scales


def _check_system(got, ref, den, what):
    for name, g, r, d in zip("Abc", got, ref, den):
        d = np.asarray(d, dtype=np.float64)
        dev = np.abs(np.asarray(g, dtype=np.longdouble) - r).astype(np.float64)
        ok = d > 0
        worst = float((dev[ok] / d[ok]).max()) if np.any(ok) else 0.0
        print(f"{what} {name}: {worst:.3e} (bound {ba_ref.GPU_BOUND:.3e})")
        assert worst <= ba_ref.GPU_BOUND and np.all(dev[~ok] == 0), (what, name, worst)


@pytest.mark.parametrize("cfg", ba_ref.BATCHES, ids=[f"F{c[0]}-P{c[1]}{'-far' if c[2] else ''}" for c in ba_ref.BATCHES])
def test_batch_through_the_dense_and_sparse_systems(cfg):
    import torch

    import gtsam_points_amd as gpa

    ba, feats, values, lits, scales = _batch(cfg)
    P = cfg[1]
    rec_host = ba.linearize(values)
    rec_dev = ba.linearize_on_device(values)
    assert np.array_equal(rec_host, rec_dev.cpu().numpy()), "host and device-pose linearise differ"
    assert torch.equal(rec_dev, ba.linearize_on_device(values)), "two linearises differ"
    assert len(ba) == len(rec_host) and np.all(np.isfinite(rec_host))
    errs = ba.errors(values)
    ref_err = np.array([float(l[2]) for l in lits])
    den_err = np.array([max(abs(float(l[2])), ba_ref.RESIDUAL_FLOOR * s[2]) for l, s in zip(lits, scales)])
    assert np.all(np.abs(errs - ref_err) <= ba_ref.GPU_BOUND * den_err)
    assert abs(rec_host[:, 1].sum() - errs.sum()) <= 1e-12 * abs(errs.sum()) and rec_host[:, 0].sum() == sum(len(f[1]) for f in feats)
    # every pose a variable; one pose held; the slots in descending pose order (a pair record's target slot above its source slot); a permutation with a held pose
    perm = np.random.default_rng(P).permutation(P - 1).astype(np.int32)
    for held, slot in ((None, np.arange(P, dtype=np.int32)), (0, np.array([-1] + list(range(P - 1)), dtype=np.int32)),
                       ("reversed", np.arange(P, dtype=np.int32)[::-1].copy()), ("permuted", np.concatenate([perm[:1], [-1], perm[1:]]).astype(np.int32))):
        n = int(slot.max()) + 1
        ref = ba_ref.dense_system(feats, lits, slot, n)
        den = ba_ref.dense_denominators(feats, lits, scales, slot, n)
        fs = ba.factor_slots(slot)
        _check_system(gpa.DenseLinearSystemGPU(n, fs).build(rec_dev).download(), ref, den, f"dense held={held}")
        _check_system(gpa.SparseLinearSystemGPU(n, fs).build(rec_dev).download(), ref, den, f"sparse held={held}")
    if cfg[3] is not None:  # the pose no feature sees has no record and an empty row
        A = gpa.DenseLinearSystemGPU(P, ba.factor_slots(np.arange(P, dtype=np.int32))).build(rec_dev).download()[0]
        assert not np.any(A[6 * cfg[3]:6 * cfg[3] + 6]) and cfg[3] not in ba.factor_slots(np.arange(P, dtype=np.int32))[:, 1]


def test_near_degenerate_edge_gives_a_finite_record():
    """lambda_0 and lambda_1 within 1e-6 relative: against the collapsed longdouble form with the cancelling pair omitted (the literal form cancels two terms of
    size 1 / (lambda_0 - lambda_1) there and is no yardstick)"""
    p, pose, values = ba_ref.near_degenerate_edge()
    l = ba_ref.BALMFeature(ba_ref.transform(p, pose, values, np.longdouble)).eigenvalues
    assert 0 < float((l[1] - l[0]) / l[1]) < 1e-6
    ref = ba_ref.collapsed_factor(ba_ref.EDGE, p, pose, values, 1.0, np.longdouble)
    scales = ba_ref.collapsed_factor(ba_ref.EDGE, p, pose, values, 1.0, np.float64, True)[3]
    got = dense_of(make_factor(ba_ref.EDGE, p, pose).linearize(values))
    d = ba_ref.deviation(got, ref, scales)
    print(f"near-degenerate edge: {d:.3e} (bound {ba_ref.GPU_BOUND:.3e})")
    assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[1])) and d <= ba_ref.GPU_BOUND


def test_end_to_end_damped_gauss_newton():
    """8 poses perturbed, pose 0 held; damped Gauss-Newton on device records + SparseLinearSystemGPU.step with T <- Exp(xi) T against the same loop on the
    restatement.  The bound: 4 x the largest deviation of the float64 CPU loop from the longdouble one over the iterates (the record bound propagated through the
    solves, measured), entries of the 4 x 4 values relative to max(1, |t|).  The CPU loops share one Cholesky and differ by a few ulp; the device solves the same
    42 x 42 system in another order (block-sparse, its own elimination order), so the bound has a floor from the solve itself: forward error n eps cond(A + lam I)
    = 42 x 2.2e-16 x 46 (eigenvalues 0.05 + 1 .. 47 + 1) = 4.3e-13 of a step of ~2e-2 per iterate, 4.3e-14 over the five iterates."""
    SOLVE_FLOOR = 5 * 42 * 2.0 ** -52 * 46 * 2e-2
    import gtsam_points_amd as gpa

    P, F, ITER, LAM = 8, 24, 5, 1.0
    rng = np.random.default_rng(77)
    truth = ba_ref.trajectory(P, rng)
    feats = []
    while len(feats) < F:
        kind = ba_ref.PLANE if len(feats) % 3 else ba_ref.EDGE
        pl = sorted(rng.choice(P, size=int(rng.integers(3, 6)), replace=False).tolist())
        p, pose = ba_ref.make_feature(kind, int(rng.integers(12, 30)), pl, truth, rng)
        feats.append((kind, p, pose, 1.0))
    start = ba_ref.perturbed(truth, rng, rot=5e-3, trans=2e-2)
    start[0] = truth[0]
    slot = np.array([-1] + list(range(P - 1)), dtype=np.int32)

    def system(factor, dtype):
        return lambda v: ba_ref.dense_system(feats, [factor(k, p, pose, v, sc, dtype) for k, p, pose, sc in feats], slot, P - 1, dtype)

    ld, ld_cost = ba_ref.gauss_newton(system(ba_ref.literal_factor, np.longdouble), start, slot, ITER, LAM, np.longdouble)
    f64, _ = ba_ref.gauss_newton(system(ba_ref.collapsed_factor, np.float64), start, slot, ITER, LAM, np.float64)
    rel = lambda a, b: float((np.abs(np.asarray(a, dtype=np.longdouble) - b) / np.maximum(1.0, np.abs(np.asarray(b)[:, :3, 3:4].astype(np.float64)).max(1, keepdims=True))).max())  # noqa: E731
    cpu_dev = max(rel(a, b) for a, b in zip(f64, ld))
    ba = gpa.BundleAdjustmentFactorsGPU([make_factor(k, p, pose, sc) for k, p, pose, sc in feats], P)
    sys_ = gpa.SparseLinearSystemGPU(P - 1, ba.factor_slots(slot))
    values, costs = start.copy(), []
    for it in range(ITER):
        x, _, c = sys_.step(ba.linearize_on_device(values), lam=LAM)
        for k in range(P):
            if slot[k] >= 0:
                values[k] = ba_ref.expmap(x[6 * slot[k]:6 * slot[k] + 6]) @ values[k]
        costs.append(c)
        d = rel(values, ld[it])
        print(f"iterate {it}: device vs longdouble {d:.3e}; cost {c:.6e} (longdouble {float(ld_cost[it]):.6e}); bound max(4 x {cpu_dev:.3e}, {SOLVE_FLOOR:.1e})")
        assert d <= max(4 * cpu_dev, SOLVE_FLOOR)
    final = float(ba.errors(values).sum())
    assert final < costs[0], (final, costs[0])

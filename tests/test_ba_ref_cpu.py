"""CPU checks of the bundle-adjustment restatement (tests/ba_ref.py) and of the host side of gp_ba_factors_*: no device."""
import ctypes as C

import numpy as np
import pytest

import ba_ref

LD = np.longdouble


def _small(kind, N=6, K=3, seed=3):
    return ba_ref.build_single(("small", kind, N, K, "sorted", 1.0, 0.0), seed)


@pytest.mark.parametrize("kind", [ba_ref.PLANE, ba_ref.EDGE])
def test_literal_J_and_H_match_central_differences_of_the_eigenvalue(kind):
    """J_i and the 3N x 3N H of the literal form against central differences of lambda_k in the points, longdouble.  Step 1e-5 on points of extent 1: truncation
    ~1e-10 and rounding 2^-64 / 1e-10 ~ 5e-10 of the second difference; held to 1e-6 of the largest entry"""
    _, p, pose, values, _ = _small(kind)
    q = ba_ref.transform(p, pose, values, LD)
    N = len(q)
    feat = ba_ref.BALMFeature(q)
    h = LD(1e-5)
    for k in ((0,) if kind == ba_ref.PLANE else (0, 1)):
        lam = lambda x: ba_ref.BALMFeature(x.reshape(N, 3)).eigenvalues[k]  # noqa: E731
        x0 = q.reshape(-1)
        J, H = np.zeros(3 * N, dtype=LD), np.zeros((3 * N, 3 * N), dtype=LD)
        E = np.eye(3 * N, dtype=LD) * h
        for i in range(3 * N):
            J[i] = (lam(x0 + E[i]) - lam(x0 - E[i])) / (2 * h)
            for j in range(i, 3 * N):
                H[i, j] = H[j, i] = (lam(x0 + E[i] + E[j]) - lam(x0 + E[i] - E[j]) - lam(x0 - E[i] + E[j]) + lam(x0 - E[i] - E[j])) / (4 * h * h)
        Jl, Hl = feat.Ji(k, q).reshape(-1), feat.H(k, q)
        assert float(np.abs(Jl - J).max() / np.abs(J).max()) < 1e-6
        assert float(np.abs(Hl - H).max() / np.abs(H).max()) < 1e-6
        assert float(np.abs(Hl - Hl.T).max()) == 0.0


def test_fixture_features_keep_their_eigenvalues_apart():
    """every fixture feature: pairwise eigenvalue gaps of at least 0.2 of the larger eigenvalue -- what keeps the literal reference itself trustworthy"""
    for c in ba_ref.single_cases():
        kind, p, pose, values, _ = ba_ref.reference_single(c)[:5]
        assert min(ba_ref.eigen_gaps(kind, p, pose, values)) >= 0.2, c[0]
    for cfg in ba_ref.BATCHES:
        feats, values = ba_ref.reference_batch(cfg)[:2]
        for i, (kind, p, pose, _) in enumerate(feats):
            assert min(ba_ref.eigen_gaps(kind, p, pose, values)) >= 0.2, (cfg, i)


def test_collapsed_equals_literal_in_longdouble():
    """the O(N) form is the reference's factor: in longdouble (2^-64 = 5.4e-20) the two agree to 1e-11 over the single cases -- float64 (1.1e-16) reaches 2.6e-9
    there, at the single-pose features whose G is what a cancellation leaves; the same ratio of roundings puts longdouble near 1e-12 -- and to 1e-7 at the single-pose
    feature 1e3 from the origin (float64: 1.07e-5)"""
    r = ba_ref.single_pose_far_case()
    d = ba_ref.deviation(ba_ref.collapsed_factor(*r[:5], LD), r[5], r[7])
    assert d < 1e-7, d
    for c in ba_ref.single_cases():
        kind, p, pose, values, scale, lit, _, scales = ba_ref.reference_single(c)
        d = ba_ref.deviation(ba_ref.collapsed_factor(kind, p, pose, values, scale, LD), lit, scales)
        assert d < 1e-11, (c[0], d)


def test_measured_tolerance():
    """MEASURED_F64_DEVIATION is the largest deviation of the collapsed float64 form from the literal longdouble one over all fixture cases"""
    worst = 0.0
    for c in ba_ref.single_cases():
        _, _, _, _, _, lit, col, scales = ba_ref.reference_single(c)
        worst = max(worst, ba_ref.deviation(col, lit, scales))
    for cfg in ba_ref.BATCHES:
        _, _, lits, cols, scales = ba_ref.reference_batch(cfg)
        worst = max([worst] + [ba_ref.deviation(c, l, s) for c, l, s in zip(cols, lits, scales)])
    print(f"largest float64 deviation {worst:.3e}; constant {ba_ref.MEASURED_F64_DEVIATION:.3e}")
    assert ba_ref.MEASURED_F64_DEVIATION / 4 <= worst <= ba_ref.MEASURED_F64_DEVIATION
    assert ba_ref.GPU_BOUND == 4 * ba_ref.MEASURED_F64_DEVIATION


def test_measured_tolerance_single_pose_far():
    """the constant of the one fixture that the common constant does not cover: all points on one pose 1e3 from the origin"""
    kind, p, pose, values, scale, lit, col, scales = ba_ref.single_pose_far_case()
    assert len(set(pose.tolist())) == 1 and np.linalg.norm(values[0][:3, 3]) > 900 and min(ba_ref.eigen_gaps(kind, p, pose, values)) >= 0.2
    d = ba_ref.deviation(col, lit, scales)
    print(f"single pose far from the origin: float64 deviation {d:.3e}; constant {ba_ref.SINGLE_POSE_FAR_DEVIATION:.3e}")
    assert ba_ref.SINGLE_POSE_FAR_DEVIATION / 4 <= d <= ba_ref.SINGLE_POSE_FAR_DEVIATION


def test_the_floor_governs_only_blocks_that_are_zero_by_construction():
    for c in ba_ref.single_cases():
        kind, p, pose, values, scale, lit, _, scales = ba_ref.reference_single(c)
        K = len(set(pose.tolist()))
        assert scales[3] == ("all" if kind == ba_ref.PLANE and len(p) == 3 else ("g" if K == 1 else "")), c[0]
        dG, dg, df = ba_ref.denominators(lit, scales)
        if scales[3] == "":
            assert df == abs(float(lit[2])) and all(dG[a, b] == float(np.abs(lit[0][6 * a:6 * a + 6, 6 * b:6 * b + 6]).max()) for a in range(K) for b in range(K))
            assert all(dg[a] == float(np.abs(lit[1][6 * a:6 * a + 6]).max()) for a in range(K))
        if scales[3] == "g":  # in exact arithmetic g is zero: what the longdouble form leaves lies far below the floor, G and f keep their own norms
            assert float(np.abs(lit[1]).max()) < 1e-6 * dg[0] and dG[0, 0] == float(np.abs(lit[0]).max()) and df == abs(float(lit[2]))


def test_edge_factor_ignores_the_scale_and_plane_applies_it():
    for kind in (ba_ref.PLANE, ba_ref.EDGE):
        _, p, pose, values, _ = _small(kind)
        G1, g1, f1 = ba_ref.literal_factor(kind, p, pose, values, 1.0)
        G3, g3, f3 = ba_ref.literal_factor(kind, p, pose, values, 3.0)
        k = 3.0 if kind == ba_ref.PLANE else 1.0
        assert np.array_equal(G3, k * G1) and np.array_equal(g3, k * g1) and f3 == k * f1


# ---- the library's host side -------------------------------------------------------------------------------------------------------------------------------------

NEW_SYMBOLS = ["gp_ba_factors_create", "gp_ba_factors_destroy", "gp_ba_factors_num_records", "gp_ba_factors_factor_slots", "gp_ba_factors_linearize",
               "gp_ba_factors_issue_linearize_dev", "gp_ba_factors_compute_errors", "gp_ba_factors_feature_num_poses", "gp_ba_factors_feature_hessian"]


def test_new_names_are_exported():
    import gtsam_points_amd as gpa
    from gtsam_points_amd import _capi

    lib = _capi.load()
    for s in NEW_SYMBOLS:
        assert s in _capi.EXPORTED_SYMBOLS and hasattr(lib, s), s
    for name in ("PlaneEVMFactorGPU", "EdgeEVMFactorGPU", "BundleAdjustmentFactorsGPU"):
        assert name in gpa.__all__ and hasattr(gpa, name), name


def _create(lib, kinds, scales, offsets, pose, points, num_poses, h):
    k, s, o, pp, pt = (np.ascontiguousarray(kinds, np.int32), np.ascontiguousarray(scales, np.float64), np.ascontiguousarray(offsets, np.int32),
                       np.ascontiguousarray(pose, np.int32), np.ascontiguousarray(points, np.float64))
    return lib.gp_ba_factors_create(k.ctypes.data, s.ctypes.data, o.ctypes.data, pp.ctypes.data, pt.ctypes.data, len(k), len(pp), num_poses, None, C.byref(h))


def test_entry_points_refuse_bad_arguments_without_a_device():
    from gtsam_points_amd import _capi

    lib = _capi.load()
    INVALID = 1
    h = C.c_void_p()
    pts = np.arange(18.0).reshape(6, 3)
    good = dict(kinds=[0, 1], scales=[1.0, 1.0], offsets=[0, 3, 6], pose=[0, 1, 2, 0, 0, 1], points=pts, num_poses=3)
    bad = [("fewer than 3 points", dict(offsets=[0, 2, 6])), ("pose index outside", dict(pose=[0, 1, 3, 0, 0, 1])), ("pose index outside", dict(pose=[0, -1, 2, 0, 0, 1])),
           ("unknown kind", dict(kinds=[0, 2])), ("not sorted", dict(offsets=[0, 7, 6])), ("must be 0", dict(offsets=[1, 3, 6])), ("must be num_points", dict(pose=[0, 1, 2, 0, 0, 1, 1], points=np.arange(21.0).reshape(7, 3)))]
    for text, change in bad:
        assert _create(lib, h=h, **{**good, **change}) == INVALID and not h.value, text
        assert b"gp_ba_factors_create" in lib.gp_last_error() and text.encode() in lib.gp_last_error(), lib.gp_last_error()
    fake = C.c_void_p(64)  # never dereferenced: every call below is refused first
    for at in range(5):
        args = [fake, fake, fake, fake, fake, 1, 3, 1, None, C.byref(h)]
        args[at] = None
        assert lib.gp_ba_factors_create(*args) == INVALID and b"null" in lib.gp_last_error()
    assert lib.gp_ba_factors_create(fake, fake, fake, fake, fake, 1, 3, 1, None, None) == INVALID
    assert lib.gp_ba_factors_destroy(None) == 0 and lib.gp_ba_factors_num_records(None) == 0 and lib.gp_ba_factors_feature_num_poses(None, 0) == 0
    assert lib.gp_ba_factors_factor_slots(None, None, None) == INVALID and lib.gp_ba_factors_linearize(None, None, None) == INVALID
    assert lib.gp_ba_factors_issue_linearize_dev(None, None, None) == INVALID and lib.gp_ba_factors_compute_errors(None, None, None) == INVALID
    assert lib.gp_ba_factors_feature_hessian(None, 0, None, None, None, None) == INVALID and b"gp_ba_factors_feature_hessian" in lib.gp_last_error()


def test_records_and_factor_slots_of_a_hand_built_set():
    """three features over five poses: {0, 2}, {2, 3, 0} (keys out of order) and {3}; pose 1 and pose 4 are seen by none.  Unary records for poses 0, 2, 3, then the
    pairs (0, 2), (0, 3), (2, 3)"""
    from gtsam_points_amd import EdgeEVMFactorGPU, PlaneEVMFactorGPU, BundleAdjustmentFactorsGPU

    rng = np.random.default_rng(0)
    fs = [PlaneEVMFactorGPU(), EdgeEVMFactorGPU(), PlaneEVMFactorGPU()]
    for f, keys in zip(fs, ([0, 2, 0, 2], [2, 3, 0, 3, 2], [3, 3, 3])):
        for k in keys:
            f.add(rng.standard_normal(3), k)
    assert fs[1].keys() == [2, 3, 0] and fs[1].num_points() == 5
    ba = BundleAdjustmentFactorsGPU(fs, 5)
    assert len(ba) == 6 and ba._lib.gp_ba_factors_feature_num_poses(ba._h, 1) == 3
    slots = ba.factor_slots([-1, 7, 0, 1, 2])
    assert slots.tolist() == [[-1, -1], [-1, 0], [-1, 1], [-1, 0], [-1, 1], [0, 1]]
    with pytest.raises(ValueError):
        ba.factor_slots([0, 1])

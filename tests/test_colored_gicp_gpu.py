"""GPU tests of estimate_intensity_gradients_gpu (gp_estimate_intensity_gradients*) and IntegratedColoredGICPFactorGPU (gp_colored_gicp_factor_*) against
tests/colored_ref.py, the numpy f64 restatement of factors/intensity_gradients.cpp and impl/integrated_colored_gicp_factor_impl.hpp.

The cloud is colored_ref.two_plane_cloud(): 4,000 jittered points on two intersecting planes with a smooth non-linear intensity field.  Its covariances and normals
come from the device estimators; they are downloaded and given to both sides, as are the device's f32 gradients in the factor tests.  The source is a jittered rigid
copy of 2,500 of the points (colored_ref.moved_copy), every 20th pushed off the surface so that the 0.3 m cut-off drops points the 1 m cut-off keeps.

Gradients.  Both sides are given the SAME neighbour table (gp_knn_search's), so ties cannot separate them.  Every compared point is held to
    |g - g_ref|_inf <= 2^-23 |g_ref|_inf + C cond(H) 2^-52 |g_ref|_inf        (colored_ref.gradient_bound)
the first term being the one rounding to f32 at the store, the second what two f64 evaluations of H^-1 e may differ by.  C = 16 is 4x what the f64 reference differs
from itself when the neighbours are summed in reversed order: measured on the CPU on this cloud at k = 10 and 32, k_photo = k and 6, the largest ratio
|g - g_reversed|_inf / (cond(H) 2^-52 |g|_inf) was 3.88 (k = 32, where cond(H) is about 2 and the 31-term sums set the difference); test_colored_ref_cpu.py repeats
the measurement.  Points with cond(H) > 1e8 may be left out, at most 1 % of a cloud: on this cloud cond(H) stays below 2e4 and none is.

Factor.  Parity at 1e-7, the project's gate for an f64 factor: both sides compute in f64 on the same f32 inputs and differ by the order of 2,500-term sums.  The
device search and the brute-force reference must pick the same target for every source point; every parity test asserts from the reference's margins (> 1e-9
relative) that no point sits on a tie or on the cut-off before it compares."""
import numpy as np
import pytest

import colored_ref
from helpers import BLOCKS, assert_linearized_close, expmap, lm_optimize, pose_error

pytestmark = pytest.mark.gpu
PARITY_TOL = 1e-7
MARGIN = 1e-9
XI = np.array([0.01, -0.02, 0.015, 0.10, -0.05, 0.03])
NEARBY = np.array([0.002, -0.001, 0.003, 0.01, 0.02, -0.01])
G = np.random.default_rng(11).normal(size=(3, 3))
T_GT = expmap(XI)
POSES = {"identity": np.eye(4), "perturbed": T_GT @ expmap([0.004, -0.003, 0.005, 0.02, -0.03, 0.01])}


@pytest.fixture(scope="module")
def scene(gpu):
    """the target on the device with its estimated covariances, normals and gradients, one search structure, and everything the reference needs on the host"""
    tp, tI = colored_ref.two_plane_cloud()
    tgt = gpu.PointCloudGPU(tp, intensities=tI)
    assert gpu.estimate_normals_covariances_gpu(tgt, 10) == 0
    tree = gpu.KdTreeGPU(tgt)
    grads = gpu.estimate_intensity_gradients_gpu(tgt, 10)
    assert grads.num_short == 0
    sp, sI = colored_ref.moved_copy(tp, tI, T_GT)
    src = gpu.PointCloudGPU(sp)
    assert gpu.estimate_covariances_gpu(src, 10) == 0
    return dict(tp=tp, tI=tI, tgt=tgt, tree=tree, grads=grads, tcov=tgt.download("covs"), tnormals=tgt.download("normals"), tgrad=grads.download(), sp=sp, sI=sI,
                scov=src.download("covs"))


# ---- intensity gradients -----------------------------------------------------------------------------------------------------------------------------------------


def _gradient_case(gpu, scene, n, k, k_photo):
    """the first n points of the cloud as a cloud of their own: normals from the device estimator, the table from gp_knn_search, both entry points against the reference"""
    p, I = np.ascontiguousarray(scene["tp"][:n]), np.ascontiguousarray(scene["tI"][:n])
    frame = gpu.PointCloudGPU(p, intensities=I)
    gpu.estimate_normals_gpu(frame, 10)
    normals = frame.download("normals")
    table, _, found = gpu.KdTreeGPU(frame).knn_search(p, k)
    short = int((found < k).sum())
    got = gpu.estimate_intensity_gradients_gpu(frame, neighbors=table, k_photo_neighbors=k_photo).download()
    ref, cond = colored_ref.intensity_gradients(p, normals, I, table, k_photo)
    full = (table[:, :k_photo] >= 0).all(axis=1)
    assert got.shape == (n, 3) and got.dtype == np.float32
    assert not got[~full].any()  # (0, 0, 0) where one of the first k_photo slots is empty
    compared = full & (cond <= colored_ref.COND_CAP)
    assert (full & ~compared).sum() <= 0.01 * n
    if compared.any():
        diff = np.abs(got.astype(np.float64) - ref).max(axis=1)
        bound = colored_ref.gradient_bound(ref, cond)
        worst = int(np.argmax(np.where(compared, diff / np.maximum(bound, 1e-300), 0.0)))
        print(f"[colored] gradients n = {n}, k = {k}, k_photo = {k_photo}: {int(compared.sum())} compared, worst point {worst}: diff {diff[worst]:.3e}, bound "
              f"{bound[worst]:.3e}, cond(H) {colored_ref.grad_H_cond(p, normals, I, table, worst, k_photo):.3g}")
        assert (diff[compared] <= bound[compared]).all(), (worst, diff[worst], bound[worst])
        assert np.isfinite(got[compared]).all() and got[compared].any()
    return frame, table, got, short


@pytest.mark.parametrize("k", [10, 32])
@pytest.mark.parametrize("n", [1, 31, 64, 65, 4000])
def test_gradients_match_reference(gpu, scene, n, k):
    frame, table, got, short = _gradient_case(gpu, scene, n, k, k)
    assert short == (n if n < k else 0)
    # the entry point that searches for itself: the same search, so the same table and the same gradients, and the count of short points
    own = gpu.estimate_intensity_gradients_gpu(frame, k)
    assert own.num_short == short and own.size() == n
    assert np.array_equal(own.download(), got)
    if n < k:
        assert not got.any()


@pytest.mark.parametrize("n,k,k_photo", [(4000, 10, 6), (4000, 32, 10), (65, 10, 4), (31, 32, 20)])
def test_gradients_from_the_first_slots_of_a_longer_table(gpu, scene, n, k, k_photo):
    _, table, got, _ = _gradient_case(gpu, scene, n, k, k_photo)
    if n == 31:  # every list is short at k = 32, but its first 20 slots are full
        assert (table[:, 31] < 0).all() and np.isfinite(got).all() and got.any()


def test_gradients_need_normals_and_intensities(gpu, scene):
    tp, tI = scene["tp"][:100], scene["tI"][:100]
    with pytest.raises(gpu.GPError, match="required attributes for intensity gradient estimation"):
        gpu.estimate_intensity_gradients_gpu(gpu.PointCloudGPU(tp, intensities=tI))
    with pytest.raises(gpu.GPError, match="required attributes for intensity gradient estimation"):
        gpu.estimate_intensity_gradients_gpu(gpu.PointCloudGPU(tp, normals=scene["tnormals"][:100]))
    frame = gpu.PointCloudGPU(tp, normals=scene["tnormals"][:100], intensities=tI)
    with pytest.raises(gpu.GPError, match="gp_estimate_intensity_gradients"):
        gpu.estimate_intensity_gradients_gpu(frame, 33)
    with pytest.raises(gpu.GPError, match="gp_estimate_intensity_gradients_from_neighbors"):
        gpu.estimate_intensity_gradients_gpu(frame, neighbors=np.zeros((100, 4), np.int32), k_photo_neighbors=5)


# ---- the factor -----------------------------------------------------------------------------------------------------------------------------------------------------


def _source(gpu, scene, n):
    return gpu.PointCloudGPU(scene["sp"][:n], covs=scene["scov"][:n], intensities=scene["sI"][:n])


def _factor(gpu, scene, src, cutoff=1.0, weight=0.25, **kw):
    return gpu.IntegratedColoredGICPFactorGPU(0, 1, scene["tgt"], src, target_tree=scene["tree"], target_gradients=scene["grads"], max_correspondence_distance=cutoff,
                                              photometric_term_weight=weight, **kw)


def _reference(scene, n, cutoff=1.0, weight=0.25):
    return colored_ref.ColoredGICPFactorRef(scene["tp"], scene["tcov"], scene["tnormals"], scene["tI"], scene["tgrad"], scene["sp"][:n], scene["scov"][:n], scene["sI"][:n],
                                            max_correspondence_distance=cutoff, photometric_term_weight=weight)


def _conditioned(ref, delta, what):
    tie, cut = ref.margins(delta)
    print(f"[colored] {what}: smallest tie gap {tie.min():.3e}, smallest cut-off gap {cut.min():.3e} (relative, squared distances)")
    assert tie.min() > MARGIN and cut.min() > MARGIN, f"{what}: a correspondence two f64 implementations could decide differently (tie {tie.min():.2e}, cut-off {cut.min():.2e})"


def _check(gpu, scene, n, delta, cutoff, weight, what, src=None):
    """one factor on the device against the reference at `delta`: record, inlier count, error at a nearby pose on the stored correspondences"""
    f = _factor(gpu, scene, src if src is not None else _source(gpu, scene, n), cutoff, weight)
    ref = _reference(scene, n, cutoff, weight)
    _conditioned(ref, delta, what)
    L, Lr = f.linearize_delta(delta), ref.linearize(delta)
    print(f"[colored] {what}: inliers {L.num_inliers} / {Lr['num_inliers']}, error {L.error!r} / {Lr['error']!r}")
    assert_linearized_close(L, Lr, PARITY_TOL, what)
    assert f.num_inliers() == Lr["num_inliers"] == f._lib.gp_colored_gicp_factor_num_correspondences(f._h)
    for k in BLOCKS + ["error"]:
        assert np.isfinite(getattr(L, k)).all(), k
    de = delta @ expmap(NEARBY)
    e, er = f.error({0: np.eye(4), 1: de}), ref.error(de)
    assert ref.searches == 1 and abs(e - er) <= PARITY_TOL * max(er, 1e-300), (e, er)
    return f, L, Lr


@pytest.mark.parametrize("pose", list(POSES))
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1024, 1025, 2500])
def test_linearize_matches_reference(gpu, scene, n, pose):
    src = _source(gpu, scene, n)
    matched = 0
    for cutoff in (1.0, 0.3):
        for weight in (0.0, 0.25, 1.0):
            _, L, _ = _check(gpu, scene, n, POSES[pose], cutoff, weight, f"n={n} {pose} cutoff={cutoff} weight={weight}", src)
            matched += L.num_inliers
    assert matched > 0
    if n == 2500:
        assert _reference(scene, n, 0.3).linearize(POSES[pose])["num_inliers"] < _reference(scene, n, 1.0).linearize(POSES[pose])["num_inliers"]  # the cut-off bites


def test_binary_and_fixed_target_forms(gpu, scene):
    delta = POSES["perturbed"]
    src = _source(gpu, scene, 2500)
    f, L, Lr = _check(gpu, scene, 2500, delta, 1.0, 0.25, "forms", src)
    T_t = expmap([0.03, 0.01, -0.02, 0.5, -0.2, 0.1])
    hf = f.linearize({0: T_t, 1: T_t @ delta})
    assert f.keys() == [0, 1] and hf.keys == [0, 1] and set(hf.G) == {(0, 0), (0, 1), (1, 1)}
    for got, want in [(hf.G[(0, 0)], Lr["H_target"]), (hf.G[(0, 1)], Lr["H_target_source"]), (hf.G[(1, 1)], Lr["H_source"]), (hf.g[0], -Lr["b_target"]), (hf.g[1], -Lr["b_source"])]:
        assert np.linalg.norm(got - want) <= PARITY_TOL * np.linalg.norm(want)  # (delta went through T_t^-1 T_t: 1e-16 on the pose)
    assert abs(hf.f - Lr["error"]) <= PARITY_TOL * Lr["error"]
    # fixed-target form: one key, the source blocks bit for bit (the same kernels in the same order)
    u = _factor(gpu, scene, src, _fixed_target_pose=np.eye(4))
    hu = u.linearize({1: delta})
    assert u.keys() == [1] and hu.keys == [1] and set(hu.G) == {(0, 0)}
    assert np.array_equal(hu.G[(0, 0)], L.H_source) and np.array_equal(hu.g[0], -L.b_source) and hu.f == L.error
    assert u.num_inliers() == Lr["num_inliers"]


def test_non_orthonormal_pose_takes_the_general_path(gpu, scene):
    delta = POSES["perturbed"].copy()
    delta[:3, :3] = delta[:3, :3] @ (np.eye(3) + 1e-6 * G)  # orthonormal to 1e-6 only
    assert np.abs(delta[:3, :3].T @ delta[:3, :3] - np.eye(3)).max() > 1e-7
    src = _source(gpu, scene, 2500)
    for weight in (0.0, 0.25, 1.0):
        _check(gpu, scene, 2500, delta, 1.0, weight, f"non-orthonormal weight={weight}", src)


def test_weight_zero_is_the_gicp_factor(gpu, scene):
    src = _source(gpu, scene, 2500)
    tgt = scene["tgt"]
    for cutoff in (1.0, 0.3):
        for delta in POSES.values():
            _conditioned(_reference(scene, 2500, cutoff), delta, f"gicp cutoff={cutoff}")
            L = _factor(gpu, scene, src, cutoff, 0.0).linearize_delta(delta)
            Lg = gpu.IntegratedGICPFactorGPU(0, 1, tgt, src, max_correspondence_distance=cutoff).linearize_delta(delta)
            assert L.num_inliers > 1000
            assert_linearized_close(L, Lg, PARITY_TOL, f"weight 0 against GICP, cutoff={cutoff}")


def test_every_point_beyond_the_cut_off(gpu, scene):
    far = expmap([0.0, 0.0, 0.0, 0.0, 0.0, 500.0])
    f, L, Lr = _check(gpu, scene, 1025, far, 1.0, 0.25, "all beyond")
    assert Lr["num_inliers"] == 0 and L.num_inliers == 0 and L.error == 0.0
    for k in BLOCKS:
        assert not np.any(getattr(L, k)), k
    assert f.error({0: np.eye(4), 1: far}) == 0.0


def test_two_linearises_are_bit_identical(gpu, scene):
    src = _source(gpu, scene, 2500)
    for delta in (POSES["perturbed"], POSES["perturbed"] @ np.diag([1.0 + 1e-6, 1.0, 1.0, 1.0])):  # the rigid and the general kernels
        f = _factor(gpu, scene, src)
        A, B = f.linearize_delta(delta), f.linearize_delta(delta)
        Cc = _factor(gpu, scene, src).linearize_delta(delta)
        for k in BLOCKS + ["error", "num_inliers"]:
            assert np.array_equal(getattr(A, k), getattr(B, k)) and np.array_equal(getattr(A, k), getattr(Cc, k)), k
        assert A.num_inliers > 2000


def test_setters(gpu, scene):
    """the weight and the cut-off set on a live factor give the record of a factor created with them"""
    src = _source(gpu, scene, 2500)
    delta = POSES["perturbed"]
    f = _factor(gpu, scene, src, 1.0, 0.25)
    f.linearize_delta(delta)
    f.set_photometric_term_weight(0.6)
    f.set_max_correspondence_distance(0.3)
    A, B = f.linearize_delta(delta), _factor(gpu, scene, src, 0.3, 0.6).linearize_delta(delta)
    for k in BLOCKS + ["error", "num_inliers"]:
        assert np.array_equal(getattr(A, k), getattr(B, k)), k
    assert_linearized_close(A, _reference(scene, 2500, 0.3, 0.6).linearize(delta), PARITY_TOL, "after the setters")
    for bad in (-0.1, 1.1):
        with pytest.raises(gpu.GPError, match="weight outside"):
            f.set_photometric_term_weight(bad)
    with pytest.raises(gpu.GPError, match="must be positive"):
        f.set_max_correspondence_distance(0.0)


def test_correspondence_update_tolerance(gpu, scene):
    d1 = POSES["perturbed"]
    d2 = d1 @ expmap([0.01, 0.0, -0.01, 0.05, 0.0, 0.02])  # 0.014 rad / 0.054 m from d1: inside (0.05 rad, 0.5 m)
    d3 = d1 @ expmap([0.06, 0.0, 0.0, 0.0, 0.0, 0.0])       # 0.06 rad from d1: outside
    src = _source(gpu, scene, 2500)
    f, ref = _factor(gpu, scene, src, 0.3), _reference(scene, 2500, 0.3)
    for h in (f, ref):
        h.set_correspondence_update_tolerance(0.05, 0.5)
    for d in (d1, d2, d3):
        _conditioned(_reference(scene, 2500, 0.3), d, "tolerance poses")
    assert_linearized_close(f.linearize_delta(d1), ref.linearize(d1), PARITY_TOL, "first linearise")
    L2, R2 = f.linearize_delta(d2), ref.linearize(d2)
    assert ref.searches == 1  # kept
    assert_linearized_close(L2, R2, PARITY_TOL, "inside the tolerance: the correspondences of the first pose, M_g at the second")
    fresh = _reference(scene, 2500, 0.3).linearize(d2)
    assert abs(fresh["error"] - R2["error"]) > 1e3 * PARITY_TOL * fresh["error"]  # the fixture tells the two apart
    de = d2 @ expmap(NEARBY)  # error() after a linearise that kept the correspondences still evaluates on them
    assert abs(f.error({0: np.eye(4), 1: de}) - ref.error(de)) <= PARITY_TOL * ref.error(de)
    L3, R3 = f.linearize_delta(d3), ref.linearize(d3)
    assert ref.searches == 2  # searched again
    assert_linearized_close(L3, R3, PARITY_TOL, "outside the tolerance")
    # only one tolerance set: the other's strict '<' fails, the search runs; zero tolerances (the default): every linearise is a fresh search
    for angle in (0.05, 0.0):
        g = _factor(gpu, scene, src, 0.3)
        g.set_correspondence_update_tolerance(angle, 0.0)
        g.linearize_delta(d1)
        assert_linearized_close(g.linearize_delta(d2), fresh, PARITY_TOL, f"tolerances ({angle}, 0)")


def test_defaults_and_missing_attributes(gpu, scene):
    tp, tI, sp, sI = scene["tp"], scene["tI"], scene["sp"], scene["sI"]
    src = _source(gpu, scene, 2500)
    # target_tree=None builds a tree, target_gradients=None estimates the gradients with k = 10: the record of the factor given both
    f = gpu.IntegratedColoredGICPFactorGPU(0, 1, scene["tgt"], src)
    assert isinstance(f.target_tree, gpu.KdTreeGPU) and np.array_equal(f.target_gradients.download(), scene["tgrad"])
    A, B = f.linearize_delta(POSES["perturbed"]), _factor(gpu, scene, src).linearize_delta(POSES["perturbed"])
    for k in BLOCKS + ["error", "num_inliers"]:
        assert np.array_equal(getattr(A, k), getattr(B, k)), k
    full = dict(covs=scene["tcov"], normals=scene["tnormals"], intensities=tI)
    for missing in full:
        with pytest.raises(gpu.GPError, match="error: target frame doesn't have required attributes for colored_gicp"):
            gpu.IntegratedColoredGICPFactorGPU(0, 1, gpu.PointCloudGPU(tp, **{k: v for k, v in full.items() if k != missing}), src)
    for kw in (dict(covs=scene["scov"]), dict(intensities=sI)):
        with pytest.raises(gpu.GPError, match="error: source frame doesn't have required attributes for colored_gicp"):
            gpu.IntegratedColoredGICPFactorGPU(0, 1, scene["tgt"], gpu.PointCloudGPU(sp, **kw))
    with pytest.raises(gpu.GPError, match="photometric_term_weight outside"):
        _factor(gpu, scene, src, 1.0, 1.5)


def test_aligns_the_moved_copy_as_tightly_as_the_reference(gpu, scene):
    """End to end: a fixed-target factor driven by helpers.lm_optimize from T_gt Expmap(xi_0), and the f64 reference driven by the same loop from the same start.
    The source's 1 cm jitter sets how far from T_gt the minimum lies (the same for both); the device may end 10 % further than the reference, for summation
    order only."""
    T0 = T_GT @ expmap([0.02, -0.015, 0.02, 0.1, -0.05, 0.05])
    f = _factor(gpu, scene, _source(gpu, scene, 2500), _fixed_target_pose=np.eye(4))
    v = lm_optimize(lambda values: [f.linearize(values)], lambda values: f.error(values), {1: T0}, [1])
    ref = _reference(scene, 2500)

    def ref_linearize(values):
        L = ref.linearize(values[1])
        return [gpu.HessianFactor([1], {(0, 0): L["H_source"]}, [-L["b_source"]], L["error"])]

    vr = lm_optimize(ref_linearize, lambda values: ref.error(values[1]), {1: T0}, [1])
    (ang, trans), (ang_r, trans_r) = pose_error(v[1], T_GT), pose_error(vr[1], T_GT)
    print(f"[colored] end to end: device {ang:.3e} rad, {trans:.3e} m from the truth ({f.num_inliers()} inliers); reference {ang_r:.3e} rad, {trans_r:.3e} m "
          f"({ref.searches} linearisations)")
    assert ang_r < 0.005 and trans_r < 0.01  # the loop converges at all
    assert ang <= 1.1 * ang_r and trans <= 1.1 * trans_r

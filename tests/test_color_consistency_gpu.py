"""GPU tests of IntegratedColorConsistencyFactorGPU (gp_color_consistency_factor_*) and of the photometric factors on XYZI correspondences (IntensityKdTreeGPU as
target_tree) against tests/color_consistency_ref.py, the numpy f64 restatement of impl/integrated_color_consistency_factor_impl.hpp.

Scene, margins and poses are those of tests/test_colored_gicp_gpu.py: colored_ref.two_plane_cloud() with device-estimated normals, covariances and gradients (downloaded
and given to both sides), colored_ref.moved_copy as the source, the poses "identity" and "perturbed".  A second scene, color_consistency_ref.textured_scene(), has
the same geometry under an intensity field with texture at the scale of the point spacing: there the 4-D nearest differs from the 3-D nearest for a large share of
the points (tests/test_color_consistency_ref_cpu.py), so a factor that searched in 3-D when handed an IntensityKdTreeGPU fails.

Parity at PARITY_TOL = 1e-7, the project's gate for an f64 factor, through helpers.assert_linearized_close; every parity test first asserts from the reference's
margins (> 1e-9 relative) that no source point sits on a tie or on the cut-off."""
import numpy as np
import pytest

import color_consistency_ref as cc
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


def _scene(gpu, tp, tI, sp, sI):
    tgt = gpu.PointCloudGPU(tp, intensities=tI)
    assert gpu.estimate_normals_covariances_gpu(tgt, 10) == 0
    grads = gpu.estimate_intensity_gradients_gpu(tgt, 10)
    assert grads.num_short == 0
    src = gpu.PointCloudGPU(sp)
    assert gpu.estimate_covariances_gpu(src, 10) == 0
    return dict(tp=tp, tI=tI, tgt=tgt, grads=grads, tcov=tgt.download("covs"), tnormals=tgt.download("normals"), tgrad=grads.download(), sp=sp, sI=sI,
                scov=src.download("covs"), trees={"3d": gpu.KdTreeGPU(tgt), "xyzi": gpu.IntensityKdTreeGPU(tgt)})


@pytest.fixture(scope="module")
def scene(gpu):
    tp, tI = colored_ref.two_plane_cloud()
    sp, sI = colored_ref.moved_copy(tp, tI, T_GT)
    return _scene(gpu, tp, tI, sp, sI)


@pytest.fixture(scope="module")
def textured(gpu):
    s = cc.textured_scene()
    return _scene(gpu, s["tp"], s["tI"], s["sp"], s["sI"])


def _source(gpu, s, n, covs=False):
    return gpu.PointCloudGPU(s["sp"][:n], intensities=s["sI"][:n], **(dict(covs=s["scov"][:n]) if covs else {}))


def _factor(gpu, s, src, search="3d", cutoff=1.0, weight=1.0, **kw):
    return gpu.IntegratedColorConsistencyFactorGPU(0, 1, s["tgt"], src, target_tree=s["trees"][search], target_gradients=s["grads"], max_correspondence_distance=cutoff,
                                                   photometric_term_weight=weight, **kw)


def _reference(s, n, search="3d", cutoff=1.0, weight=1.0):
    return cc.ColorConsistencyFactorRef(s["tp"], s["tnormals"], s["tI"], s["tgrad"], s["sp"][:n], s["sI"][:n], max_correspondence_distance=cutoff,
                                        photometric_term_weight=weight, search="3d" if search == "3d" else ("xyzi", 1.0))


def _conditioned(ref, delta, what):
    tie, cut = ref.margins(delta)
    if len(tie):
        print(f"[color] {what}: smallest tie gap {tie.min():.3e}, smallest cut-off gap {cut.min():.3e} (relative, squared distances)")
        assert tie.min() > MARGIN and cut.min() > MARGIN, f"{what}: a correspondence two f64 implementations could decide differently"


def _check(gpu, s, n, delta, search, cutoff, weight, what, src=None, **kw):
    """one factor on the device against the reference at `delta`: record, inlier count, error at a nearby pose on the stored correspondences"""
    f = _factor(gpu, s, src if src is not None else _source(gpu, s, n), search, cutoff, weight, **kw)
    ref = _reference(s, n, search, cutoff, weight)
    _conditioned(ref, delta, what)
    L, Lr = f.linearize_delta(delta), ref.linearize(delta)
    print(f"[color] {what}: inliers {L.num_inliers} / {Lr['num_inliers']}, error {L.error!r} / {Lr['error']!r}")
    assert_linearized_close(L, Lr, PARITY_TOL, what)
    assert f.num_inliers() == Lr["num_inliers"] == f._lib.gp_color_consistency_factor_num_correspondences(f._h)
    for k in BLOCKS + ["error"]:
        assert np.isfinite(getattr(L, k)).all(), k
    de = delta @ expmap(NEARBY)
    e, er = f.error({0: np.eye(4), 1: de}), ref.error(de)
    assert ref.searches == 1 and abs(e - er) <= PARITY_TOL * max(er, 1e-300), (e, er)
    return f, L, Lr


@pytest.mark.parametrize("search", ["3d", "xyzi"])
@pytest.mark.parametrize("pose", list(POSES))
@pytest.mark.parametrize("n", [0, 1, 64, 65, 1024, 1025, 2500])
def test_linearize_matches_reference(gpu, scene, textured, n, pose, search):
    """both searches on the colored test's scene and on the textured one, both cut-offs (0.3 m drops points 1 m keeps), both weights"""
    for s, name in ((scene, "smooth"), (textured, "textured")):
        src = _source(gpu, s, n)
        for cutoff in (1.0, 0.3):
            for weight in (1.0, 0.25):
                _, L, _ = _check(gpu, s, n, POSES[pose], search, cutoff, weight, f"{name} n={n} {pose} {search} cutoff={cutoff} weight={weight}", src)
                if n == 0:
                    assert L.num_inliers == 0 and L.error == 0.0 and not any(np.any(getattr(L, k)) for k in BLOCKS)
        if n == 2500:
            few, many = (_reference(s, n, search, c).linearize(POSES[pose])["num_inliers"] for c in (0.3, 1.0))
            assert 0 < few < many  # the cut-off bites


def test_xyzi_correspondences_differ_from_the_3d_ones(gpu, textured):
    """the fixture tells the two searches apart: on the textured scene the two references disagree far beyond the gate, and each device factor sides with its own"""
    src = _source(gpu, textured, 2500)
    for pose in POSES.values():
        r3, r4 = (_reference(textured, 2500, k, 0.3).linearize(pose) for k in ("3d", "xyzi"))
        assert abs(r3["error"] - r4["error"]) > 1e3 * PARITY_TOL * r4["error"] and r4["num_inliers"] < r3["num_inliers"]
        assert_linearized_close(_factor(gpu, textured, src, "xyzi", 0.3).linearize_delta(pose), r4, PARITY_TOL, "xyzi")
        assert_linearized_close(_factor(gpu, textured, src, "3d", 0.3).linearize_delta(pose), r3, PARITY_TOL, "3d")


@pytest.mark.parametrize("search", ["3d", "xyzi"])
def test_binary_and_fixed_target_forms(gpu, textured, search):
    delta = POSES["perturbed"]
    src = _source(gpu, textured, 2500)
    f, L, Lr = _check(gpu, textured, 2500, delta, search, 1.0, 1.0, f"forms {search}", src)
    T_t = expmap([0.03, 0.01, -0.02, 0.5, -0.2, 0.1])
    hf = f.linearize({0: T_t, 1: T_t @ delta})
    assert f.keys() == [0, 1] and hf.keys == [0, 1] and set(hf.G) == {(0, 0), (0, 1), (1, 1)}
    for got, want in [(hf.G[(0, 0)], Lr["H_target"]), (hf.G[(0, 1)], Lr["H_target_source"]), (hf.G[(1, 1)], Lr["H_source"]), (hf.g[0], -Lr["b_target"]), (hf.g[1], -Lr["b_source"])]:
        assert np.linalg.norm(got - want) <= PARITY_TOL * np.linalg.norm(want)
    assert abs(hf.f - Lr["error"]) <= PARITY_TOL * Lr["error"]
    # fixed-target form: one key, the source blocks bit for bit (the same kernels in the same order)
    u = _factor(gpu, textured, src, search, _fixed_target_pose=np.eye(4))
    hu = u.linearize({1: delta})
    assert u.keys() == [1] and hu.keys == [1] and set(hu.G) == {(0, 0)}
    assert np.array_equal(hu.G[(0, 0)], L.H_source) and np.array_equal(hu.g[0], -L.b_source) and hu.f == L.error
    assert u.num_inliers() == Lr["num_inliers"]
    ref = _reference(textured, 2500, search)
    ref.linearize(delta)  # error() at a second pose evaluates on the correspondences stored at delta, on both sides
    er = ref.error(delta @ expmap(NEARBY))
    assert abs(u.error({1: delta @ expmap(NEARBY)}) - er) <= PARITY_TOL * er


@pytest.mark.parametrize("search", ["3d", "xyzi"])
def test_non_orthonormal_pose_takes_the_general_path(gpu, textured, search):
    delta = POSES["perturbed"].copy()
    delta[:3, :3] = delta[:3, :3] @ (np.eye(3) + 1e-6 * G)  # orthonormal to 1e-6 only
    assert np.abs(delta[:3, :3].T @ delta[:3, :3] - np.eye(3)).max() > 1e-7
    src = _source(gpu, textured, 2500)
    for weight in (1.0, 0.25):
        _check(gpu, textured, 2500, delta, search, 1.0, weight, f"non-orthonormal {search} weight={weight}", src)


@pytest.mark.parametrize("search", ["3d", "xyzi"])
def test_stored_correspondences_and_update_tolerance(gpu, textured, search):
    d1 = POSES["perturbed"]
    d2 = d1 @ expmap([0.01, 0.0, -0.01, 0.05, 0.0, 0.02])  # 0.014 rad / 0.054 m from d1: inside (0.05 rad, 0.5 m)
    d3 = d1 @ expmap([0.06, 0.0, 0.0, 0.0, 0.0, 0.0])       # 0.06 rad from d1: outside
    src = _source(gpu, textured, 2500)
    f, ref = _factor(gpu, textured, src, search, 0.3), _reference(textured, 2500, search, 0.3)
    for h in (f, ref):
        h.set_correspondence_update_tolerance(0.05, 0.5)
    for d in (d1, d2, d3):
        _conditioned(_reference(textured, 2500, search, 0.3), d, "tolerance poses")
    assert_linearized_close(f.linearize_delta(d1), ref.linearize(d1), PARITY_TOL, "first linearise")
    L2, R2 = f.linearize_delta(d2), ref.linearize(d2)
    assert ref.searches == 1  # kept
    assert_linearized_close(L2, R2, PARITY_TOL, "inside the tolerance: the correspondences of the first pose")
    fresh = _reference(textured, 2500, search, 0.3).linearize(d2)
    assert abs(fresh["error"] - R2["error"]) > 1e3 * PARITY_TOL * fresh["error"]  # the fixture tells the two apart
    de = d2 @ expmap(NEARBY)  # error() at a second pose evaluates on the stored correspondences
    assert abs(f.error({0: np.eye(4), 1: de}) - ref.error(de)) <= PARITY_TOL * ref.error(de)
    L3, R3 = f.linearize_delta(d3), ref.linearize(d3)
    assert ref.searches == 2  # searched again
    assert_linearized_close(L3, R3, PARITY_TOL, "outside the tolerance")
    g = _factor(gpu, textured, src, search, 0.3)  # zero tolerances (the default): every linearise is a fresh search
    g.linearize_delta(d1)
    assert_linearized_close(g.linearize_delta(d2), fresh, PARITY_TOL, "zero tolerances")


def test_every_point_beyond_the_cut_off(gpu, scene):
    far = expmap([0.0, 0.0, 0.0, 0.0, 0.0, 500.0])
    for search in ("3d", "xyzi"):
        f, L, Lr = _check(gpu, scene, 1025, far, search, 1.0, 1.0, f"all beyond {search}")
        assert Lr["num_inliers"] == 0 and L.num_inliers == 0 and L.error == 0.0
        assert not any(np.any(getattr(L, k)) for k in BLOCKS)
        assert f.error({0: np.eye(4), 1: far}) == 0.0


def test_two_linearises_are_bit_identical(gpu, textured):
    src = _source(gpu, textured, 2500)
    for search in ("3d", "xyzi"):
        for delta in (POSES["perturbed"], POSES["perturbed"] @ np.diag([1.0 + 1e-6, 1.0, 1.0, 1.0])):  # the rigid and the general kernels
            f = _factor(gpu, textured, src, search)
            A, B = f.linearize_delta(delta), f.linearize_delta(delta)
            Cc = _factor(gpu, textured, src, search).linearize_delta(delta)
            for k in BLOCKS + ["error", "num_inliers"]:
                assert np.array_equal(getattr(A, k), getattr(B, k)) and np.array_equal(getattr(A, k), getattr(Cc, k)), k
            assert A.num_inliers > 2000


def test_setters(gpu, scene):
    src = _source(gpu, scene, 2500)
    delta = POSES["perturbed"]
    f = _factor(gpu, scene, src, "3d", 1.0, 1.0)
    f.linearize_delta(delta)
    f.set_photometric_term_weight(0.25)
    f.set_max_correspondence_distance(0.3)
    A, B = f.linearize_delta(delta), _factor(gpu, scene, src, "3d", 0.3, 0.25).linearize_delta(delta)
    for k in BLOCKS + ["error", "num_inliers"]:
        assert np.array_equal(getattr(A, k), getattr(B, k)), k
    assert_linearized_close(A, _reference(scene, 2500, "3d", 0.3, 0.25).linearize(delta), PARITY_TOL, "after the setters")
    with pytest.raises(gpu.GPError, match="weight negative"):
        f.set_photometric_term_weight(-0.1)
    with pytest.raises(gpu.GPError, match="must be positive"):
        f.set_max_correspondence_distance(0.0)


def test_agrees_with_the_colored_factor_at_weight_one(gpu, scene, textured):
    """the device cross-check: on the same tree IntegratedColoredGICPFactorGPU(photometric_term_weight=1.0) -- w_g = 0 -- and the new factor agree"""
    for s in (scene, textured):
        src = _source(gpu, s, 2500, covs=True)
        for search in ("3d", "xyzi"):
            for delta in POSES.values():
                c = gpu.IntegratedColoredGICPFactorGPU(0, 1, s["tgt"], src, target_tree=s["trees"][search], target_gradients=s["grads"], photometric_term_weight=1.0)
                Lc, L = c.linearize_delta(delta), _factor(gpu, s, src, search).linearize_delta(delta)
                assert L.num_inliers == Lc.num_inliers > 2000
                assert_linearized_close(L, Lc, PARITY_TOL, f"against the colored factor, {search}")


def test_colored_gicp_on_xyzi_correspondences(gpu, textured):
    """IntegratedColoredGICPFactorGPU(target_tree=IntensityKdTreeGPU) searches in 4-D (integrated_colored_gicp_factor_impl.hpp:121-127): its restatement on XYZI
    correspondences, which on this scene is far from the one on 3-D correspondences"""
    s = textured
    src = _source(gpu, s, 2500, covs=True)
    for cutoff in (1.0, 0.3):
        for name, delta in POSES.items():
            args = (s["tp"], s["tcov"], s["tnormals"], s["tI"], s["tgrad"], s["sp"], s["scov"], s["sI"])
            ref = cc.ColoredGICPXyziRef(*args, max_correspondence_distance=cutoff, photometric_term_weight=0.25)
            _conditioned(ref, delta, f"colored xyzi {name} cutoff={cutoff}")
            f = gpu.IntegratedColoredGICPFactorGPU(0, 1, s["tgt"], src, target_tree=s["trees"]["xyzi"], target_gradients=s["grads"], max_correspondence_distance=cutoff)
            L, Lr = f.linearize_delta(delta), ref.linearize(delta)
            assert_linearized_close(L, Lr, PARITY_TOL, f"colored GICP on XYZI correspondences, {name} cutoff={cutoff}")
            L3 = colored_ref.ColoredGICPFactorRef(*args, max_correspondence_distance=cutoff, photometric_term_weight=0.25).linearize(delta)
            assert abs(L3["error"] - Lr["error"]) > 1e3 * PARITY_TOL * Lr["error"]  # a 3-D search would not pass
            de = delta @ expmap(NEARBY)
            assert abs(f.error({0: np.eye(4), 1: de}) - ref.error(de)) <= PARITY_TOL * ref.error(de)


def test_defaults_and_missing_attributes(gpu, scene):
    tp, tI, sp, sI = scene["tp"], scene["tI"], scene["sp"], scene["sI"]
    src = _source(gpu, scene, 2500)
    # target_tree=None builds a KdTreeGPU, target_gradients=None estimates the gradients with k = 10, the weight defaults to 1.0: the record of the factor given all three
    f = gpu.IntegratedColorConsistencyFactorGPU(0, 1, scene["tgt"], src)
    assert isinstance(f.target_tree, gpu.KdTreeGPU) and np.array_equal(f.target_gradients.download(), scene["tgrad"])
    A, B = f.linearize_delta(POSES["perturbed"]), _factor(gpu, scene, src).linearize_delta(POSES["perturbed"])
    for k in BLOCKS + ["error", "num_inliers"]:
        assert np.array_equal(getattr(A, k), getattr(B, k)), k
    full = dict(normals=scene["tnormals"], intensities=tI)
    for missing in full:  # (the reference's texts say colored_gicp in this factor too)
        with pytest.raises(gpu.GPError, match="error: target frame doesn't have required attributes for colored_gicp"):
            gpu.IntegratedColorConsistencyFactorGPU(0, 1, gpu.PointCloudGPU(tp, **{k: v for k, v in full.items() if k != missing}), src)
    with pytest.raises(gpu.GPError, match="error: source frame doesn't have required attributes for colored_gicp"):
        gpu.IntegratedColorConsistencyFactorGPU(0, 1, scene["tgt"], gpu.PointCloudGPU(sp))
    with pytest.raises(gpu.GPError, match="photometric_term_weight negative"):
        _factor(gpu, scene, src, weight=-1.0)
    # a tree over another frame's points, or over this frame's points with other intensities, is refused
    other = gpu.PointCloudGPU(tp, normals=scene["tnormals"], intensities=tI)
    with pytest.raises(gpu.GPError, match="was not built over the target frame's points"):
        gpu.IntegratedColorConsistencyFactorGPU(0, 1, other, src, target_tree=scene["trees"]["xyzi"])
    with pytest.raises(TypeError):
        gpu.IntegratedColorConsistencyFactorGPU(0, 1, scene["tgt"], src, target_tree=object())


def test_batch_and_lm_graph_refuse_the_new_configurations(gpu, scene):
    src = _source(gpu, scene, 1025, covs=True)
    consistency = _factor(gpu, scene, src)
    colored_xyzi = gpu.IntegratedColoredGICPFactorGPU(0, 1, scene["tgt"], src, target_tree=scene["trees"]["xyzi"], target_gradients=scene["grads"])
    colored_3d = gpu.IntegratedColoredGICPFactorGPU(0, 1, scene["tgt"], src, target_tree=scene["trees"]["3d"], target_gradients=scene["grads"])
    for bad, text in ((consistency, "IntegratedColorConsistencyFactorGPU cannot join"), (colored_xyzi, "XYZI search")):
        with pytest.raises(gpu.GPError, match=text):
            gpu.CorrespondenceFactorBatchGPU([colored_3d, bad])
        with pytest.raises(gpu.GPError, match=text):
            gpu.LevenbergMarquardtGraphGPU([], [], 2, fixed=(0,), corr_factors=[bad], corr_pairs=[(0, 1)])
    # the library refuses it too, whoever asks
    import ctypes as C

    h = C.c_void_p()
    ca = (C.c_void_p * 1)(colored_xyzi._h.value)
    none = (C.c_void_p * 1)()
    assert colored_xyzi._lib.gp_corr_batch_create_ex2(none, 0, none, 0, none, 0, ca, 1, None, C.byref(h)) == 1 and not h.value
    assert b"XYZI" in colored_xyzi._lib.gp_last_error()
    gpu.CorrespondenceFactorBatchGPU([colored_3d]).close()  # (the 3-D colored factor still joins)


def test_icp_plus_color_consistency_moves_towards_the_truth(gpu, scene):
    """Use: point-to-plane ICP plus the color consistency factor through helpers.lm_optimize from the "perturbed" start ends nearer T_GT than it began, and the device
    factor's error at the final pose is the restatement's there"""
    src = _source(gpu, scene, 2500)
    T0 = POSES["perturbed"]
    icp = gpu.IntegratedPointToPlaneICPFactorGPU(0, 1, scene["tgt"], src, target_tree=scene["trees"]["3d"], _fixed_target_pose=np.eye(4))
    f = _factor(gpu, scene, src, "xyzi", _fixed_target_pose=np.eye(4))
    v = lm_optimize(lambda values: [icp.linearize(values), f.linearize(values)], lambda values: icp.error(values) + f.error(values), {1: T0}, [1])
    (a0, t0), (a1, t1) = pose_error(T0, T_GT), pose_error(v[1], T_GT)
    print(f"[color] ICP + color consistency: from {a0:.3e} rad, {t0:.3e} m to {a1:.3e} rad, {t1:.3e} m off the truth")
    assert a1 < a0 and t1 < t0
    ref = _reference(scene, 2500, "xyzi")
    _conditioned(ref, v[1], "final pose")
    g = _factor(gpu, scene, src, "xyzi", _fixed_target_pose=np.eye(4))
    e, er = g.error({1: v[1]}), ref.error(v[1])  # both search at the final pose
    assert abs(e - er) <= PARITY_TOL * er, (e, er)

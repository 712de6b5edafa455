"""GPU sweep of estimate_intensity_gradients_gpu and IntegratedColoredGICPFactorGPU over the factor domain of tests/test_factor_domain_gpu.py -- a sensor up to
10 km from the map's origin, rotations near pi, both clouds far from the origin, other units of length -- over 8- and 16-bit intensity ranges and over
near-degenerate neighbourhoods.  Inputs and statements: tests/colored_domain_ref.py (the scene and placements of tests/factor_domain_ref.py, the f64 statements of
tests/colored_ref.py), self-checked on the CPU by tests/test_colored_domain_ref_cpu.py.  Target normals and both covariances are the scene's own.

Gradients.  At each placement the target's neighbour table comes from KdTreeGPU.knn_search and is given to both sides; every full row with cond(H) <= 1e8 (all
but 1 % of a cloud at most) is held to colored_domain_ref.gradient_bound_far = 2^-23 |g| + 16 cond(H) 2^-52 |g| max(1, |p| / rho), the bound of
tests/test_colored_gicp_gpu.py with the cancellation of a = (t - along n) - p at |p| >> |a| in it (derived in the helper, held to the f64 reference on the CPU).
Factor.  The device's f32 gradients are downloaded once per placement and given to the reference.  Asserted (helpers.assert_linearized_close: every block
norm-wise, the error, the inlier count; the stored correspondence count; the error at a nearby pose on the stored correspondences): 1e-7 at |t| = 0, in the
control and in other units, the 1e-5 gate of DESIGN.md section 2 further out.  Every comparison asserts its input condition first
(colored_domain_ref.conditioned); each test prints its worst figure in the [domain] format.

Measured on one MI355X (the unmodified library; worst block over both rotations, both cut-offs and both weights): (a) 3.2e-14 at 0 m (b_source), 4.4e-14 at
100 m, 2.8e-12 at 1000 m, 2.4e-10 at 10 km (H_source from 100 m on; at weight 1 alone, M of rank one: 6.2e-15, 1.8e-14, 2.1e-12, 2.4e-10); the error below 3e-14
everywhere, also at the nearby pose.  (b) 4.7e-14, (c) 1.6e-14, (e) 1.7e-14, (h) 1.3e-10 at 10 km with 16-bit intensities (the photometric share of the error is
0.99997 at x 255 and 1.000000 at x 65535), (s) every field bit-identical, (w) 2.1e-10 / 4.1e-10 at 0.4 rad / pi - 1e-3, (n) all five blocks and the error
non-finite on both sides, 1.0e-14 with the target unmatched, (r) identical bits.  Gradients, largest diff / bound per placement: (G1) 0.485 .. 0.497 at every
placement, distance and table shape, (G2) 0.488 .. 0.499 -- the rounding of the f32 store, half of the bound's first term, decides everywhere: the second term
stays below 1e-8 |g| in the scene (cond(H) <= 58 in metres, 5.8e5 in hundreds of metres); (G3) origin 0.38 / 0.19 / 0.039 at cond(H) 1e4 / 1e6 / 2.5e7, where
the second term takes over (bound 2.6e-5 at 2.5e7), 10 km 0.095 / 1.1e-3 at realised cond(H) 9.0e3 .. 1.05e4 / 5.3e5 .. 1.0e6, and none to compare at 2.5e7
(realised 1.8e16 and beyond); (G4) 257 gradients NaN in every component, 2313 short lists."""
import numpy as np
import pytest

import colored_domain_ref as cd
import colored_ref
import factor_domain_ref as fd
import loam_domain_ref as ld
from helpers import BLOCKS, assert_linearized_close
from icp_ref import nearest_two, transform

pytestmark = pytest.mark.gpu
HASHED = 1  # GP_TUNE_KNN_STRUCTURE, as tests/test_knn_edges_gpu.py
FIELDS = BLOCKS + ["error", "num_inliers"]
PLACEMENTS = list(cd.placements())
SWEEP = list(cd.sweep())
_DEVICE = {}


def _device(gpu, maker, args, intensity_scale=1.0):
    """one placement on the device, built once: target (points, covariances, normals, intensities), source, the search structure over the target in the case's
    units, the k = 10 table of the target, the gradients on it and their download"""
    key = (maker, tuple(args), float(intensity_scale))
    if key not in _DEVICE:
        d, _, _, _, unit = cd.case(maker, args, intensity_scale)
        tgt = gpu.PointCloudGPU(d["target_points"], d["target_covs"], normals=d["target_normals"], intensities=d["target_intensities"])
        src = gpu.PointCloudGPU(d["source_points"], d["source_covs"], intensities=d["source_intensities"])
        tree = gpu.KdTreeGPU(tgt, cell_size=0.25 * unit)
        table, _, found = tree.knn_search(d["target_points"], 10)
        assert (found == 10).all()
        grads = gpu.estimate_intensity_gradients_gpu(tgt, neighbors=table, k_photo_neighbors=10)
        _DEVICE[key] = dict(tgt=tgt, src=src, tree=tree, table=table, grads=grads, tgrad=grads.download())
    return _DEVICE[key]


# ---- gradients ----------------------------------------------------------------------------------------------------------------------------------------------------------
def _compare_gradients(what, got, points, normals, intensities, table, k_photo, rows=None, cap_share=0.01):
    """the device's gradients against the f64 statement on the same table within gradient_bound_far, on `rows` (default: every full row) with cond(H) <= COND_CAP
    -> the number compared"""
    ref, cond, rho = cd.gradient_reference(points, normals, intensities, table, k_photo)
    full = (np.asarray(table)[:, :k_photo] >= 0).all(axis=1)
    assert got.shape == ref.shape and got.dtype == np.float32
    assert not got[~full].any()  # (0, 0, 0) where one of the first k_photo slots is empty
    at = full if rows is None else np.isin(np.arange(len(ref)), rows)
    assert not (at & ~full).any()
    compared = at & (cond <= colored_ref.COND_CAP)
    assert (at & ~compared).sum() <= cap_share * len(ref), (what, int((at & ~compared).sum()))
    if not compared.any():
        print(f"[domain] {what}: no point within the cond(H) cap")
        return 0
    diff = np.abs(got.astype(np.float64) - ref).max(axis=1)
    bound = cd.gradient_bound_far(ref, cond, points, rho)
    ratio = np.where(compared, diff / np.maximum(bound, 1e-300), 0.0)
    worst = int(np.argmax(ratio))
    amp = np.abs(np.asarray(points, dtype=np.float64)).max(axis=1)[worst] / rho[worst]
    print(f"[domain] {what}: {int(compared.sum())} compared, largest diff / bound {ratio[worst]:.3e} at point {worst} (diff {diff[worst]:.3e}, bound {bound[worst]:.3e}, "
          f"cond(H) {cond[worst]:.3g}, |p| / rho {amp:.3g}), cond(H) up to {cond[compared].max():.3g}")
    assert np.isfinite(got[compared]).all(), what
    assert (diff[compared] <= bound[compared]).all(), (what, worst, diff[worst], bound[worst])
    assert got[compared].any()
    return int(compared.sum())


def _gradient_placement(gpu, name, maker, args, k, k_photo, intensity_scale=1.0):
    d, _, _, _, unit = cd.case(maker, args, intensity_scale)
    dev = _device(gpu, maker, args, intensity_scale)
    tp = d["target_points"]
    if k == 10:
        table = dev["table"]
        got = dev["tgrad"] if k_photo == 10 else None
    else:
        table, _, found = dev["tree"].knn_search(tp, k)
        assert (found == k).all()
        got = None
    if got is None:
        got = gpu.estimate_intensity_gradients_gpu(dev["tgt"], neighbors=table, k_photo_neighbors=k_photo).download()
    what = f"gradients {name} k = {k}, k_photo = {k_photo}" + (f", intensities x {intensity_scale:g}" if intensity_scale != 1.0 else "")
    assert _compare_gradients(what, got, tp, d["target_normals"], d["target_intensities"], table, k_photo) >= 0.99 * len(tp)
    # the entry point that searches for itself: no short list, and on all k slots the same bits
    own = gpu.estimate_intensity_gradients_gpu(dev["tgt"], k, cell_size=0.25 * unit)
    assert own.num_short == 0 and own.size() == len(tp)
    if k_photo == k:
        assert np.array_equal(own.download(), got), what


@pytest.mark.parametrize("k,k_photo", cd.K_GRADIENTS)
@pytest.mark.parametrize("name,maker,args,far", PLACEMENTS, ids=[p[0] for p in PLACEMENTS])
def test_gradients_over_the_domain(gpu, name, maker, args, far, k, k_photo):
    """(G1) every placement of (a), (b), (c) at k = 10 and at k = 32 with the first 10 slots used"""
    _gradient_placement(gpu, name, maker, args, k, k_photo)


@pytest.mark.parametrize("intensity_scale,distance,rotation", cd.HIGH_RANGE)
def test_gradients_of_8_and_16_bit_intensities(gpu, intensity_scale, distance, rotation):
    """(G2) the same bound, which is relative to |g|"""
    _gradient_placement(gpu, f"a {distance:g} m {rotation}", "scan_to_map", (distance, rotation), 10, 10, intensity_scale)


def _cluster_gradients(gpu, scene):
    """a cluster scene on the device: (table of the search within RADIUS, the gradients on it)"""
    frame = gpu.PointCloudGPU(scene["points"], normals=scene["normals"], intensities=scene["intensities"])
    table, _, found = gpu.KdTreeGPU(frame).knn_search(scene["points"], cd.K_CLUSTER, cd.RADIUS**2)
    full = found == cd.K_CLUSTER
    assert np.array_equal(np.flatnonzero(full), np.sort(scene["centres"])) and ((table >= 0).all(axis=1) == full).all()  # only the centres have all nine neighbours
    return table, gpu.estimate_intensity_gradients_gpu(frame, neighbors=table).download()


@pytest.mark.parametrize("cond_target,far", cd.STRIP_CASES, ids=[f"{c:g}-{'10km' if far else 'origin'}" for c, far in cd.STRIP_CASES])
def test_gradients_of_strip_clusters(gpu, cond_target, far):
    """(G3) 257 isolated clusters whose neighbours lie in a narrow strip: cond(H) about 1e4, 1e6, 2.5e7.  All 257 centres are compared wherever the f32 inputs
    realise a cond(H) within the cap (tests/test_colored_domain_ref_cpu.py::test_strip_scene: everywhere but at 10 km with the last target, where the 2^-11 m
    grid swallows the offsets across the strip and nothing can be compared)"""
    what = f"strips cond {cond_target:g} {'10 km' if far else 'origin'}"
    s = cd.strip_scene(cond_target, far)
    table, got = _cluster_gradients(gpu, s)
    low, high = cd.realised(s, table)
    print(f"[domain] {what}: realised cond(H) {low:.4g} .. {high:.4g}")
    compared = _compare_gradients(what, got, s["points"], s["normals"], s["intensities"], table, cd.K_CLUSTER, rows=s["centres"], cap_share=1.0)
    assert compared == cd.STRIP_COMPARED[(cond_target, far)]
    assert (np.count_nonzero(got, axis=1) > 0).sum() <= cd.CLUSTERS


def test_gradients_of_collinear_clusters(gpu):
    """(G4) det H = 0 exactly (exact inputs, exact products): every centre's stored gradient is non-finite in every component, as the reference's is -- "a singular H
    is not guarded" as it stands; every other point has a short list within RADIUS and gets (0, 0, 0).  (The count of short lists, 2570 - 257, is taken from the
    table: the entry point on a caller's table does not report num_short.)"""
    s = cd.collinear_scene()
    table, got = _cluster_gradients(gpu, s)
    ref, _ = colored_ref.intensity_gradients(s["points"], s["normals"], s["intensities"], table)
    short = (table < 0).any(axis=1)
    print(f"[domain] collinear clusters: {int((~np.isfinite(got)).all(axis=1).sum())} gradients non-finite in every component, {int(short.sum())} short lists")
    assert not np.isfinite(ref[s["centres"]]).any() and not np.isfinite(got[s["centres"]]).any()
    assert int(short.sum()) == len(got) - cd.CLUSTERS and not got[short].any() and not ref[short].any()


# ---- the factor -----------------------------------------------------------------------------------------------------------------------------------------------------------
def _factor(gpu, dev, cutoff, weight, src=None, tree=None, grads=None):
    return gpu.IntegratedColoredGICPFactorGPU(0, 1, dev["tgt"], src if src is not None else dev["src"], target_tree=tree if tree is not None else dev["tree"],
                                              target_gradients=grads if grads is not None else dev["grads"], max_correspondence_distance=cutoff,
                                              photometric_term_weight=weight)


def _report(what, L, ref, tol, path="f64 rigid sums + adjoint"):
    worst, block, errs = fd.worst_block(L, ref)
    e = abs(L.error - ref["error"]) / ref["error"] if ref["error"] else abs(L.error)
    print(f"[domain] {what}: path {path}, worst block {block} {worst:.3e} (H_source {errs['H_source']:.3e}, b_source {errs['b_source']:.3e}, H_target {errs['H_target']:.3e}), "
          f"error {e:.3e}, inliers {L.num_inliers} / {ref['num_inliers']}, asserted at {tol:.0e}")
    return worst


def _check(gpu, d, dev, delta, near, cutoff, weight, tol, what, src=None, path="f64 rigid sums + adjoint"):
    """one factor on the device against colored_ref at `delta`: the record, the inlier and correspondence counts, the error at `near` on the stored correspondences"""
    ref = cd.make_ref(d, dev["tgrad"], cutoff, weight)
    f = _factor(gpu, dev, cutoff, weight, src)
    cd.conditioned(ref, delta, what)
    L, Lr = f.linearize_delta(delta), ref.linearize(delta)
    _report(what, L, Lr, tol, path)
    assert_linearized_close(L, Lr, tol, what)
    assert f.num_inliers() == Lr["num_inliers"] == f._lib.gp_colored_gicp_factor_num_correspondences(f._h), what
    for k in BLOCKS + ["error"]:
        assert np.isfinite(getattr(L, k)).all(), k
    e, er = f.error({0: np.eye(4), 1: near}), ref.error(near)
    print(f"[domain] {what}: error at the nearby pose {abs(e - er) / er if er else abs(e):.3e}")
    assert ref.searches == 1 and abs(e - er) <= tol * max(er, 1e-300), (what, e, er)
    return f, L, Lr, ref


@pytest.mark.parametrize("name,maker,args,cutoff,weight,far", SWEEP, ids=[s[0] for s in SWEEP])
def test_factor_over_the_domain(gpu, name, maker, args, cutoff, weight, far):
    """(F-a) scan to map at 0 m .. 10 km, both rotations, cut-offs 1 and 0.5, weights 0.25 and 1 (M of rank one, H_source rank deficient); (F-b) both clouds 1000 m
    out, the relative pose near identity; (F-c) the scene in centimetres, metres and hundreds of metres, the cut-off one metre in those units"""
    d, delta, near, _, _ = cd.case(maker, args)
    tol = cd.tolerance(far) if maker == "scan_to_map" else cd.PARITY_TOL
    _, L, _, _ = _check(gpu, d, _device(gpu, maker, args), delta, near, cutoff, weight, tol, f"({'abc'[['scan_to_map', 'both_far', 'scaled'].index(maker)]}) colored {name}")
    assert L.num_inliers > 2000


@pytest.mark.parametrize("weight", cd.GENERAL_WEIGHTS)
def test_non_orthonormal_block_at_1000m(gpu, weight):
    """(F-e) test_loam_gpu.py's perturbation of the 3x3 block, 1000 m out, the source re-filtered for that pose: the general kernels (92 explicit sums, J_s from
    the block as given) with the rank-one part in them, held to the gate"""
    d, delta, _, _, _ = cd.case("scan_to_map", (1000.0, "0.4rad"))
    skew = ld.non_orthonormal(delta)
    assert np.abs(skew[:3, :3].T @ skew[:3, :3] - np.eye(3)).max() > 1e-7
    d2, dropped = cd.with_margin(d, skew)
    assert dropped <= fd.DROP_CAP
    src = gpu.PointCloudGPU(d2["source_points"], d2["source_covs"], intensities=d2["source_intensities"])
    _, L, _, _ = _check(gpu, d2, _device(gpu, "scan_to_map", (1000.0, "0.4rad")), skew, skew @ fd.expmap(cd.NEARBY), 1.0, weight, cd.GATE,
                        f"(e) colored non-orthonormal 1000 m weight {weight:g}", src=src, path="explicit J_s")
    assert L.num_inliers > 2000


@pytest.mark.parametrize("intensity_scale,distance,rotation", cd.HIGH_RANGE)
def test_factor_with_8_and_16_bit_intensities(gpu, intensity_scale, distance, rotation):
    """(F-h) r_p and the gradients 255 and 65535 times larger: the two parts of the error differ by up to ten orders of magnitude"""
    d, delta, near, _, _ = cd.case("scan_to_map", (distance, rotation), intensity_scale)
    dev = _device(gpu, "scan_to_map", (distance, rotation), intensity_scale)
    _, L, _, ref = _check(gpu, d, dev, delta, near, 1.0, 0.25, cd.tolerance(distance > 0), f"(h) colored {distance:g} m {rotation} intensities x {intensity_scale:g}")
    print(f"[domain] (h) intensities x {intensity_scale:g}: photometric share of the error {cd.photometric_share(ref, delta):.6f}")
    assert L.num_inliers > 2000


@pytest.mark.parametrize("distance,rotation", cd.HASHED_CASES)
def test_hashed_structure_gives_the_same_record(gpu, distance, rotation):
    """(F-s) the factor on the hashed search structure: every field of the record bit-identical to the default structure's"""
    d, delta, _, _, _ = cd.case("scan_to_map", (distance, rotation))
    dev = _device(gpu, "scan_to_map", (distance, rotation))
    A = _factor(gpu, dev, 1.0, 0.25).linearize_delta(delta)
    B = _factor(gpu, dev, 1.0, 0.25, tree=gpu.KdTreeGPU(dev["tgt"], structure=HASHED)).linearize_delta(delta)
    print(f"[domain] (s) hashed structure {distance:g} m {rotation}: {A.num_inliers} / {B.num_inliers} inliers, error {A.error!r} / {B.error!r}")
    assert A.num_inliers > 2000
    for k in FIELDS:
        assert np.array_equal(getattr(A, k), getattr(B, k)), k


@pytest.mark.parametrize("rotation", list(fd.ROTATIONS))
def test_weight_zero_is_the_gicp_factor_at_10km(gpu, rotation):
    """(F-w) weight 0 against IntegratedGICPFactorGPU on the same clouds, 10 km out, at the gate"""
    d, delta, _, _, _ = cd.case("scan_to_map", (cd.FAR, rotation))
    dev = _device(gpu, "scan_to_map", (cd.FAR, rotation))
    cd.conditioned(cd.make_ref(d, dev["tgrad"], 1.0, 0.0), delta, f"(w) gicp 10 km {rotation}")
    L = _factor(gpu, dev, 1.0, 0.0).linearize_delta(delta)
    Lg = gpu.IntegratedGICPFactorGPU(0, 1, dev["tgt"], dev["src"]).linearize_delta(delta)
    _report(f"(w) weight 0 against GICP, 10 km {rotation}", L, {k: getattr(Lg, k) for k in FIELDS}, cd.GATE)
    assert L.num_inliers > 2000
    assert_linearized_close(L, Lg, cd.GATE, "weight 0 against GICP at 10 km")


def test_one_non_finite_gradient_reaches_the_record(gpu):
    """(F-n) the contract of "a singular H is not guarded" as it stands, one step on: the gradient of ONE matched target point is NaN on both sides.  Device and
    reference agree on which fields of the record are non-finite; with the cut-off at 0.5, where that target is no longer matched (asserted on the reference),
    the same factor is finite and within 1e-7"""
    import torch

    maker, args = "scan_to_map", (0.0, "0.4rad")
    d, delta, _, _, _ = cd.case(maker, args)
    dev = _device(gpu, maker, args)
    probe = cd.make_ref(d, dev["tgrad"], 1.0, 0.25)
    cd.conditioned(probe, delta, "(n) cut-off 1")
    probe.update_correspondences(delta)
    _, d1, _ = nearest_two(probe.target, transform(delta, probe.source))
    matched = probe.correspondences >= 0
    nearest = np.full(len(probe.target), np.inf)
    np.minimum.at(nearest, probe.correspondences[matched], d1[matched])
    candidates = np.flatnonzero(np.isfinite(nearest) & (nearest > 0.3) & (nearest < 0.9))  # matched at 1.0, every match beyond 0.5 (0.25 squared)
    assert len(candidates) > 0
    j = int(candidates[0])
    tgrad = dev["tgrad"].copy()
    tgrad[j] = np.nan
    g = dev["grads"].gradients_gpu.clone()
    g[j] = float("nan")
    torch.cuda.synchronize()
    grads = gpu.IntensityGradientsGPU(g)
    ref = cd.make_ref(d, tgrad, 1.0, 0.25)
    L, Lr = _factor(gpu, dev, 1.0, 0.25, grads=grads).linearize_delta(delta), ref.linearize(delta)
    assert (ref.correspondences == j).any() and L.num_inliers == Lr["num_inliers"]
    bad = {k: not np.isfinite(getattr(L, k)).all() for k in BLOCKS + ["error"]}
    bad_ref = {k: not np.isfinite(Lr[k]).all() for k in BLOCKS + ["error"]}
    print(f"[domain] (n) target {j} with a NaN gradient: non-finite fields on the device {sorted(k for k in bad if bad[k])}, in the reference {sorted(k for k in bad_ref if bad_ref[k])}")
    assert bad == bad_ref and bad["error"]
    ref = cd.make_ref(d, tgrad, 0.5, 0.25)
    cd.conditioned(ref, delta, "(n) cut-off 0.5")
    f = _factor(gpu, dev, 0.5, 0.25, grads=grads)
    L, Lr = f.linearize_delta(delta), ref.linearize(delta)
    assert not (ref.correspondences == j).any() and Lr["num_inliers"] > 2000
    _report(f"(n) cut-off 0.5, target {j} unmatched", L, Lr, cd.PARITY_TOL)
    for k in BLOCKS + ["error"]:
        assert np.isfinite(getattr(L, k)).all(), k
    assert_linearized_close(L, Lr, cd.PARITY_TOL, "(n) cut-off 0.5")


@pytest.mark.parametrize("rotation", list(fd.ROTATIONS))
def test_two_linearises_are_bit_identical_at_10km(gpu, rotation):
    """(F-r) two linearises and a fresh factor give identical bits 10 km out, on the rigid and on the general path"""
    d, delta, _, _, _ = cd.case("scan_to_map", (cd.FAR, rotation))
    dev = _device(gpu, "scan_to_map", (cd.FAR, rotation))
    for pose in (delta, delta @ np.diag([1.0 + 1e-6, 1.0, 1.0, 1.0])):
        f = _factor(gpu, dev, 1.0, 0.25)
        A, B = f.linearize_delta(pose), f.linearize_delta(pose)
        Cc = _factor(gpu, dev, 1.0, 0.25).linearize_delta(pose)
        for k in FIELDS:
            assert np.array_equal(getattr(A, k), getattr(B, k)) and np.array_equal(getattr(A, k), getattr(Cc, k)), k
        assert A.num_inliers > 2000

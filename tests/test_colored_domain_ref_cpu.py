"""Self-check of tests/colored_domain_ref.py, the inputs and statements of the colored GICP factor-domain sweep (no GPU needed).

For every placement tests/test_colored_domain_gpu.py runs: the input condition of test_colored_gicp_gpu.py holds, the case keeps a floor of inliers, neither term
of the error hides behind the other, and the bound the device's gradients are held to (colored_domain_ref.gradient_bound_far, a derivation) holds the f64
reference itself to a quarter against the same statement in long double.  Where the GPU tests take the target's gradients and the neighbour tables from the
device, these take them from the f64 statement on the exact tables of tests/knn_ref.py."""
import numpy as np
import pytest

import colored_domain_ref as cd
import colored_ref
import factor_domain_ref as fd
import loam_domain_ref as ld
from helpers import rel_err

PLACEMENTS = list(cd.placements())
GRADIENT_PLACEMENTS = [(name, maker, args, 1.0) for name, maker, args, _ in PLACEMENTS] + [
    (f"a {t:g} m {r} intensities x {s:g}", "scan_to_map", (t, r), s) for s, t, r in cd.HIGH_RANGE]
_GRADIENTS = {}


def _host_gradients(maker, args, intensity_scale=1.0):
    """the f64 statement's gradients of a placement's target on the exact k = 10 table, rounded to f32 as the device stores them"""
    key = (maker, tuple(args), intensity_scale)
    if key not in _GRADIENTS:
        d = cd.case(maker, args, intensity_scale)[0]
        g, _ = colored_ref.intensity_gradients(d["target_points"], d["target_normals"], d["target_intensities"], cd.host_table(d["target_points"], 10))
        _GRADIENTS[key] = g.astype(np.float32)
    return _GRADIENTS[key]


@pytest.mark.parametrize("name,maker,args,far", PLACEMENTS, ids=[p[0] for p in PLACEMENTS])
def test_sweep_case(name, maker, args, far):
    """the cases of (F-a) .. (F-c) on one placement: conditioned, more than 2000 inliers at the full cut-off, the cut-off of 0.5 bites, and at weight 0.25 the
    photometric term carries between 5 % and 95 % of the reference's error"""
    d, delta, near, dropped, unit = cd.case(maker, args)
    n = len(d["source_points"])
    assert dropped <= fd.DROP_CAP and n >= (1.0 - fd.DROP_CAP) * fd.N_SOURCE and len(d["source_intensities"]) == n and len(d["target_intensities"]) == len(d["target_points"])
    grads = _host_gradients(maker, args)
    inliers = {}
    for cname, cmaker, cargs, cutoff, weight, cfar in cd.sweep():
        if (cmaker, cargs) != (maker, args):
            continue
        assert cfar == far
        ref = cd.make_ref(d, grads, cutoff, weight)
        cd.conditioned(ref, delta, cname)
        L = ref.linearize(delta)
        inliers[cutoff] = L["num_inliers"]
        share = cd.photometric_share(ref, delta)
        print(f"[colored domain ref] {cname}: {L['num_inliers']} inliers of {n}, photometric share of the error {share:.3f}")
        if cutoff == unit:
            assert L["num_inliers"] > 2000
        if weight == 0.25:
            assert 0.05 <= share <= 0.95, (cname, share)
        else:
            assert weight != 1.0 or abs(share - 1.0) < 1e-12
        assert ref.error(near) > 0.0 and ref.searches == 1
    if maker == "scan_to_map":
        assert inliers[0.5] < inliers[1.0]


def test_intensities_are_the_same_at_every_placement():
    """the field is evaluated in the sensor frame before placement and scaling: a target point kept at two placements carries the same f32 intensity, and the
    intensity scales multiply it"""
    a, b = cd.case("scan_to_map", (0.0, "0.4rad"))[0], cd.case("scaled", (100.0,))[0]
    s = fd.scene()
    full = (cd.field(s["target_points"])).astype(np.float32)
    for d in (a, b):
        assert np.isin(d["target_intensities"], full).all()
    assert 100.0 < np.abs(full).max() < 1000.0 and full.std() > 10.0
    hi = cd.case("scan_to_map", (0.0, "0.4rad"), 65535.0)[0]
    assert np.array_equal(hi["target_points"], a["target_points"])
    assert np.abs(hi["target_intensities"] / a["target_intensities"] - 65535.0).max() < 65535.0 * 2.0**-22
    src = cd.field(s["source_points"])
    assert len(hi["source_points"]) < fd.N_SOURCE or 0.005 < (hi["source_intensities"] / 65535.0 - src).std() < 0.02  # N(0, 0.01) beside the f32 rounding of 650


def test_long_double_statement_in_f64_is_the_statement():
    d = cd.case("scan_to_map", (0.0, "0.4rad"))[0]
    tab = cd.host_table(d["target_points"], 10)
    a, ca = colored_ref.intensity_gradients(d["target_points"], d["target_normals"], d["target_intensities"], tab)
    b, cb = colored_ref.intensity_gradients(d["target_points"], d["target_normals"], d["target_intensities"], tab, dtype=np.float64)
    x, _ = colored_ref.intensity_gradients(d["target_points"], d["target_normals"], d["target_intensities"], tab, dtype=np.longdouble)
    assert a.dtype == np.float64 and x.dtype == np.longdouble and np.array_equal(a, b) and np.array_equal(ca, cb)
    assert 0.0 < np.abs(a - x).max() < 1e-9 * np.abs(a).max()


def _held_to_the_reference(what, points, normals, intensities, table, k_photo, cap_share=0.01):
    """reorder ratio <= GRADIENT_C / 4 and |g_f64 - g_longdouble|_inf <= gradient_bound_far / 4 on every full row with cond(H) <= COND_CAP -> the two largest ratios"""
    g, cond, rho = cd.gradient_reference(points, normals, intensities, table, k_photo)
    x, _, _ = cd.gradient_reference(points, normals, intensities, table, k_photo, dtype=np.longdouble)
    full = (np.asarray(table)[:, :k_photo] >= 0).all(axis=1)
    keep = full & (cond <= colored_ref.COND_CAP)
    assert (full & ~keep).sum() <= cap_share * len(g), (what, int((full & ~keep).sum()))
    if not keep.any():
        print(f"[colored domain ref] {what}: no point within the cond(H) cap")
        return 0.0, 0.0
    bound = cd.gradient_bound_far(g, cond, points, rho)
    ratio = np.abs(g - x).max(axis=1).astype(np.float64)[keep] / bound[keep]
    reorder = colored_ref.reorder_ratio(points, normals, intensities, table, k_photo)
    amp = np.abs(np.asarray(points, dtype=np.float64)).max(axis=1)[keep] / rho[keep]
    print(f"[colored domain ref] {what}: {int(keep.sum())} compared, cond(H) up to {cond[keep].max():.3g}, |p| / rho up to {amp.max():.3g}, f64 against long double / bound "
          f"{ratio.max():.2e}, reorder ratio {reorder.max():.2f}")
    assert np.isfinite(g[keep]).all() and reorder.max() <= colored_ref.GRADIENT_C / 4.0, (what, reorder.max())
    assert ratio.max() <= 0.25, (what, ratio.max())
    return float(ratio.max()), float(reorder.max())


@pytest.mark.parametrize("name,maker,args,intensity_scale", GRADIENT_PLACEMENTS, ids=[p[0] for p in GRADIENT_PLACEMENTS])
def test_gradient_bound_holds_the_reference(name, maker, args, intensity_scale):
    """(G1), (G2) on the CPU.  Measured: the module docstring of tests/colored_domain_ref.py"""
    if not np.finfo(np.longdouble).eps < 1e-18:
        pytest.skip("this platform's long double is no wider than double")
    d = cd.case(maker, args, intensity_scale)[0]
    for k, k_photo in cd.K_GRADIENTS:
        _held_to_the_reference(f"{name} k = {k}, k_photo = {k_photo}", d["target_points"], d["target_normals"], d["target_intensities"], cd.host_table(d["target_points"], k), k_photo)


@pytest.mark.parametrize("cond_target,far", cd.STRIP_CASES, ids=[f"{c:g}-{'10km' if far else 'origin'}" for c, far in cd.STRIP_CASES])
def test_strip_scene(cond_target, far):
    """(G3) on the CPU: only the centres have a full list within RADIUS; at the origin cond(H) is within a factor 2 of its target and below the cap; at 10 km the
    2^-11 m f32 grid decides (printed), and the number of centres it leaves within the cap is the one the GPU test compares"""
    s = cd.strip_scene(cond_target, far)
    assert s["points"].shape == (cd.CLUSTERS * cd.K_CLUSTER, 3) and s["points"].dtype == np.float32 and np.abs(s["points"]).max() < 8192.0 and cd.CLUSTERS == 256 + 1
    table = cd.host_table(s["points"], cd.K_CLUSTER, cd.RADIUS)
    full = (table >= 0).all(axis=1)
    assert np.array_equal(np.sort(np.flatnonzero(full)), np.sort(s["centres"]))
    low, high = cd.realised(s, table)
    _, cond = colored_ref.intensity_gradients(s["points"], s["normals"], s["intensities"], table)
    within = int((cond[s["centres"]] <= colored_ref.COND_CAP).sum())
    print(f"[colored domain ref] strips cond {cond_target:g} {'10 km' if far else 'origin'}: realised cond(H) {low:.4g} .. {high:.4g}, {within} centres within the cap")
    assert within == cd.STRIP_COMPARED[(cond_target, far)]
    if not far:
        assert 0.5 * cond_target <= low <= high <= 2.0 * cond_target and high < colored_ref.COND_CAP
    if not np.finfo(np.longdouble).eps < 1e-18:
        pytest.skip("this platform's long double is no wider than double")
    _held_to_the_reference(f"strips cond {cond_target:g} {'10 km' if far else 'origin'}", s["points"], s["normals"], s["intensities"], table, cd.K_CLUSTER, cap_share=1.0)


def test_collinear_scene():
    """(G4) on the CPU: exact inputs, det H = 0 exactly, and the f64 statement's gradient is non-finite in every component for every centre"""
    s = cd.collinear_scene()
    table = cd.host_table(s["points"], cd.K_CLUSTER, cd.RADIUS)
    full = (table >= 0).all(axis=1)
    assert np.array_equal(np.sort(np.flatnonzero(full)), np.sort(s["centres"]))
    rows, H, e, _ = colored_ref.gradient_systems(s["points"], s["normals"], s["intensities"], table)
    assert np.array_equal(rows, np.sort(s["centres"]))
    Hx = colored_ref.gradient_systems(s["points"], s["normals"], s["intensities"], table, dtype=np.longdouble)[1]
    assert np.array_equal(H.astype(np.longdouble), Hx)  # nothing was rounded
    det = H[:, 0, 0] * (H[:, 1, 1] * H[:, 2, 2] - H[:, 1, 2] ** 2) + H[:, 0, 1] * (H[:, 0, 2] * H[:, 1, 2] - H[:, 0, 1] * H[:, 2, 2]) + H[:, 0, 2] * (H[:, 0, 1] * H[:, 1, 2] - H[:, 0, 2] * H[:, 1, 1])
    assert not det.any() and np.abs(e).max() > 0.0
    g, cond = colored_ref.intensity_gradients(s["points"], s["normals"], s["intensities"], table)
    assert not np.isfinite(g[s["centres"]]).any() and not g[~full].any() and (cond[s["centres"]] > colored_ref.COND_CAP).all()


def test_record_matches_central_differences_at_10km():
    """test_colored_ref_cpu.test_record_matches_finite_differences_and_gauss_newton_products's method and tolerance (1e-6) on the (10 km, pi - 1e-3) placement at
    weight 0.25: b = J^T rho = grad(error) / 2 and H = J^T J with J the central differences of residuals(), for a source and a target perturbation"""
    d, delta, _, _, _ = cd.case("scan_to_map", (cd.FAR, "pi-1e-3"))
    ref = cd.make_ref(d, _host_gradients("scan_to_map", (cd.FAR, "pi-1e-3")), 1.0, 0.25)
    L = ref.linearize(delta)
    assert L["num_inliers"] > 2000
    h = 1e-6
    source = lambda xi: delta @ fd.expmap(xi)  # noqa: E731
    target = lambda xi: fd.expmap(-np.asarray(xi)) @ delta  # noqa: E731
    J, grad = {}, {}
    for name, move in (("source", source), ("target", target)):
        J[name] = np.stack([(ref.residuals(move(h * e)) - ref.residuals(move(-h * e))) / (2 * h) for e in np.eye(6)], axis=2)
        grad[name] = np.array([(ref.error(move(h * e)) - ref.error(move(-h * e))) / (2 * h) for e in np.eye(6)])
    rho = ref.residuals(delta)
    assert abs((rho * rho).sum() - L["error"]) <= 1e-12 * L["error"]
    for name in ("source", "target"):
        figures = (rel_err(np.einsum("nki,nk->i", J[name], rho), L["b_" + name]), rel_err(0.5 * grad[name], L["b_" + name]), rel_err(np.einsum("nki,nkj->ij", J[name], J[name]), L["H_" + name]))
        print(f"[colored domain ref] central differences at 10 km, {name}: J^T rho {figures[0]:.2e}, grad / 2 {figures[1]:.2e}, J^T J {figures[2]:.2e}")
        assert max(figures) < 1e-6, (name, figures)
    assert rel_err(np.einsum("nki,nkj->ij", J["target"], J["source"]), L["H_target_source"]) < 1e-6
    assert ref.searches == 1


def test_non_orthonormal_case():
    """(F-e): the perturbed block at 1000 m, the source re-filtered: conditioned at the three weights, more than 2000 inliers"""
    d, delta, _, _, _ = cd.case("scan_to_map", (1000.0, "0.4rad"))
    skew = ld.non_orthonormal(delta)
    assert np.abs(skew[:3, :3].T @ skew[:3, :3] - np.eye(3)).max() > 1e-7
    d2, dropped = cd.with_margin(d, skew)
    assert dropped <= fd.DROP_CAP and len(d2["source_intensities"]) == len(d2["source_points"])
    for weight in cd.GENERAL_WEIGHTS:
        ref = cd.make_ref(d2, _host_gradients("scan_to_map", (1000.0, "0.4rad")), 1.0, weight)
        cd.conditioned(ref, skew, f"non-orthonormal 1000 m weight {weight:g}")
        assert ref.linearize(skew)["num_inliers"] > 2000


def test_case_list():
    """the lists the GPU file is parametrised with contain every item of the sweep: (a) 4 distances x 2 rotations, (b), (c) 3 units; 2 cut-offs and 2 weights in
    (a); both table shapes; the high intensity ranges at both ends; 3 strip targets x 2 placements; the hashed structure at 10 km with both rotations"""
    names = [p[0] for p in PLACEMENTS]
    assert len(names) == len(set(names)) == 8 + 1 + 3
    assert {(m, a) for _, m, a, _ in PLACEMENTS} == {("scan_to_map", (t, r)) for t in (0.0, 100.0, 1000.0, 10000.0) for r in ("0.4rad", "pi-1e-3")} | {("both_far", ())} | {
        ("scaled", (s,)) for s in (0.01, 1.0, 100.0)}
    sweep = list(cd.sweep())
    assert len(sweep) == 8 * 2 * 2 + 2 + 3 * 2
    for t in (0.0, 100.0, 1000.0, 10000.0):
        for r in ("0.4rad", "pi-1e-3"):
            for c in (1.0, 0.5):
                for w in (0.25, 1.0):
                    assert ("scan_to_map", (t, r), c, w, t > 0) in [s[1:] for s in sweep]
    for s in (0.01, 1.0, 100.0):
        assert [x[3] for x in sweep if x[1] == "scaled" and x[2] == (s,)] == [s, s]  # the cut-off is one unit
    assert all(not far for _, m, _, _, _, far in sweep if m != "scan_to_map")
    assert cd.K_GRADIENTS == [(10, 10), (32, 10)] and cd.INTENSITY_SCALES == [1.0, 255.0, 65535.0]
    assert set(cd.HIGH_RANGE) == {(s, t, r) for s in (255.0, 65535.0) for t, r in ((0.0, "0.4rad"), (10000.0, "pi-1e-3"))}
    assert set(cd.STRIP_CASES) == {(c, f) for c in (1e4, 1e6, 2.5e7) for f in (False, True)} and set(cd.STRIP_COMPARED) == set(cd.STRIP_CASES)
    assert cd.GENERAL_WEIGHTS == [0.0, 0.25, 1.0] and set(cd.HASHED_CASES) == {(10000.0, "0.4rad"), (10000.0, "pi-1e-3")}
    assert (cd.PARITY_TOL, cd.GATE, cd.MARGIN) == (ld.PARITY_TOL, ld.GATE, ld.MARGIN) and np.array_equal(cd.NEARBY, ld.NEARBY)
    assert cd.tolerance(False) == 1e-7 and cd.tolerance(True) == 1e-5

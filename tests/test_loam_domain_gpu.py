"""GPU sweep of the LOAM point-to-edge, point-to-plane and combined factors over the factor domain of tests/test_factor_domain_gpu.py -- a sensor up to 10 km from
the map's origin, rotations near pi, both clouds far from the origin, other units of length -- and over near-degenerate neighbours.  Inputs and statements:
tests/loam_domain_ref.py (the scene and placements of tests/factor_domain_ref.py, the f64 reference of tests/loam_ref.py), self-checked on the CPU by
tests/test_loam_domain_ref_cpu.py.  The target cloud is edge target and plane target at once, the source both sources.

Asserted (helpers.assert_linearized_close: every block norm-wise, the error, the inlier count; the per-part counts; the error at a nearby pose on the stored
correspondences): test_loam_gpu.py's 1e-7 at |t| = 0, in the control and in other units, the 1e-5 gate of DESIGN.md section 2 further out.  The correspondence
factors have no far-pose routing: a rigid pose at any distance takes the f64 rigid sums + the adjoint expansion, with the edge term's full rank-2 M in them.
Every comparison asserts its input condition first (loam_domain_ref.conditioned); each test prints its worst block figure in the [domain] format.

Measured on one MI355X (worst block over the three kinds, both rotations and both cut-offs; the unmodified library): (a) 7.0e-15 at 0 m (b_source), 2.1e-14 at
100 m, 2.5e-12 at 1000 m, 1.8e-10 at 10 km (H_source from 100 m on); the error below 5e-15 everywhere.  (b) 1.2e-14, (c) 5.0e-15, (e) 6.4e-15, (f) LOAM members
6.3e-15 / 1.5e-10 and the GICP member 4.5e-15 / 3.2e-10 at 0 m / 10 km, every record bit-identical to the single-factor call, (g) 3.7e-15 at 0 m, 8.8e-15 at 100 m,
all zero at 10 km; (d) no row differs on either structure; the clusters 3.3e-15 at the origin and 3.7e-13 at 10 km (b_target)."""
import numpy as np
import pytest

import factor_domain_ref as fd
import loam_domain_ref as ld
import loam_ref
import oracle
from helpers import BLOCKS, assert_linearized_close

pytestmark = pytest.mark.gpu
HASHED = 1  # GP_TUNE_KNN_STRUCTURE, as tests/test_knn_edges_gpu.py
FIELDS = BLOCKS + ["error", "num_inliers"]
_DEVICE = {}


def _device(gpu, key, d, structure=0):
    """target cloud (with covariances, for the GICP member), source cloud and the search structure over the target, built once per placement"""
    key = key + (structure,)
    if key not in _DEVICE:
        tgt = gpu.PointCloudGPU(d["target_points"], d["target_covs"])
        src = gpu.PointCloudGPU(d["source_points"], d["source_covs"])
        _DEVICE[key] = (tgt, src, gpu.KdTreeGPU(tgt, structure=structure))
    return _DEVICE[key]


def _factor(gpu, kind, tgt, src, tree, cutoff):
    if kind == "edge":
        return gpu.IntegratedPointToEdgeFactorGPU(0, 1, tgt, src, target_tree=tree, max_correspondence_distance=cutoff)
    if kind == "plane":
        return gpu.IntegratedPointToPlaneFactorGPU(0, 1, tgt, src, target_tree=tree, max_correspondence_distance=cutoff)
    return gpu.IntegratedLOAMFactorGPU(0, 1, tgt, tgt, src, src, target_edges_tree=tree, target_planes_tree=tree, max_correspondence_distance=cutoff)


def _report(what, L, ref, tol, path="f64 rigid sums + adjoint"):
    worst, block, errs = fd.worst_block(L, ref)
    e = abs(L.error - ref["error"]) / ref["error"] if ref["error"] else abs(L.error)
    print(f"[domain] {what}: path {path}, worst block {block} {worst:.3e} (H_source {errs['H_source']:.3e}, b_source {errs['b_source']:.3e}, H_target {errs['H_target']:.3e}), "
          f"error {e:.3e}, inliers {L.num_inliers} / {ref['num_inliers']}, asserted at {tol:.0e}")
    return worst


def _part_counts(ref):
    return [int((p.correspondences[:, 0] >= 0).sum()) for p in ref.parts]


def _check(gpu, kind, target, source, dev, delta, near, cutoff, tol, what, validation=False, path="f64 rigid sums + adjoint"):
    """one factor on the device against loam_ref at `delta`: the record, the per-part inlier counts, the error at `near` on the stored correspondences"""
    tgt, src, tree = dev
    ref = ld.make_ref(kind, target, source, cutoff)
    f = _factor(gpu, kind, tgt, src, tree, cutoff)
    if validation:
        ref.set_enable_correspondence_validation(True)
        f.set_enable_correspondence_validation(True)
    ld.conditioned(ref, delta, what, validation)
    L, Lr = f.linearize_delta(delta), ref.linearize(delta)
    _report(what, L, Lr, tol, path)
    assert_linearized_close(L, Lr, tol, what)
    counts = _part_counts(ref)
    ne, npl = f.num_correspondences()
    assert (ne, npl) == {"edge": (counts[0], 0), "plane": (0, counts[0])}.get(kind, tuple(counts)) and ne + npl == L.num_inliers, (what, ne, npl, counts)
    e, er = f.error({0: np.eye(4), 1: near}), ref.error(near)
    print(f"[domain] {what}: error at the nearby pose {abs(e - er) / er if er else abs(e):.3e}")
    assert ref.searches == 1 and abs(e - er) <= tol * max(er, 1e-300), (what, e, er)
    return f, L, Lr, ref


# ---- (a) scan to map ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cutoff", ld.CUTOFFS)
@pytest.mark.parametrize("kind", ld.KINDS)
@pytest.mark.parametrize("distance,rotation", ld.CASES_A)
def test_scan_to_map(gpu, distance, rotation, kind, cutoff):
    """(a) the target in a world frame, the source in its sensor frame; at 0.5 m between 8 % and 17 % of the points have no correspondence (asserted on the CPU)"""
    d, delta, near, _, _ = ld.case("scan_to_map", (distance, rotation))
    dev = _device(gpu, ("a", distance, rotation), d)
    _check(gpu, kind, d["target_points"], d["source_points"], dev, delta, near, cutoff, ld.tolerance(distance > 0), f"(a) loam {kind} {distance:g} m {rotation} cutoff {cutoff:g}")


# ---- (b) both clouds far, (c) units -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cutoff", ld.CUTOFFS)
@pytest.mark.parametrize("kind", ld.KINDS)
def test_both_clouds_far(gpu, kind, cutoff):
    """(b) control: source and target both 1000 m out, the relative pose near identity: nothing cancels, the project's own tolerance"""
    d, delta, near, _, _ = ld.case("both_far", ())
    _check(gpu, kind, d["target_points"], d["source_points"], _device(gpu, ("b",), d), delta, near, cutoff, ld.PARITY_TOL, f"(b) loam {kind} both far cutoff {cutoff:g}")


@pytest.mark.parametrize("kind", ld.KINDS)
@pytest.mark.parametrize("scale", fd.SCALES)
def test_units(gpu, scale, kind):
    """(c) the whole scene in centimetres, metres and hundreds of metres, the cut-off one metre in those units: the record scales as the reference's does"""
    d, delta, near, _, unit = ld.case("scaled", (scale,))
    assert unit == scale
    _check(gpu, kind, d["target_points"], d["source_points"], _device(gpu, ("c", scale), d), delta, near, scale, ld.PARITY_TOL, f"(c) loam {kind} scale {scale:g}")


# ---- (d) the correspondences themselves -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("structure", [0, HASHED], ids=["default", "hashed"])
@pytest.mark.parametrize("cutoff", ld.CUTOFFS)
@pytest.mark.parametrize("distance,rotation", [(t, r) for t in (0.0, 10000.0) for r in fd.ROTATIONS])
def test_stored_correspondences_equal_brute_force(gpu, distance, rotation, cutoff, structure):
    """(d) the int[K][n] sets read back from the device against PartRef.correspondences: the same indices in the same order, -1 in all K slots where fewer than K
    target points lie within the cut-off"""
    d, delta, _, _, _ = ld.case("scan_to_map", (distance, rotation))
    what = f"(d) {distance:g} m {rotation} cutoff {cutoff:g} structure {structure}"
    tgt, src, tree = _device(gpu, ("a", distance, rotation), d, structure)
    ref = ld.make_ref("loam", d["target_points"], d["source_points"], cutoff)
    ld.conditioned(ref, delta, what)
    ref.update_correspondences(delta)
    f = _factor(gpu, "loam", tgt, src, tree, cutoff)
    L = f.linearize_delta(delta)
    n = len(d["source_points"])
    for part, got in zip(ref.parts, f.correspondences()):
        want = part.correspondences
        none = int((want[:, 0] < 0).sum())
        wrong = np.flatnonzero((got != want).any(axis=1))
        print(f"[domain] {what} K={part.K}: {none} of {n} points without a correspondence, {len(wrong)} rows differ")
        assert got.shape == (n, part.K) and got.dtype == np.int32
        assert ((got < 0).all(axis=1) | (got >= 0).all(axis=1)).all(), "a row is neither a full correspondence nor all -1"
        assert len(wrong) == 0, (what, part.K, wrong[:5], got[wrong[:5]], want[wrong[:5]])
        assert (none >= 0.05 * n) == (cutoff == 0.5)  # at half the cut-off a large share goes through the all-or-nothing path
    assert L.num_inliers == sum(_part_counts(ref))


# ---- (e) a non-orthonormal block at a far pose ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ld.KINDS)
def test_non_orthonormal_block_at_1000m(gpu, kind):
    """(e) test_loam_gpu.py's perturbation of the 3x3 block, 1000 m out: the general kernels (92 explicit sums, J_s from the block as given), held to the gate"""
    d, delta, _, _, _ = ld.case("scan_to_map", (1000.0, "0.4rad"))
    skew = ld.non_orthonormal(delta)
    assert np.abs(skew[:3, :3].T @ skew[:3, :3] - np.eye(3)).max() > 1e-7
    d2, dropped = fd.with_margin(d, skew)
    assert dropped <= fd.DROP_CAP
    tgt, _, tree = _device(gpu, ("a", 1000.0, "0.4rad"), d)
    src = gpu.PointCloudGPU(d2["source_points"], d2["source_covs"])
    _check(gpu, kind, d2["target_points"], d2["source_points"], (tgt, src, tree), skew, skew @ fd.expmap(ld.NEARBY), 1.0, ld.GATE, f"(e) loam {kind} non-orthonormal 1000 m",
           path="explicit J_s")


# ---- (f) batch and device poses ---------------------------------------------------------------------------------------------------------------------------------------
PLACEMENTS = [(0.0, "0.4rad"), (10000.0, "pi-1e-3")]
MEMBERS = ["edge", "gicp", "plane", "loam"]  # (the GICP member between LOAM members: the record order differs from the caller's)


def test_batch_on_device_poses(gpu):
    """(f) one correspondence batch of an edge, a GICP, a plane and a combined member at each of two placements (0 m / 0.4 rad and 10 km / pi - 1e-3), its poses
    taken from the device pose table of a three-pose LM graph (pose 0 the identity, held; pose 1 and 2 the two relative poses, exact to the last bit) and once
    more through the batch's own device-pose entry point: every record bit-identical to the member's single-factor call, and within (a)'s tolerance of the reference"""
    factors, pairs, singles, refs, tols, names, deltas = [], [], [], [], [], [], []
    for slot, (t, r) in enumerate(PLACEMENTS, start=1):
        d, delta, _, _, _ = ld.case("scan_to_map", (t, r))
        tgt, src, tree = _device(gpu, ("a", t, r), d)
        for kind in MEMBERS:
            what = f"(f) {kind} {t:g} m {r}"
            if kind == "gicp":
                f = gpu.IntegratedGICPFactorGPU(0, slot, tgt, src)
                Lo = oracle.OracleGICPFactor(d["target_points"], d["target_covs"], d["source_points"], d["source_covs"], 4).linearize(delta)
                ref = {k: getattr(Lo, k) for k in FIELDS}
            else:
                f = _factor(gpu, kind, tgt, src, tree, 1.0)
                r_ = ld.make_ref(kind, d["target_points"], d["source_points"], 1.0)
                ld.conditioned(r_, delta, what)
                ref = r_.linearize(delta)
            assert ref["num_inliers"] > 2000
            factors.append(f)
            pairs.append((0, slot))
            singles.append(f.linearize_delta(delta))
            refs.append(ref)
            tols.append(ld.tolerance(t > 0))
            names.append(what)
            deltas.append(delta)
    values = np.stack([np.eye(4)] + [ld.case("scan_to_map", p)[1] for p in PLACEMENTS])
    lm = gpu.LevenbergMarquardtGraphGPU([], [], 3, fixed=(0,), corr_factors=factors, corr_pairs=pairs)
    try:
        lm.set_values(values)
        lm.linearize()
        recs = lm.records().cpu().numpy()
        order = list(lm.corr_order)
    finally:
        lm.close()
    assert sorted(order) == list(range(len(factors))) and order != list(range(len(factors)))
    batch = gpu.CorrespondenceFactorBatchGPU(factors)
    try:
        direct = batch.linearize_deltas(np.stack(deltas), corr_set=1)
    finally:
        batch.close()
    for row, k in enumerate(order):
        L = gpu.LinearizedSystem6.from_doubles(recs[row])
        _report(f"{names[k]}, graph record {row}", L, refs[k], tols[k], "batch, device poses")
        for field in FIELDS:
            assert np.array_equal(getattr(L, field), getattr(singles[k], field)), f"{names[k]}: {field} of the graph's record differs from the single-factor call"
            assert np.array_equal(getattr(direct[k], field), getattr(singles[k], field)), f"{names[k]}: {field} of the batch's record differs from the single-factor call"
        assert_linearized_close(L, refs[k], tols[k], names[k])


# ---- (g) validation on ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("distance", [0.0, 100.0, 10000.0])
def test_validation(gpu, distance):
    """(g) validate_correspondences behind the search: a mixed decision at 0 m and 100 m (the theta margin > 1e-9 rad asserted first; measured on the CPU 1.6e-6 and
    1.2e-6 rad, so 100 m needs no replacement); at 10 km every neighbour pair subtends far less than 0.1 degrees: both sides reject every correspondence and return
    an all-zero record with error 0"""
    d, delta, near, _, _ = ld.case("scan_to_map", (distance, "0.4rad"))
    dev = _device(gpu, ("a", distance, "0.4rad"), d)
    f, L, Lr, ref = _check(gpu, "loam", d["target_points"], d["source_points"], dev, delta, near, 1.0, ld.tolerance(distance > 0), f"(g) validation on, {distance:g} m",
                           validation=True)
    print(f"[domain] (g) {distance:g} m: rejected {ref.rejected}")
    for part, got in zip(ref.parts, f.correspondences()):
        assert np.array_equal(got, part.correspondences), f"K={part.K}: the validated sets differ"
    if distance == 10000.0:
        assert Lr["num_inliers"] == 0 and L.num_inliers == 0 and L.error == 0.0 and f.num_correspondences() == (0, 0)
        for k in BLOCKS:
            assert not np.any(getattr(L, k)), k
        assert f.error({0: np.eye(4), 1: near}) == 0.0
    else:
        assert min(ref.rejected) > 0 and Lr["num_inliers"] > 2000


# ---- near-degenerate neighbours ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,value,far", ld.CLUSTER_CASES, ids=[f"{'length' if K == 2 else 'sine'}-{v:g}-{'10km' if far else 'origin'}" for K, v, far in ld.CLUSTER_CASES])
def test_near_degenerate_neighbours(gpu, K, value, far):
    """257 isolated clusters of K + 1 target points with a prescribed edge length / sine of the triple, one source point beside each; the margins are asserted on what
    the f32 inputs REALISE (printed), and the case list is the one tests/test_loam_domain_ref_cpu.py::test_cluster_case_list holds to the 1e-8 rule"""
    kind = "edge" if K == 2 else "plane"
    what = f"clusters {kind} {'length' if K == 2 else 'sine'} {value:g} {'10 km' if far else 'origin'}"
    target, source, delta = ld.cluster_scene(K, value, far)
    part = loam_ref.PartRef(K, target, source, 1.0)
    part.update_correspondences(delta)
    print(f"[domain] {what}: realised {ld.realised(part, delta)}")
    tgt, src = gpu.PointCloudGPU(target), gpu.PointCloudGPU(source)
    f, L, Lr, ref = _check(gpu, kind, target, source, (tgt, src, gpu.KdTreeGPU(tgt)), delta, delta @ fd.expmap(ld.NEARBY), 1.0, ld.tolerance(far), what)
    assert L.num_inliers == ld.CLUSTERS
    got = f.correspondences()[0 if K == 2 else 1]
    assert np.array_equal(got, ref.correspondences)
    for k in FIELDS:
        assert np.isfinite(getattr(L, k)).all(), k

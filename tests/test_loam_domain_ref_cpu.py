"""Self-check of tests/loam_domain_ref.py, the inputs and statements of the LOAM factor-domain sweep (no GPU needed).

For every case tests/test_loam_domain_gpu.py runs: the input condition of test_loam_gpu.py holds (tie, cut-off and length margins > 1e-9, sine > 1e-6), the case
keeps a floor of inliers (and, at the 0.5 m cut-off, leaves at least 5 % of the points WITHOUT a correspondence), and the reference is not the weak side: the f64
cross-product statement of tests/loam_ref.py and the M-form the kernel sums, restated in np.longdouble, agree on every block and on the error to a tenth of the
tolerance the GPU test asserts (1e-8 where it asserts 1e-7, 1e-6 where it asserts the 1e-5 gate)."""
import numpy as np
import pytest

import factor_domain_ref as fd
import loam_domain_ref as ld
import loam_ref
from helpers import BLOCKS, rel_err

SWEEP = list(ld.sweep())


def test_long_double_is_wider_than_double():
    assert np.finfo(np.longdouble).eps < 1e-18, "this platform's long double is no wider than double"


def test_mform_in_f64_is_the_reference_on_a_small_cloud():
    """the M-form is the cross-product form's algebra: both in f64 on 300 random points agree to rounding, part by part and combined, record and error nearby"""
    rng = np.random.default_rng(3)
    tgt = rng.uniform(-2.0, 2.0, (400, 3)).astype(np.float32)
    src = rng.uniform(-2.0, 2.0, (300, 3)).astype(np.float32)
    delta = fd.expmap(fd.SMALL)
    for kind in ld.KINDS:
        ref = ld.make_ref(kind, tgt, src, 1.0)
        L = ref.linearize(delta)
        X = ld.mform(ref, delta, np.float64)
        assert L["num_inliers"] == X["num_inliers"] > 100
        assert max(rel_err(X[k], L[k]) for k in BLOCKS) < 1e-12 and abs(X["error"] - L["error"]) < 1e-12 * L["error"]
        near = delta @ fd.expmap(ld.NEARBY)
        assert abs(ld.mform(ref, near, np.float64)["error"] - ref.error(near)) < 1e-12 * ref.error(near)
    # M of the edge term is the full rank-2 projector the kernel sums: off-diagonals live, trace 2
    part = loam_ref.EdgeFactorRef(tgt, src, 1.0)
    part.update_correspondences(delta)
    c = part.correspondences[part.correspondences[:, 0] >= 0]
    v = part.target[c[:, 0]] - part.target[c[:, 1]]
    M = np.eye(3)[None] - v[:, :, None] * v[:, None, :] / (v * v).sum(1)[:, None, None]
    assert np.allclose(np.trace(M, axis1=1, axis2=2), 2.0) and np.abs(M[:, 0, 1]).max() > 0.1 and np.allclose(np.einsum("nij,nj->ni", M, v), 0.0, atol=1e-12)


@pytest.mark.parametrize("name,maker,args,cutoff,far", SWEEP, ids=[s[0] for s in SWEEP])
def test_sweep_case(name, maker, args, cutoff, far):
    d, delta, near, dropped, unit = ld.case(maker, args)
    n = len(d["source_points"])
    assert dropped <= fd.DROP_CAP and n >= (1.0 - fd.DROP_CAP) * fd.N_SOURCE
    tenth = 0.1 * ld.tolerance(far)
    figures = []
    for kind in ld.KINDS:
        ref = ld.make_ref(kind, d["target_points"], d["source_points"], cutoff)
        ld.conditioned(ref, delta, f"{name} {kind}")
        L = ref.linearize(delta)
        counts = [int((p.correspondences[:, 0] >= 0).sum()) for p in ref.parts]
        if cutoff == unit:
            assert all(c >= 0.99 * n for c in counts), (name, kind, counts, n)
        else:  # half the cut-off: the all-or-nothing -1 path, for a large share of the points
            assert all(0.75 * n <= c <= 0.95 * n for c in counts), (name, kind, counts, n)
        X = ld.mform(ref, delta)
        assert X["num_inliers"] == L["num_inliers"] == sum(counts)
        worst, e = ld.agreement(L, X)
        en = float(abs(np.longdouble(ref.error(near)) - ld.mform(ref, near)["error"]) / ld.mform(ref, near)["error"])
        figures.append((kind, counts, worst, e, en))
        print(f"[loam domain ref] {name} {kind}: inliers {counts} of {n}, f64 cross-product form vs long-double M-form: worst block {worst:.2e}, error {e:.2e}, error nearby {en:.2e}"
              f" (a tenth of the asserted tolerance: {tenth:.0e})")
        assert worst <= tenth and e <= tenth and en <= tenth, (name, kind, worst, e, en)


@pytest.mark.parametrize("distance", [0.0, 100.0, 10000.0])
def test_validation_cases(distance):
    """case (g): the theta margin > 1e-9 rad at 0 m and 100 m (a mixed decision: some pairs rejected, some kept); at 10 km every neighbour pair subtends far less
    than 0.1 degrees, every correspondence is rejected and the reference's record is all zero"""
    d, delta, near, _, _ = ld.case("scan_to_map", (distance, "0.4rad"))
    ref = ld.make_ref("loam", d["target_points"], d["source_points"], 1.0)
    ref.set_enable_correspondence_validation(True)
    lows = ld.conditioned(ref, delta, f"validation {distance:g} m", validation=True)
    L = ref.linearize(delta)
    print(f"[loam domain ref] validation {distance:g} m: rejected {ref.rejected}, {L['num_inliers']} inliers, theta margins {lows[2]['theta']:.2e} / {lows[3]['theta']:.2e} rad")
    if distance == 10000.0:
        assert L["num_inliers"] == 0 and L["error"] == 0.0 and not any(np.any(L[k]) for k in BLOCKS) and ref.error(near) == 0.0
    else:
        assert min(ref.rejected) > 0 and L["num_inliers"] > 2000
        worst, e = ld.agreement(L, ld.mform(ref, delta))
        assert worst <= 0.1 * ld.tolerance(distance > 0) and e <= 0.1 * ld.tolerance(distance > 0)


def test_non_orthonormal_case():
    """case (e): test_loam_gpu.py's perturbed block at 1000 m -- conditioned, and the M-form (J_s from the block as given) agrees with the reference"""
    d, delta, _, _, _ = ld.case("scan_to_map", (1000.0, "0.4rad"))
    skew = ld.non_orthonormal(delta)
    assert np.abs(skew[:3, :3].T @ skew[:3, :3] - np.eye(3)).max() > 1e-7
    d2, dropped = fd.with_margin(d, skew)
    assert dropped <= fd.DROP_CAP
    for kind in ld.KINDS:
        ref = ld.make_ref(kind, d2["target_points"], d2["source_points"], 1.0)
        ld.conditioned(ref, skew, f"non-orthonormal 1000 m {kind}")
        worst, e = ld.agreement(ref.linearize(skew), ld.mform(ref, skew))
        print(f"[loam domain ref] non-orthonormal 1000 m {kind}: worst block {worst:.2e}, error {e:.2e}")
        assert worst <= 0.1 * ld.GATE and e <= 0.1 * ld.GATE


def test_cluster_scene_shape():
    for K, value in ((2, 1e-2), (3, 1e-3)):
        tgt, src, delta = ld.cluster_scene(K, value, False)
        assert tgt.shape == (ld.CLUSTERS * (K + 1), 3) and src.shape == (ld.CLUSTERS, 3) and tgt.dtype == np.float32 and ld.CLUSTERS == 256 + 1
        part = loam_ref.PartRef(K, tgt, src, 1.0)
        part.update_correspondences(delta)
        c = part.correspondences
        assert (c >= 0).all() and len(np.unique(c)) == ld.CLUSTERS * K  # every cluster serves its own source point, with K of its K + 1 points
        r = ld.realised(part, delta)
        if K == 2:
            assert abs(r["length"][0] - value) < 1e-5 * value + 2e-7 and abs(r["length"][1] - value) < 1e-5 * value + 2e-7
        else:
            assert 0.9 * value < r["sine"][0] <= r["sine"][1] < 1.1 * value
        far_t, _, far_d = ld.cluster_scene(K, value, True)
        assert np.allclose(far_d[:3, 3] - delta[:3, 3], ld.FAR * fd.DIRECTION) and np.abs(far_t).max() < 8192.0


def test_cluster_case_list():
    """Every prescribed case of section 3, measured here: the smallest margins and the realised geometry of the f32 inputs, and how far the f64 cross-product
    reference is from the long-double M-form.  A case is in loam_domain_ref.CLUSTER_CASES exactly when its input condition holds on the realised values and that
    figure is <= 1e-8; the list must reach a sine of 1e-4 and a length of 1e-2 m at the origin.

    Measured (f64 against long double: worst block | error; realised smallest .. largest; smallest tie margin where it is small):
      origin  length 1       1.8e-15 | 1.3e-15   1.000 .. 1.000 m
              length 1e-2    7.6e-16 | 4.1e-14   1.000e-2 .. 1.000e-2 m            tie 2.8e-4
              length 1e-4    3.0e-15 | 1.7e-14   9.999e-5 .. 1.000e-4 m            tie 1.9e-9
              sine 1e-1 .. 1e-5   4.0e-15 .. 4.6e-15 | 1.7e-15 .. 1.9e-15   each within 0.4 % of the prescribed value (1e-5: 9.964e-6 .. 1.005e-5)
      10 km   length 1       2.4e-13 | 1.6e-13   0.9997 .. 1.000 m
              length 1e-2    2.1e-13 | 8.4e-14   9.667e-3 .. 1.027e-2 m            tie 4.6e-6
              length 1e-4    out: x_j and x_l round to the same f32 point (length 0, a tie)
              sine 1e-1      7.3e-13 | 2.3e-13   9.932e-2 .. 1.007e-1
              sine 1e-2      7.3e-13 | 2.2e-13   9.327e-3 .. 1.066e-2
              sine 1e-3      1.1e-12 | 2.9e-13   9.387e-4 .. 1.540e-3
              sine 1e-4, 1e-5   out: the 0.5 mm f32 grid makes every triple exactly collinear (sine 0)
    No case is out by the 1e-8 rule; the three that are out cannot state their input condition."""
    kept = []
    for far in (False, True):
        for K, values in ((2, ld.LENGTHS), (3, ld.SINES)):
            for value in values:
                f = ld.cluster_figure(K, value, far)
                what = "length" if K == 2 else "sine"
                r = f["realised"].get(what, (np.nan, np.nan))
                print(f"[loam domain ref] clusters K={K} {what} {value:g} {'10 km' if far else 'origin'}: condition {'holds' if f['ok'] else 'FAILS'}, margins {f['margins']}, "
                      f"realised {what} {r[0]:.3e} .. {r[1]:.3e}, f64 vs long double: worst block {f['worst']:.2e}, error {f['error']:.2e}")
                if f["ok"] and f["worst"] <= 1e-8 and f["error"] <= 1e-8:
                    kept.append((K, value, far))
    assert kept == ld.CLUSTER_CASES, kept
    assert (3, 1e-4, False) in kept and (2, 1e-2, False) in kept

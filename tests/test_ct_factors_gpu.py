"""GPU tests of IntegratedCTICPFactorGPU / IntegratedCTGICPFactorGPU (gp_ct_factor_*, csrc/gp_ct_factors.hip) against tests/ct_ref.py, the numpy f64 restatement of
impl/integrated_ct_icp_factor_impl.hpp and impl/integrated_ct_gicp_factor_impl.hpp.

Fixtures.  ct_ref.skewed_scan: the synthetic walls as the target (6,000 points, their normals, covariances from the normals) and a second cast of them, skewed
with known (T0, T1), as the source.  tests/test_ct_ref_cpu.py asserts for every search compared here that no query sits on a tie or on the cut-off (margins
> 1e-9), so the device search and the brute-force search must pick the same target for every point: the comparisons of correspondences are exact.

Pose table.  The bound is computed here, on the CPU: the restatement evaluated in float64 and in np.longdouble over the sweep (rotation angle of T0^-1 T1 in
{0, 1e-12, 1e-8, 1e-5, 1e-3, 0.1, 1, 2} rad, translations of 0.01 and 100), the device is given 16x their largest entry-wise difference but not less than 2^-40, both
relative to the largest entry of the block -- T, D0 or D1 over all bins of a pose pair (D0(1) and D1(0) are zero blocks, so a bin has no scale of its own).
Measured on the CPU: float64 against long double differs by at most 5.3e-15 of the block's largest entry, 16x that is 8.5e-14, so the 2^-40 = 9.1e-13 floor is
the bound; the header's functions compiled for the host differ from long double by 4.9e-15.

Records.  Entry-wise 1e-7 of the block's largest magnitude, the bound of the project's other f64 record tests, against the restatement evaluated on the device's
own correspondences.  One block can be exactly zero -- H_01 when every bin sits at t = 0 or t = 1 -- and is then held to one f64 ulp of sqrt(|H_00| |H_11|)
instead (assert_record).

End to end.  T1 after six damped Gauss-Newton steps on device records against the same steps on restatement records: measured 1.7e-16, bound 16x that
(END_TO_END_TOL, test_end_to_end)."""
import numpy as np
import pytest

import ct_ref
from helpers import BLOCKS, expmap, pose_error
from test_ct_ref_cpu import A0, A1, LAYOUTS, POSE_PAIRS, SIZES, T0, T1, bin_layout, fixture, make_ref, one_match_cutoff

pytestmark = pytest.mark.gpu
RECORD_TOL = 1e-7
END_TO_END_TOL = 16 * 1.665e-16  # 16x the larger of the two measured differences (test_end_to_end)


@pytest.fixture(scope="module")
def target(gpu):
    fx = fixture(8)
    tgt = gpu.PointCloudGPU(fx["target_points"], covs=fx["target_covs"], normals=fx["target_normals"])
    return dict(tgt=tgt, tree=gpu.KdTreeGPU(tgt))


_FIXTURES = {}


def shared_fixture(n, layout="eight"):
    if (n, layout) not in _FIXTURES:
        _FIXTURES[(n, layout)] = fixture(n, layout)
    return _FIXTURES[(n, layout)]


def make_factor(gpu, target, fx, kind, cutoff=1.0, times=None):
    src = gpu.PointCloudGPU(fx["points"], covs=fx["covs"])
    src.add_times(fx["times"] if times is None else times)
    cls = gpu.IntegratedCTGICPFactorGPU if kind else gpu.IntegratedCTICPFactorGPU
    return cls(0, 1, target["tgt"], src, target_tree=target["tree"], max_correspondence_distance=cutoff)


def blocks_of(hf):
    """the record's blocks out of the HessianFactor (g = -b)"""
    return {"H_target": hf.G[(0, 0)], "H_target_source": hf.G[(0, 1)], "H_source": hf.G[(1, 1)], "b_target": -hf.g[0], "b_source": -hf.g[1], "error": hf.f}


def assert_record(got, want, what):
    # H_01 = sum H_0^T M H_1 is EXACTLY zero when every bin sits at t = 0 or t = 1 (D1(0) = 0, D0(1) = 0: the two-bin layouts): both sides then hold rounding
    # residue of sums whose terms are as large as sqrt(|H_00| |H_11|) (Cauchy-Schwarz), and a block without a value has no magnitude to be relative to.  No f64
    # sum resolves below one ulp of its terms, so that block's bound is not taken below 2^-52 of that scale; every other block, and H_01 whenever it has a
    # value, is held to RECORD_TOL of its own largest entry.
    floor = 2.0**-52 * np.sqrt(np.abs(want["H_target"]).max() * np.abs(want["H_source"]).max())
    for k in BLOCKS:
        scale = np.abs(want[k]).max()
        diff = np.abs(got[k] - want[k]).max()
        print(f"[ct] {what} {k}: {diff / max(scale, 1e-300):.2e} of the block's largest entry")
        assert diff <= max(RECORD_TOL * scale, floor if k == "H_target_source" else 0.0), (what, k, diff, scale)
    assert abs(got["error"] - want["error"]) <= RECORD_TOL * abs(want["error"]), what


def check_case(gpu, target, n, layout, pair, kind, cutoff=1.0):
    fx = shared_fixture(n, layout)
    P0, P1 = POSE_PAIRS[pair]
    f = make_factor(gpu, target, fx, kind, cutoff)
    ref = make_ref(kind, fx, cutoff)
    hf = f.linearize({0: P0, 1: P1})
    corr = f.correspondences()
    brute = ref.update_correspondences(P0, P1)
    assert np.array_equal(corr, brute), (n, layout, pair, int((corr != brute).sum()))
    want = ref.linearize(P0, P1, corr)
    assert f.num_inliers() == want["num_inliers"] == int((corr >= 0).sum())
    if want["num_inliers"]:
        assert_record(blocks_of(hf), want, f"n {n} {layout} {pair} kind {kind}")
    return f, ref, hf, want


# ---- time table --------------------------------------------------------------------------------------------------------------------------------------------------


def test_time_table_and_indices_equal_the_restatement(gpu, target):
    rng = np.random.default_rng(5)
    fx = shared_fixture(257)
    above = np.float32(1e-3)
    cases = {
        "layout": fx["times"],
        "equal": np.full(257, 0.25, np.float32),
        "unsorted": rng.uniform(0.0, 0.1, 257).astype(np.float32),
        "offset": (10.0 + 0.01 * (np.arange(257) // 40)).astype(np.float32),
        "last zero": np.linspace(-0.5, 0.0, 257).astype(np.float32),
        "threshold": np.where(np.arange(257) < 100, 0.0, np.where(np.arange(257) < 200, np.nextafter(above, np.float32(0)), above + above)).astype(np.float32),
    }
    for name, times in cases.items():
        f = make_factor(gpu, target, fx, 0, times=times)
        table, idx = f.time_table()
        want_table, want_idx = ct_ref.time_table(times)
        assert np.array_equal(table, want_table) and np.array_equal(idx, want_idx), name
    assert len(ct_ref.time_table(cases["threshold"])[0]) == 2 and len(ct_ref.time_table(cases["equal"])[0]) == 1


# ---- pose table --------------------------------------------------------------------------------------------------------------------------------------------------


def test_pose_table_against_the_restatement(gpu, target):
    """measured (CPU): float64 vs long double 5.3e-15 of the block's largest entry over the sweep -> 16x = 8.5e-14 < 2^-40: the bound is 2^-40 = 9.1e-13; the device
    (one MI355X) differs from long double by 5.3e-15"""
    rng = np.random.default_rng(3)
    fx = shared_fixture(257)
    f = make_factor(gpu, target, fx, 0)
    table, _ = f.time_table()
    cases, own = [], 0.0
    for angle in (0.0, 1e-12, 1e-8, 1e-5, 1e-3, 0.1, 1.0, 2.0):
        for trans in (0.01, 100.0):
            axis = rng.normal(size=3)
            axis /= np.linalg.norm(axis)
            P0 = expmap(np.concatenate([0.5 * rng.normal(size=3), trans * rng.normal(size=3)]))
            P1 = P0 @ expmap(np.concatenate([angle * axis, trans * rng.normal(size=3)]))
            exact = ct_ref.pose_table(P0, P1, table, np.longdouble)
            for a, b in zip(ct_ref.pose_table(P0, P1, table), exact):
                own = max(own, float(np.abs(a.astype(np.longdouble) - b).max() / np.abs(b).max()))
            cases.append((angle, trans, P0, P1, exact))
    bound = max(16.0 * own, 2.0**-40)
    print(f"[ct] pose table: float64 vs long double {own:.2e}, bound {bound:.2e}")
    worst = 0.0
    for angle, trans, P0, P1, exact in cases:
        f.linearize({0: P0, 1: P1})
        for name, got, want in zip(("T", "D0", "D1"), f.pose_table(), exact):
            want = want[:, :3, :] if name == "T" else want
            err = float(np.abs(got.astype(np.longdouble) - want).max() / np.abs(want).max())
            worst = max(worst, err)
            assert err <= bound, (angle, trans, name, err, bound)
        T = f.pose_table()[0]
        assert np.abs(np.einsum("bij,bkj->bik", T[:, :, :3], T[:, :, :3]) - np.eye(3)).max() < 1e-14
    print(f"[ct] pose table: device vs long double {worst:.2e}")
    # the ends: D0(0) = I, D1(0) = 0, D0(1) = 0, D1(1) = I (table[0] is 0 and table[-1] is 1 in this layout)
    assert table[0] == 0.0 and table[-1] == 1.0
    f.linearize({0: A0, 1: A1})
    _, D0, D1 = f.pose_table()
    assert np.abs(D0[0] - np.eye(6)).max() < 1e-14 and np.abs(D1[0]).max() == 0.0 and np.abs(D0[-1]).max() < 1e-13 and np.abs(D1[-1] - np.eye(6)).max() < 1e-13


# ---- correspondences and records -------------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_records_at_the_lane_wave_and_tile_edges(gpu, target, n, kind):
    check_case(gpu, target, n, "eight", "moving", kind)


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_records_over_the_bin_layouts(gpu, target, layout, kind):
    f, _, _, _ = check_case(gpu, target, 2049, layout, "moving", kind)
    assert np.array_equal(f.time_table()[1], bin_layout(layout, 2049))


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("pair,n", [("still", 2049), ("far", 600)])
def test_records_at_zero_velocity_and_at_a_large_motion(gpu, target, pair, n, kind):
    _, _, _, want = check_case(gpu, target, n, "eight", pair, kind)
    assert want["num_inliers"] > 20


@pytest.mark.parametrize("kind", [0, 1])
def test_cutoffs_that_leave_one_point_and_none(gpu, target, kind):
    fx = shared_fixture(2049)
    cutoff = one_match_cutoff(make_ref(kind, fx), A0, A1)
    _, _, _, want = check_case(gpu, target, 2049, "eight", "moving", kind, cutoff)
    assert want["num_inliers"] == 1
    f, _, hf, want = check_case(gpu, target, 2049, "eight", "moving", kind, 1e-6)
    assert want["num_inliers"] == 0 and f.num_inliers() == 0 and hf.f == 0.0
    assert not any(np.any(b) for b in hf.G.values()) and not any(np.any(g) for g in hf.g)
    assert f.error({0: A0, 1: A1}) == 0.0


@pytest.mark.parametrize("kind", [0, 1])
def test_empty_source_gives_a_zero_record(gpu, target, kind):
    """num_points == 0 at the C interface, as the ICP factor takes it: live pointers, no point behind them"""
    import ctypes as C

    from gtsam_points_amd import _capi
    from gtsam_points_amd.types import _pose16

    lib, tgt = _capi.load(), target["tgt"]
    pts, nrm, cov = tgt.ptr(tgt.points_gpu), tgt.ptr(tgt.normals_gpu), tgt.ptr(tgt.covs_gpu)
    h = C.c_void_p()
    _capi.check(lib.gp_ct_factor_create(target["tree"]._h, pts, nrm, cov, tgt.size(), pts, cov, pts, 0, 1.0, kind, None, C.byref(h)), "gp_ct_factor_create")
    try:
        rec, err = _capi.Linearized6(), C.c_double(-1.0)
        _capi.check(lib.gp_ct_factor_linearize(h, _pose16(A0), _pose16(A1), C.byref(rec)), "gp_ct_factor_linearize")
        _capi.check(lib.gp_ct_factor_compute_error(h, _pose16(A0), _pose16(A1), C.byref(err)), "gp_ct_factor_compute_error")
        assert not np.frombuffer(rec, dtype=np.float64).any() and err.value == 0.0 and lib.gp_ct_factor_num_time_bins(h) == 0
    finally:
        lib.gp_ct_factor_destroy(h)


# ---- error -------------------------------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind", [0, 1])
def test_error_on_stored_correspondences(gpu, target, kind):
    f, ref, hf, want = check_case(gpu, target, 2049, "eight", "moving", kind)
    values = {0: A0, 1: A1}
    e = f.error(values)
    assert abs(e - hf.f) <= 1e-12 * hf.f  # (the error pass sums e^2 alone, the linearise 92 sums: the same terms in the same order)
    other = {0: T0 @ expmap([0.001, 0.002, -0.001, 0.01, 0.0, 0.02]), 1: T1}
    got, expect = f.error(other), ref.error(other[0], other[1])  # the stored correspondences, and for GICP the stored M
    assert np.array_equal(f.correspondences(), ref.corr)
    assert abs(got - expect) <= RECORD_TOL * expect and abs(got - e) > 1e-3 * e
    if kind == 1:  # M of the poses in hand would give another value
        fresh = make_ref(1, shared_fixture(2049))
        fresh.update_correspondences(other[0], other[1], ref.corr)
        assert abs(fresh.error(other[0], other[1]) - expect) > 1e-6 * expect


@pytest.mark.parametrize("kind", [0, 1])
def test_error_before_any_linearise_searches_at_its_poses(gpu, target, kind):
    fx = shared_fixture(1025)
    f, ref = make_factor(gpu, target, fx, kind), make_ref(kind, fx)
    with pytest.raises(gpu.GPError, match="gp_ct_factor_correspondences"):
        f.correspondences()
    got, expect = f.error({0: A0, 1: A1}), ref.error(A0, A1)
    assert np.array_equal(f.correspondences(), ref.corr) and ref.searches == 1
    assert abs(got - expect) <= RECORD_TOL * expect
    got, expect = f.error({0: T0, 1: T1}), ref.error(T0, T1)  # now they are stored: no search at the new poses
    assert np.array_equal(f.correspondences(), ref.corr) and ref.searches == 1
    assert abs(got - expect) <= RECORD_TOL * expect


# ---- determinism, deskew, refusals -------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind", [0, 1])
def test_two_linearises_are_bit_identical(gpu, target, kind):
    f = make_factor(gpu, target, shared_fixture(2049, "own"), kind)
    a = blocks_of(f.linearize({0: A0, 1: A1}))
    f.linearize({0: T0, 1: T1})
    b = blocks_of(f.linearize({0: A0, 1: A1}))
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("local", [False, True])
def test_deskewed_points(gpu, target, local):
    fx = shared_fixture(1025)
    f, ref = make_factor(gpu, target, fx, 0), make_ref(0, fx)
    got, want = f.deskewed_source_points({0: A0, 1: A1}, local=local), ref.deskewed(A0, A1, local=local)
    assert got.shape == (1025, 4) and got.dtype == np.float64 and (got[:, 3] == 1.0).all()
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_missing_attributes_are_refused(gpu, target):
    fx = shared_fixture(257)
    src = gpu.PointCloudGPU(fx["points"], covs=fx["covs"])
    with pytest.raises(gpu.GPError, match="source frame doesn't have required attributes for ct_icp"):
        gpu.IntegratedCTICPFactorGPU(0, 1, target["tgt"], src, target_tree=target["tree"])
    with pytest.raises(gpu.GPError, match="source frame doesn't have required attributes for ct_icp"):
        gpu.IntegratedCTGICPFactorGPU(0, 1, target["tgt"], src, target_tree=target["tree"])
    src.add_times(fx["times"])
    bare = gpu.PointCloudGPU(fx["target_points"])
    with pytest.raises(gpu.GPError, match="target cloud doesn't have normals"):
        gpu.IntegratedCTICPFactorGPU(0, 1, bare, src)
    with pytest.raises(gpu.GPError, match="target frame doesn't have required attributes for ct_gicp"):
        gpu.IntegratedCTGICPFactorGPU(0, 1, bare, src)
    timed = gpu.PointCloudGPU(fx["points"])
    timed.add_times(fx["times"])
    with pytest.raises(gpu.GPError, match="source frame doesn't have required attributes for ct_gicp"):
        gpu.IntegratedCTGICPFactorGPU(0, 1, target["tgt"], timed, target_tree=target["tree"])


# ---- end to end --------------------------------------------------------------------------------------------------------------------------------------------------


def gauss_newton(linearize, P0, P1, steps=6, prior=1e8, damping=1e-6):
    """`steps` damped Gauss-Newton steps on the 12x12 system with T0 held by a strong prior: (H + damping diag(H)) dx = -b, poses retracted from the right"""
    anchor = P0.copy()
    for _ in range(steps):
        H, b = ct_ref.system12(linearize(P0, P1))
        H[:6, :6] += prior * np.eye(6)
        b[:6] += prior * ct_ref.logmap(ct_ref.inverse(anchor) @ P0)
        dx = np.linalg.solve(H + damping * np.diag(np.diag(H)), -b)
        P0, P1 = P0 @ expmap(dx[:6]), P1 @ expmap(dx[6:])
    return P0, P1


@pytest.mark.parametrize("kind", [0, 1])
def test_end_to_end(gpu, target, kind):
    """a scan skewed by (T0, T1), T0 held, T1 started 3 cm / 0.3 degrees off: six steps on device records and on restatement records.
    Measured on an MI355X: the two final T1 differ entry-wise by at most 1.665e-16 (CT-ICP) and 1.110e-16 (CT-GICP); the bound END_TO_END_TOL is 16x the larger,
    2.7e-15.  Both runs end 6e-6 rad from the truth, 0.25 mm (CT-ICP) / 0.05 mm (CT-GICP), from a start 7e-3 rad and 37 mm off."""
    fx = shared_fixture(2049)
    f, ref = make_factor(gpu, target, fx, kind), make_ref(kind, fx)
    start = T1 @ expmap([0.004, -0.003, 0.005, 0.02, -0.03, 0.01])
    same = []

    def on_device(P0, P1):
        return blocks_of(f.linearize({0: P0, 1: P1}))

    def on_host(P0, P1):
        L = ref.linearize(P0, P1)
        same.append(np.array_equal(ref.corr, dev_corr.pop(0)))
        return L

    dev_corr = []

    def on_device_keep(P0, P1):
        L = on_device(P0, P1)
        dev_corr.append(f.correspondences())
        return L

    _, dev = gauss_newton(on_device_keep, T0.copy(), start.copy())
    _, host = gauss_newton(on_host, T0.copy(), start.copy())
    assert len(same) == 6 and all(same)  # both trajectories kept the same correspondences at every iteration
    diff = float(np.abs(dev - host).max())
    print(f"[ct] end to end kind {kind}: final T1 differ by {diff:.3e}")
    assert diff <= END_TO_END_TOL
    before, after = pose_error(start, T1), pose_error(dev, T1)
    print(f"[ct] end to end kind {kind}: start {before}, end {after}")
    assert after[0] < before[0] and after[1] < before[1]

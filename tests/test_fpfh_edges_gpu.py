"""FPFH on the device at the walk's and the grid's edges (gp_fpfh.hip) against tests/fpfh_ref.py: the strict radius on a lattice that ties exactly, the cap inside a
cell's second and third batch of 64, hundreds of neighbours per lane of the FPFH sum, the cell clamp on both signs, probes across the end of the hash table,
coordinates near 1e5 m, duplicated, infinite and huge points, zero normals, and the C entry's corners.  tests/test_fpfh_ref_cpu.py certifies every cloud used here
by the restatement alone (settled shares, ties, clamp and wrap counts).  Integer results are compared exactly -- on the exact clouds the neighbour counts of every
finite point --, settled FPFH rows entry-wise within fpfh_ref.fpfh_tolerance(n), zero entries zero and NaN rows NaN on both sides."""
import ctypes as C

import numpy as np
import pytest

import fpfh_ref as R

pytestmark = pytest.mark.gpu
CASES = tuple((name, cap) for name in R.EDGE_CLOUDS for cap in R.EDGE_CAPS[name])


@pytest.fixture(scope="module")
def gpa():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import gtsam_points_amd

    return gtsam_points_amd


def _frame(gpa, points, normals):
    return gpa.PointCloudGPU(np.ascontiguousarray(points), normals=np.ascontiguousarray(normals))


def _host(result):
    return tuple(t.cpu().numpy() if hasattr(t, "cpu") else t for t in result)


def _run(gpa, cloud, cap, **kw):
    import torch

    p, n, radius = cloud
    return gpa.estimate_fpfh_gpu(_frame(gpa, p, n), gpa.FPFHEstimationParams(radius, cap), dtype=torch.float64, return_spfh=True, **kw)


@pytest.fixture(scope="module")
def runs(gpa):
    """(fpfh, spfh, num, cut) of every edge cloud under every cap of its list: one call each, never modified"""
    return {(name, cap): _host(_run(gpa, R.edge_cloud(name), cap)) for name, cap in CASES}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.mark.parametrize("name,cap", CASES)
def test_counts_histograms_and_truncation_are_the_references(runs, name, cap):
    ref = R.edge_ref(name, cap)
    fpfh, spfh, num, cut = runs[(name, cap)]
    s = ref.settled
    assert s.mean() >= 0.99
    if name in R.EXACT_CLOUDS:
        assert np.array_equal(num[ref.finite], ref.n[ref.finite])  # exact d2 and r * r: every finite point, no exemption; a tie partner is not counted
    assert np.array_equal(num[s], ref.n[s])
    assert cut == ref.num_truncated
    counts = np.rint(spfh * (np.maximum(num - 1, 0) / 100.0)[:, None]).astype(np.int64)
    assert np.array_equal(counts[s], ref.hist[s])
    assert np.array_equal(_bits(spfh[s]), _bits(ref.spfh[s]))  # the stored value is the reference's f64 product (:245-246), to the bit
    assert not spfh[num <= 1].any() and not fpfh[num <= 1].any()


@pytest.mark.parametrize("name,cap", CASES)
def test_settled_rows_are_within_the_derived_bound(runs, name, cap):
    ref = R.edge_ref(name, cap)
    fpfh = runs[(name, cap)][0]
    rows = np.nonzero(ref.row_settled)[0]
    assert len(rows) >= 0.99 * len(ref.n)
    worst = 0.0
    for i in rows:
        want, got = ref.fpfh[i], fpfh[i]
        if np.isnan(want).any():
            assert np.isnan(want).all() and np.isnan(got).all(), i
            continue
        zero = want == 0.0
        assert np.array_equal(got[zero], want[zero]), i
        rel = np.abs(got[~zero] - want[~zero]) / np.abs(want[~zero])
        if rel.size:
            worst = max(worst, float(rel.max() / R.fpfh_tolerance(ref.n[i])))
            assert (rel <= R.fpfh_tolerance(ref.n[i])).all(), (i, rel.max(), R.fpfh_tolerance(ref.n[i]))
    print(f"{name} cap {cap}: worst entry at {worst:.4f} of the bound, n up to {int(ref.n.max())}")


def test_a_candidate_at_exactly_the_radius_is_outside(runs):
    p, _, radius = R.edge_cloud("lattice384")
    ref = R.edge_ref("lattice384")
    num = runs[("lattice384", 10000)][2]
    ties = R.exact_ties(p, radius)
    assert len(ties) == 5472
    tied = np.unique(ties[:, 0])
    assert len(tied) == 384  # every point has a partner at d2 == r * r
    assert np.array_equal(num[tied], ref.n[tied])  # ... and the partner is not counted: the restatement's strict rule leaves it out
    assert all(j not in ref.neighbors[i].tolist() for i, j in ties)


def test_cap_one_and_two_on_the_dense_cloud(runs):
    fpfh, spfh, num, cut = runs[("dense1500", 1)]
    assert (num == 1).all() and cut == 1500 and not spfh.any() and not fpfh.any()
    fpfh, spfh, num, cut = runs[("dense1500", 2)]
    ref = R.edge_ref("dense1500", 2)
    assert (num == 2).all() and cut == 1500
    # two accepted points: one pair where the query is one of them, two where it is not -- three single 100s or three blocks that sum to 200
    own = np.array([k in js.tolist() for k, js in enumerate(ref.neighbors)])
    assert own.any() and (~own).any()
    assert np.array_equal(spfh.reshape(1500, 3, 11).sum(axis=2), np.where(own, 100.0, 200.0)[:, None].repeat(3, axis=1))


def test_points_that_are_infinite_or_huge(runs):
    fpfh, spfh, num, _ = runs[("dirty300", 10000)]
    ref = R.edge_ref("dirty300")
    d = R.DIRTY
    for i in (d["nan_point"], d["pos_inf"], d["neg_inf"]):
        assert num[i] == 0 and not spfh[i].any() and not fpfh[i].any()
    assert num[d["huge"]] == 1 and not spfh[d["huge"]].any() and not fpfh[d["huge"]].any()
    # none of them is anybody's neighbour: the counts of every other point are the restatement's, which leaves them out
    assert ref.settled.all() and np.array_equal(num, ref.n)


def test_duplicated_points_and_zero_normals(runs):
    fpfh, spfh, num, _ = runs[("dirty300", 10000)]
    ref = R.edge_ref("dirty300")
    for s, copies in R.dirty_copies().items():
        for i in [s] + copies:
            assert ref.settled[i] and ref.row_settled[i]
            assert num[i] == ref.n[i] and np.array_equal(_bits(spfh[i]), _bits(ref.spfh[i]))
            assert spfh[i][5] * (num[i] - 1) / 100.0 >= len(copies) - 1e-9  # the coincident pairs land in bin 5
            assert np.isfinite(fpfh[i]).all() and fpfh[i].any()  # their zero distance is skipped, not divided by
    for i in R.DIRTY["zero_normals"]:
        assert ref.settled[i] and num[i] == ref.n[i] > 1 and np.array_equal(_bits(spfh[i]), _bits(ref.spfh[i]))
        for j in ref.neighbors[i]:
            assert np.array_equal(_bits(spfh[j]), _bits(ref.spfh[j]))  # the pairs that see the zero normal as n2: atan2 of signed zeros


def test_indices_naming_dirty_points_give_the_full_calls_rows(gpa, runs):
    import torch

    copies = R.dirty_copies()
    s = R.DIRTY["sources"][2]
    idx = np.array([R.DIRTY["nan_point"], R.DIRTY["pos_inf"], s, copies[s][0], R.DIRTY["neg_inf"], R.DIRTY["huge"], copies[s][-1], R.DIRTY["zero_normals"][0]], np.int32)
    p, n, radius = R.edge_cloud("dirty300")
    sub = gpa.estimate_fpfh_gpu(_frame(gpa, p, n), gpa.FPFHEstimationParams(radius, 10000), indices=idx, dtype=torch.float64)
    assert tuple(sub.shape) == (len(idx), 33)
    assert np.array_equal(_bits(sub.cpu().numpy()), _bits(runs[("dirty300", 10000)][0][idx]))


def test_the_largest_cap_gives_the_bits_of_the_default(gpa):
    cloud = R.cloud("random600")
    a, b = _host(_run(gpa, cloud, 10000)), _host(_run(gpa, cloud, 2**31 - 1))
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))
    assert np.array_equal(a[2], b[2]) and a[3] == b[3] == 0


def _c_call(gpa, frame, radius, cap, n, rows, idx=None, f64=False, f32=False, spfh=False):
    """gp_estimate_fpfh as a C caller reaches it: -> (fpfh f64, fpfh f32, spfh, num, cut), each requested output as a host array, the others None"""
    import torch

    dev = frame.device
    out64 = torch.full((rows, 33), -1.0, dtype=torch.float64, device=dev) if f64 else None
    out32 = torch.full((rows, 33), -1.0, dtype=torch.float32, device=dev) if f32 else None
    sp = torch.full((n, 33), -1.0, dtype=torch.float64, device=dev) if spfh else None
    num = torch.full((n,), -1, dtype=torch.int32, device=dev)
    ix = torch.as_tensor(idx, dtype=torch.int32).to(dev) if idx is not None else None
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    cut = C.c_int(-1)
    cp = gpa._capi.FpfhParams(float(radius), int(cap))
    torch.cuda.synchronize()
    gpa._capi.check(gpa._capi.load().gp_estimate_fpfh(frame.ptr(frame.points_gpu), frame.ptr(frame.normals_gpu), n, C.byref(cp), ptr(ix), 0 if idx is None else len(idx),
                                                      ptr(out64), ptr(out32), ptr(sp), ptr(num), C.byref(cut), None), "gp_estimate_fpfh")
    return tuple(t.cpu().numpy() if t is not None else None for t in (out64, out32, sp, num)) + (cut.value,)


def test_the_c_entry_with_both_outputs_and_with_the_spfh_alone(gpa, runs):
    p, n, radius = R.edge_cloud("dirty300")
    fr = _frame(gpa, p, n)
    full = runs[("dirty300", 10000)]
    both = _c_call(gpa, fr, radius, 10000, 300, 300, f64=True, f32=True, spfh=True)
    only64 = _c_call(gpa, fr, radius, 10000, 300, 300, f64=True)
    assert np.array_equal(_bits(both[0]), _bits(only64[0])) and np.array_equal(_bits(both[0]), _bits(full[0]))
    assert np.array_equal(_bits(both[1]), _bits(both[0].astype(np.float32)))  # those bits rounded once
    assert np.array_equal(_bits(both[2]), _bits(full[1])) and np.array_equal(both[3], full[2]) and both[4] == full[3]
    # both outputs through an index list (indices_dev set): row k is the request's
    idx = np.array([R.DIRTY["sources"][0], 299, R.DIRTY["pos_inf"], 0, 299], np.int32)
    sub = _c_call(gpa, fr, radius, 10000, 300, len(idx), idx=idx, f64=True, f32=True)
    assert np.array_equal(_bits(sub[0]), _bits(full[0][idx])) and np.array_equal(_bits(sub[1]), _bits(full[0][idx].astype(np.float32)))
    # the SPFH alone: no FPFH pass, the same bits, counts and truncation
    alone = _c_call(gpa, fr, radius, 10000, 300, 0, spfh=True)
    assert alone[0] is None and alone[1] is None
    assert np.array_equal(_bits(alone[2]), _bits(full[1])) and np.array_equal(alone[3], full[2]) and alone[4] == full[3]
    # ... and through the binding, where an empty index list leaves nothing but the SPFH to compute
    import torch

    out, spfh, num, cut = gpa.estimate_fpfh_gpu(fr, gpa.FPFHEstimationParams(radius, 10000), indices=np.zeros(0, np.int32), dtype=torch.float64, return_spfh=True)
    assert tuple(out.shape) == (0, 33) and np.array_equal(_bits(spfh.cpu().numpy()), _bits(full[1])) and np.array_equal(num.cpu().numpy(), full[2]) and cut == full[3]


@pytest.mark.parametrize("name,cap", (("dense1500", 100), ("wrap2000", 10000), ("wrap2000", R.CAP)))
def test_two_calls_give_the_same_bits(gpa, runs, name, cap):
    again = _host(_run(gpa, R.edge_cloud(name), cap))  # (the table's layout may differ from call to call; the outputs may not)
    first = runs[(name, cap)]
    assert np.array_equal(_bits(again[0]), _bits(first[0])) and np.array_equal(_bits(again[1]), _bits(first[1]))
    assert np.array_equal(again[2], first[2]) and again[3] == first[3]

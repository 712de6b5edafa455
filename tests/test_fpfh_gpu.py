"""FPFH on the device (gp_estimate_fpfh / estimate_fpfh_gpu) against tests/fpfh_ref.py, the f64 restatement of the reference (tests/test_fpfh_ref_cpu.py holds the
hand cases and shows that every cloud here is settled by the restatement alone).  On settled points the neighbour counts and the integer histograms are compared
exactly; settled FPFH rows entry-wise within fpfh_ref.fpfh_tolerance, the bound derived there; zero entries are zero and NaN rows NaN on both sides."""
import numpy as np
import pytest

import fpfh_ref as R

pytestmark = pytest.mark.gpu
CAPS = (10000, R.CAP)


@pytest.fixture(scope="module")
def gpa():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import gtsam_points_amd

    return gtsam_points_amd


@pytest.fixture(scope="module")
def refs():
    """the restatement of every cloud, with and without the binding cap: computed once, never modified"""
    return {(name, cap): R.estimate(*R.cloud(name), cap) for name in R.CLOUDS for cap in CAPS}


def _frame(gpa, points, normals):
    return gpa.PointCloudGPU(np.ascontiguousarray(points), normals=np.ascontiguousarray(normals))


def _run(gpa, name, cap, **kw):
    import torch

    p, n, radius = R.cloud(name)
    return gpa.estimate_fpfh_gpu(_frame(gpa, p, n), gpa.FPFHEstimationParams(radius, cap), dtype=torch.float64, return_spfh=True, **kw)


@pytest.fixture(scope="module")
def runs(gpa):
    return {(name, cap): tuple(t.cpu().numpy() if hasattr(t, "cpu") else t for t in _run(gpa, name, cap)) for name in R.CLOUDS for cap in CAPS}


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("name", R.CLOUDS)
def test_neighbour_counts_and_histograms_are_the_references(refs, runs, name, cap):
    ref = refs[(name, cap)]
    fpfh, spfh, num, cut = runs[(name, cap)]
    s = ref.settled
    assert s.mean() >= 0.99
    assert np.array_equal(num[s], ref.n[s])
    assert cut == ref.num_truncated
    if cap == R.CAP and name == "random600":
        assert cut > 300  # the cap binds for most points: the walk order is what is being compared
    counts = np.rint(spfh * ((num - 1) / 100.0)[:, None]).astype(np.int64)
    assert np.array_equal(counts[s], ref.hist[s])
    # ... and the stored value is the reference's f64 product (:245-246), to the bit
    assert np.array_equal(spfh[s], ref.spfh[s])
    assert not spfh[num <= 1].any()


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("name", R.CLOUDS)
def test_settled_rows_are_within_the_derived_bound(refs, runs, name, cap):
    ref = refs[(name, cap)]
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
    print(f"{name} cap {cap}: worst entry at {worst:.3f} of the bound")


def test_points_that_are_not_finite(refs, runs):
    fpfh, spfh, num, _ = runs[("signed300", 10000)]
    assert num[7] == 0 and not spfh[7].any() and not fpfh[7].any()  # the NaN point: nobody's neighbour, zero rows
    ref = refs[("signed300", 10000)]
    assert all(7 not in js.tolist() for k, js in enumerate(ref.neighbors) if k != 7)
    assert num[11] == ref.n[11] > 1  # the point with the NaN normal is a neighbour like any other; its own pairs return zero: bin 5 of each block
    assert np.array_equal(spfh[11], ref.spfh[11]) and spfh[11][[5, 16, 27]].tolist() == [100.0] * 3


def test_coincident_copies_give_a_nan_row(gpa):
    import torch

    p = np.tile(np.array([[0.5, 0.25, -1.0]], np.float32), (3, 1))
    n = np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (3, 1))
    fpfh, spfh, num, cut = gpa.estimate_fpfh_gpu(_frame(gpa, p, n), gpa.FPFHEstimationParams(0.8, 10000), dtype=torch.float64, return_spfh=True)
    assert num.cpu().tolist() == [3, 3, 3] and cut == 0
    assert np.array_equal(spfh.cpu().numpy(), R.estimate(p, n, 0.8).spfh)
    assert torch.isnan(fpfh).all()


def test_f32_output_is_the_f64_output_rounded_once(gpa, runs):
    for name in ("random600", "signed300"):
        p, n, radius = R.cloud(name)
        f32 = gpa.estimate_fpfh_gpu(_frame(gpa, p, n), gpa.FPFHEstimationParams(radius, 10000))
        assert str(f32.dtype) == "torch.float32" and tuple(f32.shape) == (len(p), 33) and f32.is_cuda
        assert np.array_equal(f32.cpu().numpy().view(np.uint32), runs[(name, 10000)][0].astype(np.float32).view(np.uint32))


@pytest.mark.parametrize("cap", CAPS)
def test_a_shuffled_subset_with_a_repeat_gives_the_full_calls_rows(gpa, runs, cap):
    import torch

    p, n, radius = R.cloud("random600")
    idx = np.random.default_rng(5).permutation(600)[:101].astype(np.int32)
    idx[100] = idx[3]
    sub = gpa.estimate_fpfh_gpu(_frame(gpa, p, n), gpa.FPFHEstimationParams(radius, cap), indices=idx, dtype=torch.float64)
    assert tuple(sub.shape) == (101, 33)
    assert np.array_equal(sub.cpu().numpy().view(np.uint64), runs[("random600", cap)][0][idx].view(np.uint64))
    none = gpa.estimate_fpfh_gpu(_frame(gpa, p, n), gpa.FPFHEstimationParams(radius, cap), indices=np.zeros(0, np.int32))
    assert tuple(none.shape) == (0, 33)


@pytest.mark.parametrize("name", ("random600", "cell65", "plane400"))
def test_two_calls_give_the_same_bits(gpa, runs, name):
    for cap in CAPS:
        again = _run(gpa, name, cap)
        first = runs[(name, cap)]
        assert np.array_equal(again[0].cpu().numpy().view(np.uint64), first[0].view(np.uint64))
        assert np.array_equal(again[1].cpu().numpy().view(np.uint64), first[1].view(np.uint64))
        assert np.array_equal(again[2].cpu().numpy(), first[2]) and again[3] == first[3]


def test_missing_normals_and_bad_indices_raise(gpa):
    p, n, radius = R.cloud("two")
    with pytest.raises(gpa.GPError):
        gpa.estimate_fpfh_gpu(gpa.PointCloudGPU(p), gpa.FPFHEstimationParams(radius))
    fr = _frame(gpa, p, n)
    for bad in ([0, 2], [-1]):
        with pytest.raises(IndexError):
            gpa.estimate_fpfh_gpu(fr, gpa.FPFHEstimationParams(radius), indices=bad)
    with pytest.raises(gpa.GPError):
        gpa.estimate_fpfh_gpu(fr, gpa.FPFHEstimationParams(0.0))


def test_descriptors_feed_gnc_and_the_known_pose_comes_back(gpa):
    tp, tn, sp, sn, T, radius = R.height_field()
    target, source = _frame(gpa, tp, tn), _frame(gpa, sp, sn)
    params = gpa.FPFHEstimationParams(radius)
    tf, sf = gpa.estimate_fpfh_gpu(target, params), gpa.estimate_fpfh_gpu(source, params)
    assert tf.is_cuda and sf.is_cuda and str(tf.dtype) == "torch.float32"
    res = gpa.estimate_pose_gnc_gpu(target, source, tf, sf)
    got = np.asarray(res.T_target_source, np.float64)
    print("rotation error", np.abs(got[:3, :3] - T[:3, :3]).max(), "translation error", np.abs(got[:3, 3] - T[:3, 3]).max(), "pairs", res.num_correspondences)
    assert np.abs(got[:3, :3] - T[:3, :3]).max() < 1e-6 and np.abs(got[:3, 3] - T[:3, 3]).max() < 1e-6

"""tests/voxelmap_ref.py checked without a GPU: the restatement against the CPU oracle on the KITTI fixture, and every generated case against its own
preconditions -- the sort width or fallback it is meant to reach, the exactness of its "exact" inputs, the faces its points are meant to lie on."""
from fractions import Fraction

import numpy as np
import pytest

import oracle
import voxelmap_ref as vr


@pytest.mark.parametrize("res", [0.3, 0.5, 1.0])
def test_restatement_equals_the_cpu_oracle_on_the_fixture(kitti00, res):
    p, c = kitti00["target_points"], kitti00["target_covs"]
    it = np.linalg.norm(p, axis=1).astype(np.float32)
    c9 = np.ascontiguousarray(c.transpose(0, 2, 1)).reshape(-1, 9).astype(np.float32)
    ref = vr.Map(p, c9, it, res)
    om = oracle.OracleVoxelMap(res)
    om.insert(p, c, it)
    oc, on, omean, ocov, oint = om.export()
    assert ref.num_voxels == om.num_voxels
    idx = np.array([ref.index[tuple(x)] for x in oc.tolist()])  # KeyError = a voxel the restatement does not have
    assert len(set(idx.tolist())) == ref.num_voxels
    np.testing.assert_array_equal(on, ref.counts[idx])
    assert np.abs(omean - ref.means[idx]).max() < 1e-12 and np.abs(ocov - ref.covs[idx]).max() < 1e-12
    np.testing.assert_array_equal(oint.astype(np.float32), ref.intensities[idx])
    # what the device stores differs from the mean by the f32 rounding of the offset from the centre
    assert np.abs(ref.means_stored - ref.means).max() <= res * 2.0**-25 + 1e-15


def test_intensity_rule():
    f = np.float32
    assert vr.intensity_max([-5.0, -1.0]).tobytes() == f(0.0).tobytes()
    assert vr.intensity_max([-0.0]).tobytes() == f(0.0).tobytes()  # +0.0, not -0.0
    assert vr.intensity_max([np.nan, -np.nan]).tobytes() == f(0.0).tobytes()
    assert vr.intensity_max([np.nan, 2.0, np.nan, -7.0]) == f(2.0)
    assert vr.intensity_max([3.0e38, 1.0, np.inf]) == f(np.inf)
    assert vr.intensity_max([1e-30, -np.inf]) == f(1e-30)


def test_valid_rule_and_paths():
    bad = vr.bad_rows()
    assert not vr.valid_mask(bad, 0.5).any()
    edge = np.array([[5.0e8, 0, 0], [np.nextafter(np.float32(5.0e8), np.float32(0)), 0, 0], [-5.0e8, 0, 0]], dtype=np.float32)
    assert vr.valid_mask(edge, 0.5).tolist() == [False, True, False]  # |p / res| < 1e9, strictly
    assert vr.predicted_path(bad, 0.5) is None
    # the thresholds of bin_points_once: 3 / 4 blocks, 1023 / 1024, 2^18 - 1 / 2^18, 2^24 / 2^24 + ...
    def line(blocks):
        return np.array([[0.5, 0.5, 0.5], [(blocks - 1) * 4 + 0.5, 0.5, 0.5]], dtype=np.float32)

    assert [vr.predicted_path(line(b), 1.0) for b in (1, 3, 4, 1023, 1024, (1 << 18) - 1, 1 << 18, 1 << 22)] == [1, 1, 2, 2, 3, 3, 4, 4]
    sq = np.array([[0.5, 0.5, 0.5], [4095 * 4 + 0.5, 4095 * 4 + 0.5, 0.5]], dtype=np.float32)
    assert vr.predicted_path(sq, 1.0) == 4
    sq[1, 0] += 4.0
    assert vr.predicted_path(sq, 1.0) == "hashed"


@pytest.mark.parametrize("name", vr.WIDTH_CASES)
def test_width_cases_reach_their_path(name):
    case = vr.case_width(name)
    assert vr.predicted_path(case["points"], case["res"]) == case["path"]
    assert vr.valid_mask(case["points"], case["res"]).all() and len(case["points"]) <= 20000
    blocks = vr.voxel_coords(case["points"], case["res"]) >> 2
    dims = blocks.max(axis=0) - blocks.min(axis=0) + 1
    if name == "4 passes":
        assert dims.tolist() == [4096, 4096, 1]  # 2^24 blocks: the last box the binned build takes
    if name == "fallback":
        assert dims.tolist() == [4097, 4097, 1]
    if name.startswith("thin"):
        a = 0 if name == "thin x" else 2
        assert dims[a] > (1 << 20) - 4096 and dims[a] <= (1 << 20) + 1 and np.delete(dims, a).tolist() == [1, 1]
    if name == "thin z":
        assert blocks[:, 2].min() < 0 < blocks[:, 2].max()


@pytest.fixture(scope="module")
def exact_case():
    return vr.case_exact_phases()


def test_exact_case_layout(exact_case):
    """every population sits behind k = 0 .. 16 one-point voxels of its own sixteen-voxel workgroup: the voxel order the build must produce is the order of the
    generator, and the large voxel's first row lies k rows behind its workgroup's first"""
    case = exact_case
    assert vr.predicted_path(case["points"], 0.5) == case["path"] == 2
    order, counts = case["voxel_order"], case["voxel_counts"]
    assert len(order) % vr.STATS_GROUP == 0
    # (block, bit) order of gp_binning.hpp: block along x here, bit = (cy & 3) << 2 | (cx & 3)
    key = (order[:, 0] >> 2) * 64 + ((order[:, 1] & 3) << 2 | (order[:, 0] & 3))
    assert (np.diff(key) > 0).all() and (order[:, 2] == 0).all() and (order[:, 0] >> 2).min() < 0 < (order[:, 0] >> 2).max()
    starts = np.concatenate([[0], np.cumsum(counts)])
    seen = set()
    for v in np.flatnonzero(counts > 1):
        g0 = v - v % vr.STATS_GROUP
        k = int(starts[v] - starts[g0])
        assert k == v % vr.STATS_GROUP  # k one-point voxels in front, inside the workgroup
        prev16 = v % vr.STATS_GROUP == 0 and g0 >= vr.STATS_GROUP and (counts[g0 - vr.STATS_GROUP : g0] == 1).all()
        seen.add((int(counts[v]), k))
        if prev16:
            seen.add((int(counts[v]), 16))
        if counts[v] + k > vr.STATS_BATCH:  # the voxel crosses the first batch boundary 512 - k rows in: lane phase -k mod 16
            assert (vr.STATS_BATCH - k) % vr.STATS_GROUP == (-k) % vr.STATS_GROUP
    assert seen >= {(p, k) for p in vr.POPULATIONS if p > 1 for k in range(17)}
    ref = vr.Map(case["points"], case["covs"], case["intensities"], 0.5)
    np.testing.assert_array_equal(np.array([ref.counts[ref.index[tuple(c)]] for c in order.tolist()]), counts)


def test_exact_case_is_exact(exact_case):
    """the rational sums equal the f64 sums in two different orders, the device's own formulas give the restatement's values bit for bit, and the reversed cloud is
    the same map"""
    case = exact_case
    p, c, it = case["points"], case["covs"], case["intensities"]
    assert (p.astype(np.float64) * 64 == np.rint(p.astype(np.float64) * 64)).all() and (c == np.rint(c)).all() and (it == np.rint(it)).all()
    ref = vr.Map(p, c, it, 0.5)
    rev = vr.Map(p, c, it, 0.5, order=vr.reversed_rows)
    for a in ("means", "means_stored", "covs", "intensities"):
        assert getattr(ref, a).tobytes() == getattr(rev, a).tobytes(), a
    p64, s6 = p.astype(np.float64), vr.sym6(c)
    for v in list(range(0, ref.num_voxels, 37)) + np.flatnonzero(ref.counts > 500).tolist():
        rows = np.flatnonzero(ref.point_voxel == v)
        n = len(rows)
        for order in (rows, rows[::-1]):
            for k in range(3):
                off = p64[order, k] - ref.centres[v, k]
                acc = 0.0
                for x in off.tolist():
                    acc += x
                assert Fraction(acc) == sum(Fraction(x) for x in off.tolist())
                local = acc * (1.0 / n)  # the device: acc * inv_n, mean_local = (float) of it, voxel_means = (float)(centre + it)
                assert ref.centres[v, k] + float(np.float32(local)) == ref.means_stored[v, k]
                assert np.float32(ref.centres[v, k] + local) == np.float32(ref.means[v, k])
            for k in range(6):
                acc = 0.0
                for x in s6[order, k].tolist():
                    acc += x
                assert Fraction(acc) == sum(Fraction(x) for x in s6[order, k].tolist())
                assert acc / n == ref.covs[v].reshape(9)[[0, 1, 2, 4, 5, 8][k]]
    r = vr.case_exact_phases(reverse=True)
    np.testing.assert_array_equal(r["points"], p[::-1])
    rr = vr.Map(r["points"], r["covs"], r["intensities"], 0.5)
    for a in ("coords", "counts", "means_stored", "covs", "intensities"):
        assert getattr(ref, a).tobytes() == getattr(rr, a).tobytes(), a


@pytest.mark.parametrize("res", vr.FACE_RESOLUTIONS)
def test_face_cases_lie_on_faces(res):
    case = vr.case_faces(res)
    p = case["points"]
    m = vr.face_margin_ulps(p, res)
    assert ((m == 0) | (m > 2)).all() and vr.valid_mask(p, res).all()
    u = vr.scaled(p, res)
    on_face = u == np.rint(u)
    assert (on_face & np.signbit(p) & (p == 0)).any() and (on_face & ~np.signbit(p) & (p == 0)).any()  # -0.0 and +0.0
    c = vr.voxel_coords(p, res)
    assert (c[np.signbit(p) & (p == 0)] == 0).all()  # -0.0 is in voxel 0, not -1
    if res in (0.5, 100.0):  # a dyadic leaf: m * res is exact, the point IS on the face, at positive and at negative coordinates
        assert (on_face & (p > 0)).any() and (on_face & (p < 0)).any()
        for s in (1.0, -1.0):
            face = np.float32(s * 2 * res)
            below, above = np.nextafter(face, np.float32(-np.inf)), np.nextafter(face, np.float32(np.inf))
            for val, want in ((face, int(s * 2)), (below, int(s * 2) - 1), (above, int(s * 2))):
                rows = (p == val).all(axis=1)
                assert rows.any() and (c[rows] == want).all()
    # one ulp either side of a face lands in two different voxels
    assert len(np.unique(c[:, 0])) >= 8


@pytest.mark.parametrize("res", [0.5, 0.1])
def test_far_cases(res):
    base = vr.case_far(0.0, res)
    for d in vr.FAR_DISTANCES:
        case = vr.case_far(d, res)
        assert len(case["points"]) == 4096 and vr.valid_mask(case["points"], res).all()
        assert isinstance(case["path"], int)
        want = (vr.far_patch() + d).astype(np.float32)  # shifted in f64, rounded to f32 once
        np.testing.assert_array_equal(case["points"], want)
        np.testing.assert_array_equal(case["covs"], base["covs"])


def test_invalid_and_intensity_and_reinsert_cases():
    for fallback in (False, True):
        case = vr.case_invalid(fallback)
        p, keep = case["points"], case["keep"]
        assert (vr.valid_mask(p, 0.5) == keep).all() and (~keep).sum() == len(vr.BAD_AT)
        assert not keep[[0, 4095, 4096, len(p) - 1]].any()
        assert vr.predicted_path(p, 0.5) == case["path"] and (case["path"] == "hashed") == fallback
        full = vr.Map(p, case["covs"], case["intensities"], 0.5)
        cut = vr.Map(p[keep], case["covs"][keep], case["intensities"][keep], 0.5)
        for a in ("coords", "counts", "means", "means_stored", "covs", "intensities"):
            assert getattr(full, a).tobytes() == getattr(cut, a).tobytes(), a
            assert np.isfinite(getattr(full, a)).all()
        assert (full.point_voxel[~keep] == -1).all()
    none = vr.case_all_invalid()
    assert len(none["points"]) > 4096 and not vr.valid_mask(none["points"], 0.5).any()
    assert vr.Map(none["points"], none["covs"], none["intensities"], 0.5).num_voxels == 0
    ic = vr.case_intensities()
    m = vr.Map(ic["points"], ic["covs"], ic["intensities"], 0.5)
    assert m.num_voxels == 48
    assert (m.intensities.view(np.uint32) == 0).any() and np.isinf(m.intensities).any() and not np.isnan(m.intensities).any() and (m.intensities >= 0).all()
    assert not np.signbit(m.intensities).any()
    it = ic["intensities"]
    assert np.isnan(it).any() and (it < 0).any() and (np.signbit(it) & (it == 0)).any() and (it == np.float32(3.0e38)).any()
    for which in ("A larger", "A smaller"):
        a, b = vr.case_reinsert(which)
        ma, mb = vr.Map(a["points"], a["covs"], a["intensities"], 0.5), vr.Map(b["points"], b["covs"], b["intensities"], 0.5)
        shared = set(ma.index) & set(mb.index)
        assert shared and set(ma.index) - shared and set(mb.index) - shared
        assert (len(a["points"]) > len(b["points"])) == (which == "A larger")

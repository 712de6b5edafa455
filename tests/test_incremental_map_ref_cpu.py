"""The restatement of the incremental voxel map (tests/incremental_map_ref.py) pinned against the reference's own class and against the oracle, and the refusals the new
entry points make on the host before any device work.

Tolerance of the comparisons with the reference classes, 1e-12 relative: both sides hold f64 sums of <= a few hundred terms of magnitude <= 20 (coordinates, metres),
each addition rounding by <= 2^-53 of the partial sum, and the reference re-multiplies its finalized mean by the count at every insert (one more rounding per insert):
a few hundred roundings of 1.1e-16 relative stay below 1e-13; means are compared with an absolute term of 1e-12 x the largest coordinate, because a mean near zero
carries the absolute error of its terms."""
import ctypes as C

import numpy as np
import pytest

import incremental_map_ref as ir
import voxelmap_ref as vr
from oracle import OracleVoxelMap, refcapi


def _by_coord(coords, *arrays):
    order = np.lexsort((coords[:, 2], coords[:, 1], coords[:, 0]))
    return [coords[order].astype(np.int64)] + [a[order] for a in arrays]


def _same_as_snapshot(snap, coords, counts, means, covs, scale, what):
    coords, counts, means, covs = _by_coord(coords, counts, means, covs)
    assert coords.shape == snap.coords.shape and (coords == snap.coords).all(), f"{what}: voxel sets differ"
    np.testing.assert_array_equal(counts, snap.counts, err_msg=f"{what}: counts")
    np.testing.assert_allclose(means, snap.means, rtol=1e-12, atol=1e-12 * scale, err_msg=f"{what}: means")
    np.testing.assert_allclose(0.5 * (covs + covs.transpose(0, 2, 1)), snap.covs, rtol=1e-12, atol=1e-12 * snap.max_abs_cov.max(), err_msg=f"{what}: covs")


@pytest.mark.skipif(not refcapi.available(), reason="the reference's own classes are not built (oracle/_ref)")
def test_restatement_equals_the_reference_class_over_a_sliding_sequence():
    frames = ir.sliding_frames()
    assert len(frames) == 21
    ref = refcapi.RefVoxelMap(ir.SLIDING_RES)  # upstream's defaults: lru_horizon 10, lru_clear_cycle 10
    mine = ir.IncrementalMap(ir.SLIDING_RES)
    sizes = []
    for k, (pts, covs, _) in enumerate(frames, start=1):
        before = set(mine.voxels)
        ref.insert(pts, covs)
        mine.insert(pts, covs)
        sizes.append(mine.num_voxels)
        assert ref.num_voxels == mine.num_voxels, f"insert {k}"
        if k in (10, 20, 21):
            coords, npts, means, covs_r, _ = ref.export()
            _same_as_snapshot(mine.snapshot(), coords, npts, means, covs_r, 20.0, f"after insert {k}")
        if k == 20:
            evicted = set(mine.evicted)
            assert evicted and sizes[-1] < sizes[-2], "insert 20 must evict"
            assert evicted <= before and all(c[0] < 12 for c in evicted)  # frames 0 .. 9 reach x < 6 m: cx < 12 at leaf 0.5
        else:
            assert not mine.evicted
    # a coordinate evicted at insert 20 and revisited at 21 holds the points of frame 21 alone
    pts = frames[20][0]
    c21 = vr.voxel_coords(pts, ir.SLIDING_RES)
    revisited = [tuple(c) for c in np.unique(c21, axis=0).tolist() if tuple(c) in evicted]
    assert revisited
    snap = mine.snapshot()
    coords, npts, _, _, _ = ref.export()
    ref_counts = {tuple(c): int(n) for c, n in zip(coords.tolist(), npts.tolist())}
    for c in revisited:
        want = int((c21 == np.array(c)).all(axis=1).sum())
        assert snap.counts[snap.index[c]] == want == ref_counts[c], c
        assert snap.stamps[snap.index[c]] == 20


def test_restatement_equals_the_oracle_over_two_inserts():
    a, b = vr.case_reinsert("A larger")
    orc = OracleVoxelMap(0.5)
    mine = ir.IncrementalMap(0.5)
    for case in (a, b):
        orc.insert(case["points"], case["covs"], case["intensities"])
        mine.insert(case["points"], case["covs"], case["intensities"])
    snap = mine.snapshot()
    both = vr.Map(np.concatenate([a["points"], b["points"]]), np.concatenate([a["covs"], b["covs"]]), np.concatenate([a["intensities"], b["intensities"]]), 0.5)
    shared = set(vr.Map(a["points"], a["covs"], None, 0.5).index) & set(vr.Map(b["points"], b["covs"], None, 0.5).index)
    assert shared and len(shared) < snap.num_voxels, "the two clouds must share some voxels and not all"
    # no eviction: the incremental map of A then B is the one-shot map of their concatenation
    assert (snap.coords == both.coords).all() and (snap.counts == both.counts).all()
    assert snap.means.tobytes() == both.means.tobytes() and snap.covs.tobytes() == both.covs.tobytes() and snap.intensities.tobytes() == both.intensities.tobytes()
    coords, npts, means, covs, intens = orc.export()
    order = np.lexsort((coords[:, 2], coords[:, 1], coords[:, 0]))
    _same_as_snapshot(snap, coords, npts, means, covs, 6.0, "oracle, A then B")
    np.testing.assert_array_equal(intens[order].astype(np.float32), snap.intensities)
    assert (snap.stamps[[snap.index[c] for c in shared]] == 1).all() and set(snap.stamps.tolist()) == {0, 1}


def test_eviction_rule_at_the_edges():
    rng = np.random.default_rng(5)
    pts = rng.uniform(-1, 1, size=(50, 3)).astype(np.float32)
    covs = ir.symmetric_covs(rng, 50)
    m = ir.IncrementalMap(0.5, lru_horizon=0, lru_clear_cycle=1)
    for k in range(3):
        m.insert(pts, covs)
        assert m.num_voxels == 0 and m.lru_counter == k + 1  # the voxels just touched go too
    m = ir.IncrementalMap(0.5, lru_horizon=2, lru_clear_cycle=1)
    m.insert(pts, covs)
    n1 = m.num_voxels
    m.insert(np.zeros((0, 3), np.float32), np.zeros((0, 9), np.float32))  # an empty frame counts: stamp 0 + 2 < 2 is false
    assert m.num_voxels == n1 > 0
    m.insert(np.zeros((0, 3), np.float32), np.zeros((0, 9), np.float32))  # 0 + 2 < 3
    assert m.num_voxels == 0 and m.lru_counter == 3


def test_new_names_are_exported():
    import gtsam_points_amd as gpa
    from gtsam_points_amd import _capi, types

    assert gpa.IncrementalGaussianVoxelMapGPU is types.IncrementalGaussianVoxelMapGPU
    assert issubclass(types.IncrementalGaussianVoxelMapGPU, types.GaussianVoxelMapGPU)
    assert "IncrementalGaussianVoxelMapGPU" not in gpa.__all__
    lib = _capi.load()
    for sym in ("gp_voxelmap_insert_incremental", "gp_voxelmap_set_lru", "gp_voxelmap_lru_get", "gp_voxelmap_download_stamps"):
        assert sym in _capi.EXPORTED_SYMBOLS and hasattr(lib, sym), sym


def test_entry_points_refuse_bad_arguments_without_a_device():
    from gtsam_points_amd import _capi

    lib = _capi.load()
    INVALID = 1
    fake = C.c_void_p(64)  # never dereferenced: every call below is refused first
    c, h, k = C.c_int64(-7), C.c_int64(-7), C.c_int64(-7)
    assert lib.gp_voxelmap_insert_incremental(None, fake, fake, None, 1) == INVALID and b"gp_voxelmap_insert_incremental" in lib.gp_last_error()
    assert lib.gp_voxelmap_set_lru(None, 10, 10) == INVALID and b"gp_voxelmap_set_lru" in lib.gp_last_error()
    assert lib.gp_voxelmap_lru_get(None, C.byref(c), C.byref(h), C.byref(k)) == INVALID and c.value == -7
    assert lib.gp_voxelmap_download_stamps(None, fake) == INVALID
    m = C.c_void_p()
    assert lib.gp_voxelmap_create(0.5, 16384, 10, 0.0, None, C.byref(m)) == 0 and m.value  # (a handle is host memory: no device work)
    try:
        assert lib.gp_voxelmap_lru_get(m, C.byref(c), C.byref(h), C.byref(k)) == 0 and (c.value, h.value, k.value) == (0, 10, 10)
        for horizon, cycle in ((-1, 10), (10, 0), (10, -3), (-1, 0)):
            assert lib.gp_voxelmap_set_lru(m, horizon, cycle) == INVALID, (horizon, cycle)
        assert lib.gp_voxelmap_lru_get(m, C.byref(c), C.byref(h), C.byref(k)) == 0 and (c.value, h.value, k.value) == (0, 10, 10)
        assert lib.gp_voxelmap_set_lru(m, 0, 1) == 0
        assert lib.gp_voxelmap_lru_get(m, None, C.byref(h), C.byref(k)) == 0 and (h.value, k.value) == (0, 1)
        assert lib.gp_voxelmap_insert_incremental(m, fake, fake, None, -1) == INVALID
        assert lib.gp_voxelmap_insert_incremental(m, None, fake, None, 1) == INVALID and lib.gp_voxelmap_insert_incremental(m, fake, None, None, 1) == INVALID
        assert lib.gp_voxelmap_lru_get(m, C.byref(c), None, None) == 0 and c.value == 0  # a refused insert does not count
    finally:
        lib.gp_voxelmap_destroy(m)

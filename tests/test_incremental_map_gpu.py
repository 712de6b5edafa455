"""The incremental Gaussian voxel map with LRU eviction (IncrementalGaussianVoxelMapGPU, csrc/gp_voxelmap_incremental.hip) against its numpy f64 / math.fsum
restatement (tests/incremental_map_ref.py, pinned against the reference's own class by tests/test_incremental_map_ref_cpu.py).  Every comparison is keyed by voxel
coordinate.  Voxel sets, counts, stamps and intensities are exact.

Bounds, from the stored formats only (res = leaf, n = points the voxel holds, over all inserts):
  download_f64 covs    n * 2^-52 * max|c|                 the device adds n terms <= max|c| in f64 -- inside a frame in the binned build's fixed order, then old +
                                                          new once per insert: at most n additions, each rounding by <= 2^-53 of a partial sum <= n max|c|,
                                                          taken as n * 2^-52 * max|c| -- and divides once.  The sums are KEPT in f64, so nothing else accrues
                                                          per insert.
  download_f64 means   res * 2^-24 + n * 2^-52 * res      the same n additions of offsets |p - centre| <= res, then ONE f32 rounding of mean_local (magnitude
                                                          <= res, so <= res * 2^-24) per finalize -- from the f64 sums, not from the last insert's f32 value
  f32 arrays           1 ulp_f32(f32(ref)) + the f64 bound above
                                                          the device rounds its f64 value, which lies within the f64 bound of the restatement's: the two roundings
                                                          are the same float or, when a rounding boundary lies between the two f64 values, neighbours
The restatement itself is correctly rounded (math.fsum over all the terms a voxel holds, one division)."""
import ctypes as C

import numpy as np
import pytest

import incremental_map_ref as ir
import oracle
import voxelmap_ref as vr
from helpers import assert_linearized_close, expmap, reference_bucket_lookup

pytestmark = pytest.mark.gpu

INVALID = 1  # GP_ERROR_INVALID_ARGUMENT, include/gtsam_points_hip.h
PARITY_TOL = 1e-6  # tests/test_vgicp_gpu.py
FIELDS = ("H_target", "H_source", "H_target_source", "b_target", "b_source")


def _cloud(gpu, points, covs, intensities=None):
    """the f32 arrays on the device exactly as they are"""
    import torch

    return gpu.PointCloudGPU.from_device(
        torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32).copy()).to("cuda:0"),
        torch.from_numpy(np.ascontiguousarray(covs, dtype=np.float32).copy()).to("cuda:0"),
        torch.from_numpy(np.ascontiguousarray(intensities, dtype=np.float32).copy()).to("cuda:0") if intensities is not None else None,
    )


def _empty_frame(gpu):
    f = _cloud(gpu, np.zeros((1, 3)), np.zeros((1, 9)))
    f.num_points = 0
    return f


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def _everything(vm):
    """every array the map hands out, for bit comparisons"""
    dl = vm.download()
    return list(vm.download_f64()) + [dl[k] for k in ("buckets", "num_points", "means", "covs", "intensities")] + [vm.download_stamps()]


def _same_bits(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), f"{what}: array {i} differs"


def _check(gpu, vm, snap, what, lookup=None):
    """the map against the restatement's snapshot.  lookup = (cloud, points): every valid point must land in the voxel of its coordinate.  Returns the worst ratios."""
    info = vm.voxelmap_info
    assert info.num_voxels == snap.num_voxels, f"{what}: {info.num_voxels} voxels, the restatement has {snap.num_voxels}"
    coords, counts, means, covs = vm.download_f64()
    dl = vm.download()
    stamps = vm.download_stamps()
    if snap.num_voxels == 0:
        assert (dl["buckets"][:, 3] < 0).all() and len(stamps) == 0
        return {}
    missing = [tuple(c) for c in coords.tolist() if tuple(c) not in snap.index]
    assert not missing, f"{what}: voxels the restatement does not have: {missing[:5]}"
    idx = np.array([snap.index[tuple(c)] for c in coords.tolist()])
    assert len(set(idx.tolist())) == snap.num_voxels, f"{what}: a voxel is listed twice"
    np.testing.assert_array_equal(counts, snap.counts[idx], err_msg=f"{what}: counts")
    np.testing.assert_array_equal(dl["num_points"], snap.counts[idx], err_msg=f"{what}: num_points")
    np.testing.assert_array_equal(stamps, snap.stamps[idx], err_msg=f"{what}: stamps")
    assert np.array_equal(_bits(dl["intensities"]), _bits(snap.intensities[idx])), f"{what}: intensities"
    for name, a in (("means64", means), ("covs64", covs), ("means32", dl["means"]), ("covs32", dl["covs"])):
        assert np.isfinite(a).all(), f"{what}: {name} holds a non-finite entry"
    n = snap.counts[idx].astype(np.float64)
    res = snap.res
    rm, rc = snap.means[idx], snap.covs[idx]
    bm = (res * 2.0**-24 + n * 2.0**-52 * res)[:, None]
    bc = (n * 2.0**-52 * snap.max_abs_cov[idx])[:, None, None]
    ulp = lambda r: np.spacing(np.abs(r.astype(np.float32))).astype(np.float64)  # noqa: E731
    ratios = {
        "means64": float((np.abs(means - rm) / bm).max()),
        "covs64": float((np.abs(covs - rc) / bc).max()),
        "means32": float((np.abs(dl["means"].astype(np.float64) - rm.astype(np.float32).astype(np.float64)) / (ulp(rm) + bm)).max()),
        "covs32": float((np.abs(dl["covs"].astype(np.float64) - rc.astype(np.float32).astype(np.float64)) / (ulp(rc) + bc)).max()),
    }
    print(f"{what}: worst ratio to the bound " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    for k, v in ratios.items():
        assert v <= 1.0, f"{what}: {k} exceeds its bound by a factor {v:.3f}"
    # the block-order numbering every map here has: voxels ascend by (block z, y, x, bit)
    blk = coords >> 2
    key = np.stack([blk[:, 2], blk[:, 1], blk[:, 0], ((coords[:, 2] & 3) << 4) | ((coords[:, 1] & 3) << 2) | (coords[:, 0] & 3)], axis=1)
    assert (np.lexsort(key.T[::-1]) == np.arange(len(key))).all(), f"{what}: voxels are not in block order"
    b = dl["buckets"]
    used = b[b[:, 3] >= 0]
    assert sorted(used[:, 3].tolist()) == list(range(info.num_voxels)), f"{what}: bucket table"
    for v in list(range(0, info.num_voxels, 3)) + [info.num_voxels - 1]:
        assert reference_bucket_lookup(b, info, coords[v]) == v, f"{what}: voxel {v} not found through the bucket table"
    if lookup is not None:
        cloud, points = lookup
        got = vm.lookup(cloud)
        where = {tuple(c): v for v, c in enumerate(coords.tolist())}
        ok = vr.valid_mask(points, res)
        want = np.array([where.get(tuple(c), -1) if o else -1 for c, o in zip(vr.voxel_coords(points, res).tolist(), ok.tolist())])
        wrong = np.flatnonzero(got != want)
        assert len(wrong) == 0, f"{what}: lookup names another voxel for {len(wrong)} points, first row {wrong[0]}: {got[wrong[0]]} for {want[wrong[0]]}"
    return ratios


def _new(gpu, res=0.5, horizon=10, cycle=10):
    return gpu.IncrementalGaussianVoxelMapGPU(res, lru_horizon=horizon, lru_clear_cycle=cycle)


def _has_grid(gpu, vm):
    return gpu.load().gp_voxelmap_has_block_grid(vm._h)


@pytest.fixture(scope="module")
def ab():
    a, b = vr.case_reinsert("A larger")
    ref = ir.IncrementalMap(0.5)
    ref.insert(a["points"], a["covs"], a["intensities"])
    snap_a = ref.snapshot()
    ref.insert(b["points"], b["covs"], b["intensities"])
    return a, b, snap_a, ref.snapshot()


@pytest.fixture(scope="module")
def sliding():
    return ir.sliding_frames()


# ---- A then B ------------------------------------------------------------------------------------------------------------------------------------------------------


def test_a_then_b_adds_to_the_voxels_already_there(gpu, ab):
    a, b, snap_a, snap_ab = ab
    vm = _new(gpu)
    assert vm.lru_counter == 0 and (vm.lru_horizon, vm.lru_clear_cycle) == (10, 10)
    ca, cb = _cloud(gpu, a["points"], a["covs"], a["intensities"]), _cloud(gpu, b["points"], b["covs"], b["intensities"])
    vm.insert(ca)
    assert vm.lru_counter == 1
    _check(gpu, vm, snap_a, "A", lookup=(ca, a["points"]))
    vm.insert(cb)
    assert vm.lru_counter == 2 and _has_grid(gpu, vm) == 1
    _check(gpu, vm, snap_ab, "A then B", lookup=(cb, b["points"]))
    both_pts = np.concatenate([a["points"], b["points"]])
    call = _cloud(gpu, both_pts, np.concatenate([a["covs"], b["covs"]]), np.concatenate([a["intensities"], b["intensities"]]))
    _check(gpu, vm, snap_ab, "A then B, every point", lookup=(call, both_pts))
    # the one-shot map of concat(A, B): the same voxels in the same order, the statistics to the same bounds (its sums run in another order)
    one = gpu.GaussianVoxelMapGPU(0.5, target_points_drop_rate=0.0)
    one.insert(call)
    c1, n1, m1, v1 = one.download_f64()
    c2, n2, m2, v2 = vm.download_f64()
    assert c1.tobytes() == c2.tobytes() and n1.tobytes() == n2.tobytes()
    idx = np.array([snap_ab.index[tuple(c)] for c in c1.tolist()])
    n = snap_ab.counts[idx].astype(np.float64)
    assert (np.abs(m1 - m2) <= 2 * (0.5 * 2.0**-24 + n * 2.0**-52 * 0.5)[:, None]).all()  # each within its bound of the restatement
    assert (np.abs(v1 - v2) <= 2 * (n * 2.0**-52 * snap_ab.max_abs_cov[idx])[:, None, None]).all()
    assert one.download()["intensities"].tobytes() == vm.download()["intensities"].tobytes()


# ---- the sliding sequence --------------------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("horizon,cycle", [(10, 10), (2, 1)])
def test_sliding_sequence_evicts_and_follows_the_box(gpu, sliding, horizon, cycle):
    vm = _new(gpu, ir.SLIDING_RES, horizon, cycle)
    ref = ir.IncrementalMap(ir.SLIDING_RES, horizon, cycle)
    sizes, evictions, lo_x = [], 0, []
    for k, (pts, covs, ints) in enumerate(sliding, start=1):
        cloud = _cloud(gpu, pts, covs, ints)
        vm.insert(cloud)
        ref.insert(pts, covs, ints)
        evictions += bool(ref.evicted)
        assert vm.lru_counter == ref.lru_counter == k
        assert vm.voxelmap_info.num_voxels == ref.num_voxels, f"insert {k}"
        sizes.append(ref.num_voxels)
        if (horizon, cycle) == (2, 1) or k in (1, 9, 10, 19, 20, 21):
            _check(gpu, vm, ref.snapshot(), f"{horizon}/{cycle} insert {k}", lookup=(cloud, pts))
        lo_x.append(int(vm.download_f64()[0][:, 0].min()))
    assert evictions >= (1 if cycle == 10 else 15)
    assert min(lo_x) < 0 < max(lo_x), "the map's low corner must cross zero: the box grows and shrinks"
    if cycle == 10:
        assert sizes[19] < sizes[18] and lo_x[19] > lo_x[18] and lo_x[20] < lo_x[19]  # insert 20 evicts, insert 21 goes back to the start


def test_horizon_zero_empties_the_map_after_every_insert(gpu, sliding):
    vm = _new(gpu, ir.SLIDING_RES, 0, 1)
    for k, (pts, covs, ints) in enumerate(sliding[:3], start=1):
        cloud = _cloud(gpu, pts, covs, ints)
        vm.insert(cloud)
        assert vm.lru_counter == k and vm.voxelmap_info.num_voxels == 0 and len(vm.download_stamps()) == 0
        assert (vm.download()["buckets"][:, 3] < 0).all()
        assert (vm.lookup(cloud) == -1).all()
    # the next insert works: with a horizon the map fills again
    vm.set_lru_horizon(5)
    assert (vm.lru_horizon, vm.lru_clear_cycle) == (5, 1)
    ref = ir.IncrementalMap(ir.SLIDING_RES, 5, 1)
    ref.lru_counter = 3
    pts, covs, ints = sliding[3]
    cloud = _cloud(gpu, pts, covs, ints)
    vm.insert(cloud)
    ref.insert(pts, covs, ints)
    _check(gpu, vm, ref.snapshot(), "after the empty maps", lookup=(cloud, pts))


# ---- lane phases and the batch edge of the segmented sum -------------------------------------------------------------------------------------------------------


def test_second_insert_at_every_lane_phase_and_the_batch_edge(gpu):
    first, second = ir.phase_frames()
    vm, ref = _new(gpu), ir.IncrementalMap(0.5)
    for name, (pts, covs, ints) in (("first", first), ("second", second)):
        cloud = _cloud(gpu, pts, covs, ints)
        vm.insert(cloud)
        ref.insert(pts, covs, ints)
        snap = ref.snapshot()
        _check(gpu, vm, snap, f"phases, {name}", lookup=(cloud, pts))
    assert sorted(snap.counts.tolist()) == sorted([3] + [3 + n for n in ir.PHASE_POPULATIONS])
    assert snap.stamps[snap.index[(4, 0, 0)]] == 0 and (np.delete(snap.stamps, snap.index[(4, 0, 0)]) == 1).all()  # the voxel only the first insert touched


# ---- intensities, invalid points, empty frames --------------------------------------------------------------------------------------------------------------------


def test_intensities_invalid_points_and_empty_frames(gpu):
    rng = np.random.default_rng(31)
    n = 900
    pts = rng.uniform(-2.0, 2.0, size=(n, 3)).astype(np.float32)
    bad = vr.bad_rows()
    frames = []
    for j, ints in enumerate((rng.uniform(100, 255, n), None, rng.uniform(0, 50, n))):
        p = pts + np.float32(0.01 * j)
        for i, at in enumerate((0, 1, 450, -2, -1)):
            p[at] = bad[(i + j) % len(bad)]
        frames.append((p, vr.general_covs(rng, n), None if ints is None else ints.astype(np.float32)))
    vm, ref = _new(gpu), ir.IncrementalMap(0.5)  # 10 / 10: nothing is evicted while the three frames go in
    high = None
    for j, (p, covs, ints) in enumerate(frames):
        cloud = _cloud(gpu, p, covs, ints)
        vm.insert(cloud)
        ref.insert(p, covs, ints)
        snap = ref.snapshot()
        _check(gpu, vm, snap, f"intensities, frame {j}", lookup=(cloud, p))
        assert vm.download()["num_points"].sum() == snap.counts.sum()
        if j == 0:
            high = dict(zip(map(tuple, snap.coords.tolist()), snap.intensities.tolist()))
    kept = [c for c in map(tuple, snap.coords.tolist()) if c in high]
    assert kept and all(snap.intensities[snap.index[c]] == np.float32(high[c]) >= 100 for c in kept)  # the frame without and the lower one change nothing
    # empty frames advance the counter and may evict: at horizon 2 / cycle 2 the one that takes the counter to 4 removes the stamps 0 and 1 (frame 0's and frame
    # 1's own voxels), the one that takes it to 6 the rest; the one in between clears nothing
    assert vm.lru_counter == 3
    vm.set_lru_horizon(2)
    vm.set_lru_clear_cycle(2)
    ref.lru_horizon, ref.lru_clear_cycle = 2, 2
    sizes = [ref.num_voxels]
    for want_counter in (4, 5, 6):
        if want_counter == 5:  # (num_points == 0 asks for no array)
            gpu._capi.check(gpu.load().gp_voxelmap_insert_incremental(vm._h, None, None, None, 0), "gp_voxelmap_insert_incremental")
        else:
            vm.insert(_empty_frame(gpu))
        ref.insert(np.zeros((0, 3), np.float32), np.zeros((0, 9), np.float32))
        assert vm.lru_counter == ref.lru_counter == want_counter
        _check(gpu, vm, ref.snapshot(), f"empty frame, counter {want_counter}")
        sizes.append(ref.num_voxels)
    assert sizes[1] <= sizes[0] and sizes[2] == sizes[1] > 0 and sizes[3] == 0 == vm.voxelmap_info.num_voxels


# ---- factors on a map that changes ------------------------------------------------------------------------------------------------------------------------------------


def _linearize(gpu, f, delta):
    rec = gpu._capi.Linearized6()
    gpu._capi.check(f._lib.gp_vgicp_factor_linearize(f._h, gpu.types._pose16(delta), C.byref(rec)), "linearize")
    return gpu.LinearizedSystem6(rec)


def test_vgicp_factor_sees_the_second_insert(gpu, ab):
    a, b, _, snap_ab = ab
    rng = np.random.default_rng(37)
    # (the clouds of A and B with covariances symmetric to the last bit: the oracle, like the reference's CPU map, sums the matrices as they are, the device their
    # symmetric parts -- tests/voxelmap_ref.py -- and the two agree where the input is symmetric)
    a = dict(a, covs=ir.symmetric_covs(rng, len(a["points"])))
    b = dict(b, covs=ir.symmetric_covs(rng, len(b["points"])))
    sp = rng.uniform(-5.5, 5.5, size=(1200, 3)).astype(np.float32)
    sc = ir.symmetric_covs(rng, len(sp))
    src = gpu.PointCloudGPU(sp, sc.reshape(-1, 3, 3))
    vm = _new(gpu)
    vm.insert(_cloud(gpu, a["points"], a["covs"], a["intensities"]))
    delta = expmap([0.01, -0.02, 0.015, 0.05, -0.04, 0.03])
    f = gpu.IntegratedVGICPFactorGPU(0, 1, vm, src)
    before = _linearize(gpu, f, delta)
    vm.insert(_cloud(gpu, b["points"], b["covs"], b["intensities"]))
    after = _linearize(gpu, f, delta)
    fresh = _linearize(gpu, gpu.IntegratedVGICPFactorGPU(0, 1, vm, src), delta)
    assert after.num_inliers == fresh.num_inliers > before.num_inliers and after.error == fresh.error
    for k in FIELDS:
        assert getattr(after, k).tobytes() == getattr(fresh, k).tobytes(), k
    om = oracle.OracleVoxelMap(0.5)
    om.insert(a["points"], a["covs"], a["intensities"])
    om.insert(b["points"], b["covs"], b["intensities"])
    assert om.num_voxels == snap_ab.num_voxels
    assert_linearized_close(after, oracle.OracleVGICPFactor(om, sp, sc, 2).linearize(delta), PARITY_TOL, "A then B vs oracle")


# ---- determinism, clone, offload --------------------------------------------------------------------------------------------------------------------------------------


def test_two_maps_fed_the_same_sequence_hold_the_same_bits(gpu, sliding):
    maps = [_new(gpu, ir.SLIDING_RES, 2, 3), _new(gpu, ir.SLIDING_RES, 2, 3)]
    for pts, covs, ints in sliding[:8]:
        for vm in maps:
            vm.insert(_cloud(gpu, pts, covs, ints))
    _same_bits(_everything(maps[0]), _everything(maps[1]), "two maps, eight inserts")
    assert maps[0].voxelmap_info.num_voxels > 0


def test_clone_then_the_two_diverge(gpu, sliding):
    vm, ref = _new(gpu, ir.SLIDING_RES, 3, 2), ir.IncrementalMap(ir.SLIDING_RES, 3, 2)
    for pts, covs, ints in sliding[:3]:
        vm.insert(_cloud(gpu, pts, covs, ints))
        ref.insert(pts, covs, ints)
    h = C.c_void_p()
    gpu._capi.check(gpu.load().gp_voxelmap_clone_to_device(vm._h, 0, None, C.byref(h)), "gp_voxelmap_clone_to_device")
    clone = gpu.IncrementalGaussianVoxelMapGPU(ir.SLIDING_RES, _handle=h)
    assert (clone.lru_counter, clone.lru_horizon, clone.lru_clear_cycle) == (3, 3, 2)
    _same_bits(_everything(vm), _everything(clone), "clone")
    assert clone.memory_usage_gpu() == vm.memory_usage_gpu() >= vm.voxelmap_info.num_voxels * 80
    import copy

    ref2 = copy.deepcopy(ref)
    (p3, c3, i3), (p9, c9, i9) = sliding[3], sliding[9]
    vm.insert(_cloud(gpu, p3, c3, i3))
    ref.insert(p3, c3, i3)
    clone.insert(_cloud(gpu, p9, c9, i9))
    ref2.insert(p9, c9, i9)
    _check(gpu, vm, ref.snapshot(), "the original after the clone")
    _check(gpu, clone, ref2.snapshot(), "the clone on its own way")
    assert ref.snapshot().coords.tobytes() != ref2.snapshot().coords.tobytes()


def test_offload_reload_then_insert(gpu, sliding):
    vm, ref = _new(gpu, ir.SLIDING_RES, 2, 2), ir.IncrementalMap(ir.SLIDING_RES, 2, 2)
    for pts, covs, ints in sliding[:3]:
        vm.insert(_cloud(gpu, pts, covs, ints))
        ref.insert(pts, covs, ints)
    before = _everything(vm)
    assert vm.offload_gpu() and not vm.loaded_on_gpu()
    lib = gpu.load()
    pts, covs, ints = sliding[3]
    cloud = _cloud(gpu, pts, covs, ints)
    assert lib.gp_voxelmap_insert_incremental(vm._h, cloud.ptr(cloud.points_gpu), cloud.ptr(cloud.covs_gpu), None, len(pts)) != 0  # not on the GPU: refused
    assert vm.lru_counter == 3
    assert vm.reload_gpu()
    _same_bits(before, _everything(vm), "offload -> reload")
    vm.insert(cloud)
    ref.insert(pts, covs, ints)
    assert ref.evicted
    _check(gpu, vm, ref.snapshot(), "insert after the reload", lookup=(cloud, pts))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------------------------------


def test_a_box_beyond_the_block_budget_is_refused_and_nothing_changes(gpu, ab):
    a, _, snap_a, _ = ab
    vm = _new(gpu)
    ca = _cloud(gpu, a["points"], a["covs"], a["intensities"])
    vm.insert(ca)
    src = gpu.PointCloudGPU(a["points"][:500], a["covs"][:500].reshape(-1, 3, 3).transpose(0, 2, 1))
    f = gpu.IntegratedVGICPFactorGPU(0, 1, vm, src)
    L0 = _linearize(gpu, f, np.eye(4))
    before = _everything(vm)
    lib = gpu.load()
    eye = np.tile(np.eye(3, dtype=np.float32).reshape(1, 9) * 0.01, (2, 1))
    # two points 2e5 m apart in x and y at leaf 0.5: 1e5 x 1e5 blocks
    far = _cloud(gpu, np.array([[-1.0e5, -1.0e5, 0.0], [1.0e5, 1.0e5, 0.0]]), eye)
    # one point whose box WITH the map's exceeds the budget, though its own does not
    lone = _cloud(gpu, np.array([[3.0e5, 3.0e5, 0.0], [3.0e5, 3.0e5, 0.1]]), eye)
    for name, cloud in (("far", far), ("lone", lone)):
        rc = lib.gp_voxelmap_insert_incremental(vm._h, cloud.ptr(cloud.points_gpu), cloud.ptr(cloud.covs_gpu), None, 2)
        assert rc == INVALID and b"exceeds the block grid" in lib.gp_last_error(), name
        with pytest.raises(gpu._capi.GPError):
            vm.insert(cloud)
        assert vm.lru_counter == 1, name
        _same_bits(before, _everything(vm), f"after the refused insert ({name})")
    L1 = _linearize(gpu, f, np.eye(4))  # the generation did not move: the factor's tables are the ones it had
    for k in FIELDS:
        assert getattr(L0, k).tobytes() == getattr(L1, k).tobytes(), k
    _check(gpu, vm, snap_a, "after the refusals", lookup=(ca, a["points"]))


def test_one_shot_maps_are_refused_and_insert_replaces_an_incremental_map(gpu, ab):
    a, b, snap_a, _ = ab
    ca, cb = _cloud(gpu, a["points"], a["covs"], a["intensities"]), _cloud(gpu, b["points"], b["covs"], b["intensities"])
    lib = gpu.load()
    one = gpu.GaussianVoxelMapGPU(0.5, target_points_drop_rate=0.0)
    one.insert(ca)
    rc = lib.gp_voxelmap_insert_incremental(one._h, cb.ptr(cb.points_gpu), cb.ptr(cb.covs_gpu), None, cb.size())
    assert rc == INVALID and b"holds no sums" in lib.gp_last_error()
    assert lib.gp_voxelmap_download_stamps(one._h, None) == INVALID
    assert one.voxelmap_info.num_voxels == snap_a.num_voxels
    # a plain insert on an incremental map replaces it, resets the counter and drops the sums: the map is a one-shot map
    vm = _new(gpu, 0.5, 7, 3)
    vm.insert(ca)
    vm.insert(cb)
    assert vm.lru_counter == 2
    with_sums = vm.memory_usage_gpu()
    vm.replace(ca)
    assert vm.lru_counter == 0 and (vm.lru_horizon, vm.lru_clear_cycle) == (7, 3)
    for x, y in zip(vm.download_f64(), one.download_f64()):
        assert x.tobytes() == y.tobytes()
    assert vm.memory_usage_gpu() == one.memory_usage_gpu() < with_sums
    with pytest.raises(gpu._capi.GPError):
        vm.insert(cb)
    empty = _cloud(gpu, vr.bad_rows(), np.zeros((len(vr.bad_rows()), 9)))
    vm.replace(empty)  # an empty one-shot map holds no voxels: an incremental map may start from it
    vm.insert(ca)
    assert vm.lru_counter == 1
    _check(gpu, vm, snap_a, "incremental again", lookup=(ca, a["points"]))

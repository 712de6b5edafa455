"""voxelgrid_sampling_gpu / randomgrid_sampling_gpu / sample_gpu on the device against tests/sampling_ref.py (the numpy restatement of
point_cloud_cpu_funcs.cpp:27-75, 119-295, 298-456 with block_size = None: one row per occupied voxel, dropped points in no row).

Bound of every mean (derived, not measured; no point is exempt): |got - ref| <= ulp32(ref) + m 2^-52 sum |x_i| with m the voxel's population -- sampling_ref.row_bound."""
import ctypes as C
import os

import numpy as np
import pytest

import sampling_ref as sr
from test_sampling_ref_cpu import full_scan, scan_attrs

pytestmark = pytest.mark.gpu

ATTRS = ("points", "covs", "normals", "intensities", "times")


def make_frame(gpu, attrs, names=ATTRS):
    f = gpu.PointCloudGPU(device="cuda:0")
    if "points" in names:
        f.add_points(np.ascontiguousarray(attrs["points"], dtype=np.float32))
    if "covs" in names:
        f.add_covs(np.ascontiguousarray(attrs["covs"], dtype=np.float32).reshape(-1, 9))
    if "normals" in names:
        f.add_normals(np.ascontiguousarray(attrs["normals"], dtype=np.float32))
    if "intensities" in names:
        f.add_intensities(attrs["intensities"])
    if "times" in names:
        f.add_times(attrs["times"])
    return f


def rows(cloud, names=ATTRS):
    return {a: getattr(cloud, a + "_gpu").cpu().numpy() for a in names if getattr(cloud, a + "_gpu") is not None}


def synthetic_cloud():
    from gtsam_points_amd import synthetic

    return synthetic.make_c2_workload(1_000_000, 64_000, seed=42)["source_points"]


@pytest.mark.parametrize("case", ["kitti 0.25", "kitti 0.5", "kitti 1.0", "synthetic 1M 0.5"])
def test_voxelgrid_matches_the_restatement(gpu, case):
    cloud = synthetic_cloud() if case.startswith("synthetic") else full_scan()
    res = float(case.split()[-1])
    attrs = scan_attrs(cloud, seed=3)
    frame = make_frame(gpu, attrs)
    gen = frame.generation
    out = gpu.voxelgrid_sampling_gpu(frame, res)
    ref = sr.voxelgrid_reference(cloud, attrs, res)
    assert out.size() == len(ref["keys"]) and out.num_dropped == 0
    got = rows(out)
    assert sorted(got) == sorted(ATTRS)
    figs = sr.assert_voxelgrid(got, ref, what=f"{case} ({len(cloud)} points, largest voxel {int(ref['counts'].max())})")
    assert max(figs.values()) <= 1.0
    assert frame.generation == gen and frame.size() == len(cloud)  # the input is not modified
    assert out.generation > 0 and str(out.points_gpu.device) == "cuda:0"


def test_bit_reproducible_and_independent_of_the_other_attributes(gpu):
    cloud = full_scan()
    attrs = scan_attrs(cloud, seed=4)
    a = rows(gpu.voxelgrid_sampling_gpu(make_frame(gpu, attrs), 0.5))
    b = rows(gpu.voxelgrid_sampling_gpu(make_frame(gpu, attrs), 0.5))
    for k in ATTRS:
        assert a[k].tobytes() == b[k].tobytes(), k
    alone = rows(gpu.voxelgrid_sampling_gpu(make_frame(gpu, attrs, names=("points", "covs")), 0.5))
    assert alone["covs"].tobytes() == a["covs"].tobytes() and sorted(alone) == ["covs", "points"]
    plan = gpu.VoxelGridPlan(make_frame(gpu, attrs), 0.5)  # ... and of how often the plan has been used
    import torch

    covs = torch.from_numpy(attrs["covs"]).to("cuda:0")
    first = plan.average(covs).cpu().numpy()
    plan.average(torch.from_numpy(attrs["intensities"]).to("cuda:0"))
    assert plan.average(covs).cpu().numpy().tobytes() == first.tobytes() == a["covs"].tobytes()
    plan.close()


def test_edge_cases(gpu):
    empty = gpu.voxelgrid_sampling_gpu(gpu.PointCloudGPU(device="cuda:0"), 0.5)
    assert empty.size() == 0 and empty.num_dropped == 0
    e2 = gpu.voxelgrid_sampling_gpu(make_frame(gpu, scan_attrs(np.zeros((0, 3), np.float32))), 0.5)
    assert e2.size() == 0 and e2.points_gpu.shape == (0, 3) and e2.covs_gpu.shape == (0, 9)
    assert gpu.randomgrid_sampling_gpu(gpu.PointCloudGPU(device="cuda:0"), 0.5, 0.5).size() == 0
    p = np.array([[1.25, -3.5, 0.75]], np.float32)
    one = gpu.voxelgrid_sampling_gpu(make_frame(gpu, {"points": p}, names=("points",)), 0.5)
    assert one.size() == 1 and one.points_gpu.cpu().numpy().tobytes() == p.tobytes()
    q = np.array([0.1234567, -7.654321, 3.3333333], np.float32)
    many = gpu.voxelgrid_sampling_gpu(make_frame(gpu, {"points": np.repeat(q[None], 10_000, 0)}, names=("points",)), 0.5)
    assert many.size() == 1 and many.points_gpu.cpu().numpy().tobytes() == q.tobytes()  # (spans 20 tiles of the reduction: the carries are exact too)
    # points exactly on voxel faces: -0.5 at 0.5 m belongs to voxel -1, 0.0 to voxel 0
    faces = np.array([[-0.5, 0.25, 0.25], [-0.25, 0.25, 0.25], [0.0, 0.25, 0.25], [0.25, 0.25, 0.25], [0.5, 0.25, 0.25], [-1.0, 0.25, 0.25], [-0.75, 0.25, 0.25]], np.float32)
    out = gpu.voxelgrid_sampling_gpu(make_frame(gpu, {"points": faces}, names=("points",)), 0.5)
    want = np.array([[-0.875, 0.25, 0.25], [-0.375, 0.25, 0.25], [0.125, 0.25, 0.25], [0.5, 0.25, 0.25]], np.float32)  # voxels x = -2, -1, 0, 1
    assert out.points_gpu.cpu().numpy().tobytes() == want.tobytes()
    sr.assert_voxelgrid(rows(out, ("points",)), sr.voxelgrid_reference(faces, {"points": faces}, 0.5), what="faces")


def test_dropped_points_are_counted_and_change_nothing(gpu):
    cloud = full_scan()[::3].copy()
    attrs = scan_attrs(cloud, seed=5)
    clean = rows(gpu.voxelgrid_sampling_gpu(make_frame(gpu, attrs), 0.5))
    big = np.float32(0.5 * 2 ** 20)
    bad = np.array([[np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [big, 0, 0], [0, -2 * big, 0], [3e38, 3e38, 3e38], [np.nan, np.nan, np.nan]], np.float32)
    at = np.array([0, 5, 17, 1000, 20_000, len(cloud) - 3, len(cloud)])
    dirty_cloud = np.insert(cloud, at, bad, axis=0)
    dirty = {"points": dirty_cloud}
    for a in ATTRS[1:]:
        filler = np.full((len(bad), attrs[a].shape[1]), np.nan, np.float32)  # their other attributes must not leak either
        dirty[a] = np.insert(attrs[a], at, filler, axis=0)
    out = gpu.voxelgrid_sampling_gpu(make_frame(gpu, dirty), 0.5)
    assert out.num_dropped == len(bad)
    got = rows(out)
    for a in ATTRS:
        assert got[a].tobytes() == clean[a].tobytes(), a
    sr.assert_voxelgrid(got, sr.voxelgrid_reference(dirty_cloud, dirty, 0.5), what="with dropped points")
    r = gpu.randomgrid_sampling_gpu(make_frame(gpu, dirty), 0.5, 0.2, seed=9)
    sr.check_randomgrid(dirty_cloud, 0.5, 0.2, r.sample_indices_gpu.cpu().numpy(), what="with dropped points")
    assert r.num_dropped == len(bad)
    only_bad = gpu.voxelgrid_sampling_gpu(make_frame(gpu, {"points": bad}, names=("points",)), 0.5)
    assert only_bad.size() == 0 and only_bad.num_dropped == len(bad)


def test_both_sort_routes_give_one_numbering(gpu):
    """two clusters 2 x 10^5 m apart at 0.1 m: the box needs more than 32 key bits, so the plan sorts twice.  The coordinates are multiples of 2^-6 m, so every f64
    sum is exact and rows can be compared bit for bit."""
    rng = np.random.default_rng(11)
    lib = gpu.load()

    def cluster(n, centre):
        return (np.round(rng.uniform(-6.0, 6.0, size=(n, 3)) * 64.0) / 64.0 + np.asarray(centre)).astype(np.float32)

    A, B = cluster(30_000, (-1.0e5, 0.0, 0.0)), cluster(30_000, (1.0e5, 0.0, 0.0))
    both = np.concatenate([A, B])[rng.permutation(60_000)]
    inten = rng.uniform(0, 255, size=(60_000, 1)).astype(np.float32)
    res = 0.1
    kx = sr.key_coords(sr.voxel_keys(both, res)[0])
    assert float(np.prod(kx.max(0) - kx.min(0) + 1.0)) > 2.0 ** 32
    out = gpu.voxelgrid_sampling_gpu(make_frame(gpu, {"points": both, "intensities": inten}, names=("points", "intensities")), res)
    ref = sr.voxelgrid_reference(both, {"points": both, "intensities": inten}, res)
    assert out.num_dropped == 0
    got = rows(out, ("points", "intensities"))
    sr.assert_voxelgrid(got, ref, what="two far clusters (two-sort route)")
    # each cluster alone (one-sort route), concatenated in key order
    is_a = both[:, 0] < 0
    parts, keys = [], []
    for sel in (is_a, ~is_a):
        o = gpu.voxelgrid_sampling_gpu(make_frame(gpu, {"points": both[sel], "intensities": inten[sel]}, names=("points", "intensities")), res)
        parts.append(rows(o, ("points", "intensities")))
        keys.append(sr.voxelgrid_reference(both[sel], {}, res)["keys"])
        assert o.size() == len(keys[-1])
    order = np.argsort(np.concatenate(keys), kind="stable")
    assert (np.concatenate(keys)[order] == ref["keys"]).all()
    assert np.concatenate([parts[0]["points"], parts[1]["points"]])[order].tobytes() == got["points"].tobytes()
    # the same clusters brought close (a shift by whole voxels: 1 / 0.1 is 10.0 in double and the coordinates are dyadic): the one-sort route, the same numbering
    shift = np.where(is_a, 99_900.0, -99_900.0).astype(np.float32)
    close = both.copy()
    close[:, 0] += shift
    near = rows(gpu.voxelgrid_sampling_gpu(make_frame(gpu, {"points": close, "intensities": inten}, names=("points", "intensities")), res), ("points", "intensities"))
    assert near["points"][:, 1:].tobytes() == got["points"][:, 1:].tobytes() and near["intensities"].tobytes() == got["intensities"].tobytes()
    # ... and the two-sort route forced on an ordinary scan: bit-identical to the one-sort route
    cloud = full_scan()
    attrs = scan_attrs(cloud, seed=6)
    narrow = rows(gpu.voxelgrid_sampling_gpu(make_frame(gpu, attrs), 0.5))
    lib.gp_debug_voxelgrid_hooks(1, 0)
    try:
        wide = rows(gpu.voxelgrid_sampling_gpu(make_frame(gpu, attrs), 0.5))
        ri_wide = gpu.randomgrid_sampling_gpu(make_frame(gpu, attrs), 0.5, 0.2, seed=3).sample_indices_gpu.cpu().numpy()
    finally:
        lib.gp_debug_voxelgrid_hooks(0, 0)
    for a in ATTRS:
        assert wide[a].tobytes() == narrow[a].tobytes(), a
    assert (ri_wide == gpu.randomgrid_sampling_gpu(make_frame(gpu, attrs), 0.5, 0.2, seed=3).sample_indices_gpu.cpu().numpy()).all()


def test_a_faulted_sort_is_run_again_with_one_class(gpu):
    """the bounded-wait protocol of gp_sort.hpp: a sort that reports an expired wait voids the build / the selection, which runs again through the one-class sort"""
    lib = gpu.load()
    cloud = full_scan()
    attrs = scan_attrs(cloud, seed=7)
    good = rows(gpu.voxelgrid_sampling_gpu(make_frame(gpu, attrs), 0.5))
    good_idx = gpu.randomgrid_sampling_gpu(make_frame(gpu, attrs), 0.5, 0.2, seed=5).sample_indices_gpu.cpu().numpy()
    before = lib.gp_debug_voxelgrid_hooks(0, 1)
    out = rows(gpu.voxelgrid_sampling_gpu(make_frame(gpu, attrs), 0.5))
    assert lib.gp_debug_voxelgrid_hooks(0, 0) == before + 1
    for a in ATTRS:
        assert out[a].tobytes() == good[a].tobytes(), a
    plan = gpu.VoxelGridPlan(make_frame(gpu, attrs), 0.5)
    lib.gp_debug_voxelgrid_hooks(0, 1)
    idx = plan.random_indices(0.2, seed=5).cpu().numpy()
    assert lib.gp_debug_voxelgrid_hooks(0, 0) == before + 2 and (idx == good_idx).all()
    lib.gp_debug_voxelgrid_hooks(1, 1)  # the two-sort route's own check
    try:
        wide = rows(gpu.voxelgrid_sampling_gpu(make_frame(gpu, attrs), 0.5))
    finally:
        assert lib.gp_debug_voxelgrid_hooks(0, 0) == before + 3
    assert wide["covs"].tobytes() == good["covs"].tobytes()
    plan.close()


@pytest.mark.parametrize("res,rate", [(1.0, 0.1), (0.5, 0.25), (0.1, 0.5)])
def test_randomgrid_properties(gpu, res, rate):
    cloud = full_scan()
    attrs = scan_attrs(cloud, seed=8)
    frame = make_frame(gpu, attrs)
    figs = sr.randomgrid_figures(cloud, res, rate)
    if (res, rate) == (0.1, 0.5):
        assert figs["V"] * figs["points_per_voxel"] > figs["cap"] and figs["cap_binds"]  # the case where the cap binds
    else:
        assert not figs["cap_binds"]
    a = gpu.randomgrid_sampling_gpu(frame, res, rate, seed=1)
    ia = a.sample_indices_gpu.cpu().numpy()
    ka = sr.check_randomgrid(cloud, res, rate, ia, what=f"{res} m rate {rate} seed 1", figs=figs)
    assert a.size() == len(ia) <= figs["cap"]
    got = rows(a)
    for k in ATTRS:  # every attribute row is the source row at its index, bit for bit
        assert got[k].tobytes() == attrs[k][ia].tobytes(), k
    again = gpu.randomgrid_sampling_gpu(frame, res, rate, seed=1)
    assert again.sample_indices_gpu.cpu().numpy().tobytes() == ia.tobytes()
    for k in ATTRS:
        assert rows(again)[k].tobytes() == got[k].tobytes()
    ib = gpu.randomgrid_sampling_gpu(frame, res, rate, seed=2).sample_indices_gpu.cpu().numpy()
    kb = sr.check_randomgrid(cloud, res, rate, ib, what=f"{res} m rate {rate} seed 2", figs=figs)
    assert not np.array_equal(ia, ib)
    if not figs["cap_binds"]:
        assert (ka == kb).all()
    # the selection is the documented one: per voxel the smallest (hash, index), beyond the cap the smallest of those
    assert np.array_equal(ia, sr.randomgrid_reference(cloud, res, rate, 1)) and np.array_equal(ib, sr.randomgrid_reference(cloud, res, rate, 2))
    print(f"{res} m rate {rate}: kept {len(ia)} of {len(cloud)}, points_per_voxel {figs['points_per_voxel']}, cap {figs['cap']} ({'binds' if figs['cap_binds'] else 'does not bind'})")


def test_randomgrid_rate_one_keeps_every_valid_point_in_order(gpu):
    cloud = full_scan()[::2].copy()
    cloud[[3, 77, 4000]] = np.nan
    frame = make_frame(gpu, {"points": cloud}, names=("points",))
    for rate in (1.0, 0.99):
        out = gpu.randomgrid_sampling_gpu(frame, 0.5, rate, seed=4)
        idx = out.sample_indices_gpu.cpu().numpy()
        assert np.array_equal(idx, np.flatnonzero(np.isfinite(cloud).all(1))) and out.num_dropped == 3
        assert out.points_gpu.cpu().numpy().tobytes() == cloud[idx].tobytes()
    small = full_scan()[:16_385].copy()  # one scan tile and one entry: the stored-flag compaction through its 16-byte loads and its scalar tail
    small[[0, 15, 16, 9000, 16_383, 16_384]] = np.nan
    out = gpu.randomgrid_sampling_gpu(make_frame(gpu, {"points": small}, names=("points",)), 0.5, 1.0, seed=4)
    idx = out.sample_indices_gpu.cpu().numpy()
    assert np.array_equal(idx, np.flatnonzero(np.isfinite(small).all(1))) and out.num_dropped == 6
    assert out.points_gpu.cpu().numpy().tobytes() == small[idx].tobytes()


def test_randomgrid_is_uniform_inside_a_voxel(gpu):
    """one voxel of 64 points, points_per_voxel = ceil(0.25 x 64 / 1) = 16, 4096 seeds: every point's selection count within 5 sigma of 1024,
    sigma = sqrt(4096 x 1/4 x 3/4) = 27.7 -- the binomial's bound, not a run's"""
    rng = np.random.default_rng(2)
    pts = rng.uniform(0.05, 0.95, size=(64, 3)).astype(np.float32)
    plan = gpu.VoxelGridPlan(make_frame(gpu, {"points": pts}, names=("points",)), 1.0)
    assert plan.num_voxels == 1
    counts = np.zeros(64, np.int64)
    for seed in range(4096):
        idx = plan.random_indices(0.25, seed).cpu().numpy()
        assert len(idx) == 16 and (np.diff(idx) > 0).all()
        counts[idx] += 1
    plan.close()
    worst = sr.check_uniform(counts, 4096, 0.25, what="64 points, 16 kept")
    print(f"uniformity: worst deviation {worst:.2f} sigma (bound 5)")


def test_sample_gpu_is_fancy_indexing(gpu):
    cloud = full_scan()[:20_000]
    attrs = scan_attrs(cloud, seed=9)
    frame = make_frame(gpu, attrs)
    rng = np.random.default_rng(1)
    for idx in (rng.integers(0, len(cloud), size=50_000), np.array([5, 5, 5, 0, len(cloud) - 1, 5]), np.arange(len(cloud))[::-1].copy(), np.zeros(0, np.int64)):
        out = gpu.sample_gpu(frame, idx)
        assert out.size() == len(idx)
        got = rows(out)
        for k in ATTRS:
            assert got[k].tobytes() == attrs[k][idx].tobytes(), k
    import torch

    out = gpu.sample_gpu(frame, torch.tensor([3, 1, 2], device="cuda:0"))
    assert out.points_gpu.cpu().numpy().tobytes() == cloud[[3, 1, 2]].tobytes()
    for bad in ([0, len(cloud)], [-1]):
        with pytest.raises(IndexError):
            gpu.sample_gpu(frame, bad)
    few = gpu.sample_gpu(make_frame(gpu, attrs, names=("points", "times")), [1, 2])
    assert few.covs_gpu is None and few.times_gpu.shape == (2, 1)


def test_downsampled_cloud_is_an_ordinary_cloud_to_the_rest_of_the_library(gpu):
    """voxelgrid_sampling_gpu at 0.25 m -> estimate_normals_covariances_gpu -> GaussianVoxelMapGPU.insert -> IntegratedVGICPFactorGPU linearise on the two kitti scans:
    the record equals the one obtained when the downsampled points are downloaded, uploaded again as a fresh PointCloudGPU and taken through the same steps"""
    from gtsam_points_amd import _capi
    from gtsam_points_amd.types import _pose16

    def record(clouds):
        tgt, src = clouds
        for c in clouds:
            assert gpu.estimate_normals_covariances_gpu(c, 10) >= 0
        vm = gpu.GaussianVoxelMapGPU(1.0, target_points_drop_rate=0.0)
        vm.insert(tgt)
        f = gpu.IntegratedVGICPFactorGPU(0, 1, vm, src)
        rec = _capi.Linearized6()
        _capi.check(f._lib.gp_vgicp_factor_linearize(f._h, _pose16(np.eye(4)), C.byref(rec)), "gp_vgicp_factor_linearize")
        return rec

    down = [gpu.voxelgrid_sampling_gpu(gpu.PointCloudGPU(full_scan(name), device="cuda:0"), 0.25) for name in ("000000.bin", "000001.bin")]
    fresh = [gpu.PointCloudGPU(d.download("points"), device="cuda:0") for d in down]
    for d, f in zip(down, fresh):
        assert f.points_gpu.cpu().numpy().tobytes() == d.points_gpu.cpu().numpy().tobytes()
    a, b = record(down), record(fresh)
    assert a.num_inliers > 5000
    assert bytes(a) == bytes(b)
    assert down[0].normals_gpu is not None and down[0].covs_gpu.shape == (down[0].size(), 9)
    # offload / reload: the device-only attributes come back bit for bit (the mirror bookkeeping of an adopted cloud)
    keep = down[1].points_gpu.cpu().numpy().copy()
    gen = down[1].generation
    assert down[1].offload_gpu() and not down[1].loaded_on_gpu() and down[1].reload_gpu()
    assert down[1].points_gpu.cpu().numpy().tobytes() == keep.tobytes() and down[1].generation > gen

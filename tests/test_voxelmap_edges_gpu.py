"""Edge tests of the voxel-map BUILD against tests/voxelmap_ref.py (numpy f64 / math.fsum on the f32 inputs): the binned build (gp_binning.hip,
segmented_stats_kernel), the hashed build (GP_TUNE_MAP_BUILD = 1, and the automatic fallback of boxes above 2^24 blocks), assign / save_compact / load,
offload / reload.  tests/test_voxelmap_ref_cpu.py checks the cases' preconditions without a GPU.

Tolerances, from the stored formats only (res = leaf, n = points of the voxel):
  download_f64 means   res * 2^-24 + n * 2^-52 * res      mean_local is an f32 of magnitude <= res / 2 (half an ulp <= res * 2^-25), each of the n additions of an
                                                          offset |p - centre| <= res rounds by <= 2^-53 of a partial sum <= n res ... taken as n * 2^-52 * res
  download_f64 covs    n * 2^-52 * max|c|                 n f64 additions of terms <= max|c|, one division
  f32 arrays           the above + 2^-24 * |value|        one f32 rounding of the f64 value
Where the inputs are exact (case a) the comparison is bit for bit.
Measured worst ratios to these bounds on an MI355X, both builds alike: case (c) at 0 / 1e2 / 1e3 / 1e4 / 1e5 m -- means64 0.31 / 0.25 / 0.25 / 0.25 / 0.25,
means32 0.95 / 0.64 / 0.51 / 0.82 / 0.66, covs32 1.00 at every distance (an f32 rounding of exactly half an ulp, never above), covs64 < 0.001; over all cases
means64 <= 0.40, means32 and covs32 <= 1.00.  Every test prints its own figures."""
import ctypes as C
import os

import numpy as np
import pytest

import voxelmap_ref as vr
from helpers import reference_bucket_lookup

pytestmark = pytest.mark.gpu

BUILDS = ("binned", "hashed")
GP_ERROR_IO = 4  # include/gtsam_points_hip.h


def _cloud(gpu, case):
    """the case's f32 arrays on the device exactly as they are (no conversion on the way)"""
    import torch

    it = case["intensities"]
    return gpu.PointCloudGPU.from_device(
        torch.from_numpy(case["points"].copy()).to("cuda:0"),
        torch.from_numpy(case["covs"].copy()).to("cuda:0"),
        torch.from_numpy(it.copy()).to("cuda:0") if it is not None else None,
    )


def _new_map(gpu, res, build):
    vm = gpu.GaussianVoxelMapGPU(res, target_points_drop_rate=0.0)
    if build == "hashed":
        gpu._capi.check(gpu.load().gp_voxelmap_set_tuning(vm._h, gpu._capi.GP_TUNE_MAP_BUILD, 1), "gp_voxelmap_set_tuning")
    return vm


def _build(gpu, case, build):
    cloud = _cloud(gpu, case)
    vm = _new_map(gpu, case["res"], build)
    vm.insert(cloud)
    return vm, cloud


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _check(gpu, vm, ref, what, exact=False, lookup_cloud=None, buckets_stride=1):
    """the map against the restatement: voxel set, counts, f64 and f32 statistics, intensities, bucket table, lookup.  Returns the worst ratios to the bounds."""
    info = vm.voxelmap_info
    assert info.num_voxels == ref.num_voxels, f"{what}: {info.num_voxels} voxels, the restatement has {ref.num_voxels}"
    coords, counts, means, covs = vm.download_f64()
    dl = vm.download()
    if ref.num_voxels == 0:
        assert (dl["buckets"][:, 3] < 0).all()
        return {}
    missing = [tuple(c) for c in coords.tolist() if tuple(c) not in ref.index]
    assert not missing, f"{what}: voxels the restatement does not have: {missing[:5]}"
    idx = np.array([ref.index[tuple(c)] for c in coords.tolist()])
    assert len(set(idx.tolist())) == ref.num_voxels, f"{what}: a voxel is listed twice"
    np.testing.assert_array_equal(counts, ref.counts[idx], err_msg=f"{what}: counts")
    np.testing.assert_array_equal(dl["num_points"], ref.counts[idx], err_msg=f"{what}: num_points")
    for name, a in (("means64", means), ("covs64", covs), ("means32", dl["means"]), ("covs32", dl["covs"]), ("intensities", dl["intensities"])):
        assert np.isfinite(a).all() or name == "intensities", f"{what}: {name} holds a non-finite entry"
    n = ref.counts[idx].astype(np.float64)
    res = ref.res
    want_int = ref.intensities[idx]
    assert np.array_equal(_bits(dl["intensities"]), _bits(want_int)), (
        f"{what}: intensities differ in {(_bits(dl['intensities']) != _bits(want_int)).sum()} voxels, e.g. "
        f"{dl['intensities'][_bits(dl['intensities']) != _bits(want_int)][:4]} for {want_int[_bits(dl['intensities']) != _bits(want_int)][:4]}"
    )
    ratios = {}
    if exact:
        for name, got, want in (
            ("means64", means, ref.means_stored[idx]),
            ("covs64", covs, ref.covs[idx]),
            ("means32", dl["means"], ref.means[idx].astype(np.float32)),
            ("covs32", dl["covs"], ref.covs[idx].astype(np.float32)),
        ):
            bad = np.flatnonzero((_bits(got) != _bits(want)).reshape(len(idx), -1).any(axis=1))
            assert len(bad) == 0, (
                f"{what}: {name} differs in {len(bad)} voxels; first: voxel {bad[0]} coord {coords[bad[0]].tolist()} n = {int(n[bad[0]])} "
                f"got {got[bad[0]].ravel()[:3]} want {want[bad[0]].ravel()[:3]}"
            )
    else:
        bm = (res * 2.0**-24 + n * 2.0**-52 * res)[:, None]
        bc = (n * 2.0**-52 * ref.max_abs_cov[idx])[:, None, None]
        ratios["means64"] = float((np.abs(means - ref.means[idx]) / bm).max())
        ratios["covs64"] = float((np.abs(covs - ref.covs[idx]) / bc).max())
        ratios["means32"] = float((np.abs(dl["means"].astype(np.float64) - ref.means[idx]) / (bm + 2.0**-24 * np.abs(ref.means[idx]))).max())
        ratios["covs32"] = float((np.abs(dl["covs"].astype(np.float64) - ref.covs[idx]) / (bc + 2.0**-24 * np.abs(ref.covs[idx]))).max())
        print(f"{what}: worst ratio to the bound " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
        for k, v in ratios.items():
            assert v <= 1.0, f"{what}: {k} exceeds its bound by a factor {v:.3f}"
    # the downloaded bucket table finds every voxel
    b = dl["buckets"]
    used = b[b[:, 3] >= 0]
    assert sorted(used[:, 3].tolist()) == list(range(info.num_voxels)), f"{what}: bucket table"
    for v in list(range(0, info.num_voxels, buckets_stride)) + [info.num_voxels - 1]:
        assert reference_bucket_lookup(b, info, coords[v]) == v, f"{what}: voxel {v} not found through the bucket table"
    if lookup_cloud is not None:
        got = vm.lookup(lookup_cloud)
        want = np.where(ref.point_voxel >= 0, np.argsort(idx)[np.maximum(ref.point_voxel, 0)], -1)
        wrong = np.flatnonzero(got != want)
        assert len(wrong) == 0, f"{what}: lookup names another voxel for {len(wrong)} points, first row {wrong[0]}: {got[wrong[0]]} for {want[wrong[0]]}"
    return ratios


def _ref(case):
    return vr.Map(case["points"], case["covs"], case["intensities"], case["res"])


def _has_grid(gpu, vm):
    return gpu.load().gp_voxelmap_has_block_grid(vm._h)


# ---- (a) exact arithmetic, batch and lane phases ------------------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def exact():
    case = vr.case_exact_phases()
    return case, _ref(case)


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reversed"])
def test_a_exact_sums_at_every_lane_phase_and_batch_boundary(gpu, exact, build, reverse):
    """populations 1 .. 5000 behind k = 0 .. 16 one-point voxels of the same workgroup (voxelmap_ref.case_exact_phases): every sum is exact in f64, so mean_local,
    covs and the f32 arrays equal the restatement's bit for bit -- a row dropped or counted twice at one lane phase changes a count-weighted sum by >= 2^-6 / n"""
    case, ref = exact
    if reverse:
        case = vr.case_exact_phases(reverse=True)  # (the same map: tests/test_voxelmap_ref_cpu.py)
    vm, cloud = _build(gpu, case, build)
    assert _has_grid(gpu, vm) == 1
    _check(gpu, vm, ref, f"exact {build}", exact=True, buckets_stride=7)
    if build == "binned":  # the voxel numbering is the (block, bit) order the layout of the case rests on
        np.testing.assert_array_equal(vm.download_f64()[0], case["voxel_order"])


# ---- (b) faces and signs ---------------------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("res", vr.FACE_RESOLUTIONS)
def test_b_faces_and_signs(gpu, res, build):
    case = vr.case_faces(res)
    vm, cloud = _build(gpu, case, build)
    _check(gpu, vm, _ref(case), f"faces {res} {build}", lookup_cloud=cloud)


# ---- (c) far from the origin -----------------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("res", [0.5, 0.1])
def test_c_accuracy_does_not_depend_on_the_distance(gpu, res, build):
    """the same patch at 0 .. 1e5 m: the bounds of the module docstring hold whatever the distance, because the mean is kept as an f32 offset from the voxel centre"""
    for d in vr.FAR_DISTANCES:
        case = vr.case_far(d, res)
        vm, cloud = _build(gpu, case, build)
        _check(gpu, vm, _ref(case), f"far d={d:g} res={res} {build}", lookup_cloud=cloud, buckets_stride=5)


# ---- (d) every sort width ----------------------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", vr.WIDTH_CASES)
def test_d_every_sort_width_and_the_fallback(gpu, name):
    case = vr.case_width(name)
    assert vr.predicted_path(case["points"], case["res"]) == case["path"]
    vm, cloud = _build(gpu, case, "binned")
    assert _has_grid(gpu, vm) == (0 if case["path"] == "hashed" else 1)
    _check(gpu, vm, _ref(case), f"width {name}", lookup_cloud=cloud, buckets_stride=11)


# ---- (e) non-finite and out-of-range points ----------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("which", ["binned", "hashed", "fallback"])
def test_e_invalid_points_belong_to_no_voxel(gpu, which):
    case = vr.case_invalid(fallback=which == "fallback")
    keep = case["keep"]
    cut = vr.Map(case["points"][keep], case["covs"][keep], case["intensities"][keep], case["res"])
    vm, cloud = _build(gpu, case, "hashed" if which == "hashed" else "binned")
    ref = _ref(case)
    assert ref.coords.tobytes() == cut.coords.tobytes() and ref.means.tobytes() == cut.means.tobytes()
    _check(gpu, vm, ref, f"invalid rows, {which}", lookup_cloud=cloud, buckets_stride=3)
    assert _has_grid(gpu, vm) == (0 if which == "fallback" else 1)
    dl = vm.download()
    for k in ("means", "covs", "intensities"):
        assert np.isfinite(dl[k]).all(), k
    assert dl["num_points"].sum() == keep.sum()


@pytest.mark.parametrize("build", BUILDS)
def test_e_cloud_without_a_valid_point(gpu, build):
    case = vr.case_all_invalid()
    vm, cloud = _build(gpu, case, build)
    assert vm.voxelmap_info.num_voxels == 0
    _check(gpu, vm, _ref(case), f"no valid point, {build}")
    assert (vm.lookup(cloud) == -1).all()


# ---- (f) intensities -------------------------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("build", BUILDS)
def test_f_intensity_rule(gpu, build):
    """negative, zero, -0.0, very large, infinite and NaN intensities: both builds give the CPU map's std::max from 0.0, bit for bit; no intensities: 0.0"""
    case = vr.case_intensities()
    vm, cloud = _build(gpu, case, build)
    _check(gpu, vm, _ref(case), f"intensities {build}")
    none = dict(case, intensities=None)
    vm, cloud = _build(gpu, none, build)
    _check(gpu, vm, _ref(none), f"no intensities {build}")
    assert (_bits(vm.download()["intensities"]) == 0).all()


# ---- (g) re-insertion --------------------------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("which", ["A larger", "A smaller", "B empty"])
def test_g_insert_replaces_the_map(gpu, build, which):
    """GaussianVoxelMapGPU::insert builds a new table and new, zeroed arrays (gaussian_voxelmap_gpu.cu:217-225, 295-296): a second insert leaves the map of the
    second cloud alone"""
    a, b = vr.case_reinsert("A larger" if which == "B empty" else which)
    vm = _new_map(gpu, 0.5, build)
    ca, cb = _cloud(gpu, a), _cloud(gpu, b)
    vm.insert(ca)
    assert vm.voxelmap_info.num_voxels == _ref(a).num_voxels
    if which == "B empty":
        cb.num_points = 0
        vm.insert(cb)
        assert vm.voxelmap_info.num_voxels == 0 and (vm.download()["buckets"][:, 3] < 0).all()
        assert (vm.lookup(ca) == -1).all()
        return
    vm.insert(cb)
    _check(gpu, vm, _ref(b), f"re-insert {which} {build}", lookup_cloud=cb, buckets_stride=3)
    alone, _ = _build(gpu, b, build)
    if build == "binned":  # deterministic: the very same map
        for x, y in zip(vm.download_f64(), alone.download_f64()):
            assert x.tobytes() == y.tobytes()


# ---- (h) file and assign edges ----------------------------------------------------------------------------------------------------------------------------------------


def _same_map(m1, m2, what):
    """voxel set, counts and f32 arrays bit for bit (the voxel numbering may differ)"""
    c1, c2 = m1.download_f64()[0], m2.download_f64()[0]
    assert len(c1) == len(c2), what
    o1 = {tuple(c): i for i, c in enumerate(c1.tolist())}
    idx = np.array([o1[tuple(c)] for c in c2.tolist()], dtype=np.int64)
    assert len(set(idx.tolist())) == len(c1), what
    d1, d2 = m1.download(), m2.download()
    for k in ("num_points", "means", "covs", "intensities"):
        assert d1[k][idx].tobytes() == d2[k].tobytes(), f"{what}: {k}"
    return idx


@pytest.mark.parametrize("far", [False, True], ids=["near", "far"])
@pytest.mark.parametrize("res", [0.5, 0.3, 0.123456789])
def test_h_save_load_round_trip(gpu, tmp_path, res, far):
    case = vr.case_file(res, far)
    vm, cloud = _build(gpu, case, "binned")
    path = os.path.join(tmp_path, "map.bin")
    vm.save_compact(path)
    vm2 = gpu.GaussianVoxelMapGPU.load(path)
    assert vm2 is not None
    assert vm2.voxel_resolution() == vm.voxel_resolution() == res, f"resolution {vm2.voxel_resolution()!r} after the round trip, {res!r} before"
    idx = _same_map(vm, vm2, f"round trip {res}")
    got, want = vm2.lookup(cloud), vm.lookup(cloud)
    assert (want >= 0).all() and np.array_equal(idx[got], want)
    # the gather records are rebuilt from the f32 means and the resolution: the same offsets from the same centres, to the f32 rounding of the file's mean
    m1, m2 = vm.download_f64()[2], vm2.download_f64()[2]
    assert np.abs(m1[idx] - m2).max() <= 2.0**-23 * np.abs(m1).max() + res * 2.0**-23


@pytest.mark.parametrize("build", BUILDS)
def test_h_zero_voxel_map_round_trips(gpu, tmp_path, build):
    case = vr.case_all_invalid()
    vm, cloud = _build(gpu, case, build)
    path = os.path.join(tmp_path, "empty.bin")
    vm.save_compact(path)
    vm2 = gpu.GaussianVoxelMapGPU.load(path)
    assert vm2 is not None and vm2.voxelmap_info.num_voxels == 0 and vm2.voxel_resolution() == 0.5
    assert (vm2.lookup(cloud) == -1).all()


def test_h_load_refuses_malformed_files(gpu, tmp_path):
    case = vr.case_file(0.5, False)
    vm, cloud = _build(gpu, case, "binned")
    good = os.path.join(tmp_path, "good.bin")
    vm.save_compact(good)
    raw = open(good, "rb").read()
    assert b"voxel_bytes 56\n" in raw
    V = vm.voxelmap_info.num_voxels
    variants = {
        "truncated": raw[: len(raw) - 56 * (V // 2) - 7],
        "voxel_bytes": raw.replace(b"voxel_bytes 56\n", b"voxel_bytes 60\n"),
        "negative": raw.replace(b"num_voxels %d\n" % V, b"num_voxels -3\n"),
        "header only": raw[: raw.index(b"voxel_bytes")],
    }
    lib = gpu.load()
    for name, data in variants.items():
        assert data != raw
        path = os.path.join(tmp_path, name.replace(" ", "_") + ".bin")
        open(path, "wb").write(data)
        h = C.c_void_p()
        rc = lib.gp_voxelmap_load(path.encode(), None, C.byref(h))
        assert rc == GP_ERROR_IO, f"{name}: rc = {rc}"
        assert not h.value, f"{name}: a map was handed out with the error"


def _assign(gpu, res, coords, counts, means, covs6, ints):
    vm = gpu.GaussianVoxelMapGPU(res)
    a = [np.ascontiguousarray(coords, dtype=np.int32), np.ascontiguousarray(counts, dtype=np.int32), np.ascontiguousarray(means, dtype=np.float32),
         np.ascontiguousarray(covs6, dtype=np.float32), np.ascontiguousarray(ints, dtype=np.float32)]
    gpu._capi.check(gpu.load().gp_voxelmap_assign(vm._h, len(a[0]), *[x.ctypes.data for x in a]), "gp_voxelmap_assign")
    return vm, a


@pytest.mark.parametrize("which", ["duplicates", "too large", "empty"])
def test_h_assign_without_a_grid(gpu, which):
    """gp_voxelmap_assign of a coordinate list with a repeated coordinate (no canonical numbering: no grid), of one whose box exceeds 2^24 blocks, and of none:
    lookups and a VGICP factor (the hashed kernel family: the map has no block grid) find every voxel"""
    rng = np.random.default_rng(19)
    res = 0.5
    if which == "empty":
        vm, _ = _assign(gpu, res, np.zeros((0, 3)), np.zeros(0), np.zeros((0, 3)), np.zeros((0, 6)), np.zeros(0))
        assert vm.voxelmap_info.num_voxels == 0 and _has_grid(gpu, vm) == 0
        probe = gpu.PointCloudGPU(np.zeros((3, 3), np.float32))
        assert (vm.lookup(probe) == -1).all()
        return
    coords = rng.integers(-20, 20, size=(300, 3))
    coords = np.unique(coords, axis=0)
    if which == "duplicates":
        coords = np.concatenate([coords, coords[:5]])
    else:
        coords = np.concatenate([coords, coords[:40] + 40000])
    V = len(coords)
    means = ((coords + rng.uniform(0.2, 0.8, size=(V, 3))) * res).astype(np.float32)
    covs6 = np.tile(np.array([0.01, 0, 0, 0.01, 0, 0.01], np.float32), (V, 1))
    vm, _ = _assign(gpu, res, coords, np.full(V, 4), means, covs6, np.arange(V))
    assert vm.voxelmap_info.num_voxels == V and _has_grid(gpu, vm) == 0
    assert (vr.voxel_coords(means, res) == coords).all()
    src = gpu.PointCloudGPU(means, np.tile(np.eye(3, dtype=np.float32) * 0.01, (V, 1, 1)))
    got = vm.lookup(src)
    assert (got >= 0).all()
    np.testing.assert_array_equal(vm.download_f64()[0][got], coords)  # the voxel named holds the point (one of the two, for a repeated coordinate)
    if which == "too large":
        np.testing.assert_array_equal(got, np.arange(V))
    f = gpu.IntegratedVGICPFactorGPU(0, 1, vm, src)
    rec = gpu._capi.Linearized6()
    gpu._capi.check(f._lib.gp_vgicp_factor_linearize(f._h, gpu.types._pose16(np.eye(4)), C.byref(rec)), "linearize")
    assert gpu.LinearizedSystem6(rec).num_inliers == V


@pytest.mark.parametrize("build", BUILDS)
def test_h_offload_reload_and_clone_are_bit_identical(gpu, build):
    case = vr.case_file(0.3, True)
    vm, cloud = _build(gpu, case, build)
    before = [x.copy() for x in vm.download_f64()] + [vm.download()[k].copy() for k in ("buckets", "num_points", "means", "covs", "intensities")]
    look = vm.lookup(cloud)

    def same(m, what):
        after = list(m.download_f64()) + [m.download()[k] for k in ("buckets", "num_points", "means", "covs", "intensities")]
        for x, y in zip(before, after):
            assert x.tobytes() == y.tobytes(), what
        assert np.array_equal(m.lookup(cloud), look), what

    assert vm.offload_gpu() and vm.reload_gpu()
    same(vm, "offload -> reload")
    h = C.c_void_p()
    rc = gpu.load().gp_voxelmap_clone_to_device(vm._h, 0, None, C.byref(h))
    if rc != 0:
        pytest.skip("gp_voxelmap_clone_to_device refuses a clone to the map's own device: " + gpu.load().gp_last_error().decode())
    same(gpu.GaussianVoxelMapGPU(0.3, _handle=h), "clone to the same device")


def test_h_offload_reload_and_clone_without_a_grid_are_bit_identical(gpu):
    """the same paths for a map WITHOUT a block grid (the "too large" input of test_h_assign_without_a_grid: its line table is built at assign): a reload builds the
    line table again and a clone copies it, and the hashed kernel family of a VGICP factor on the clone finds every voxel through it"""
    rng = np.random.default_rng(19)
    res = 0.5
    coords = np.unique(rng.integers(-20, 20, size=(300, 3)), axis=0)
    coords = np.concatenate([coords, coords[:40] + 40000])
    V = len(coords)
    means = ((coords + rng.uniform(0.2, 0.8, size=(V, 3))) * res).astype(np.float32)
    covs6 = np.tile(np.array([0.01, 0, 0, 0.01, 0, 0.01], np.float32), (V, 1))
    vm, _ = _assign(gpu, res, coords, np.full(V, 4), means, covs6, np.arange(V))
    assert vm.voxelmap_info.num_voxels == V and _has_grid(gpu, vm) == 0
    src = gpu.PointCloudGPU(means, np.tile(np.eye(3, dtype=np.float32) * 0.01, (V, 1, 1)))
    before = [x.copy() for x in vm.download_f64()] + [vm.download()[k].copy() for k in ("buckets", "num_points", "means", "covs", "intensities")]
    look = vm.lookup(src)
    np.testing.assert_array_equal(look, np.arange(V))

    def same(m, what):
        assert _has_grid(gpu, m) == 0, what
        after = list(m.download_f64()) + [m.download()[k] for k in ("buckets", "num_points", "means", "covs", "intensities")]
        for x, y in zip(before, after):
            assert x.tobytes() == y.tobytes(), what
        assert np.array_equal(m.lookup(src), look), what

    assert vm.offload_gpu() and vm.reload_gpu()
    same(vm, "offload -> reload")
    h = C.c_void_p()
    rc = gpu.load().gp_voxelmap_clone_to_device(vm._h, 0, None, C.byref(h))
    if rc != 0:
        pytest.skip("gp_voxelmap_clone_to_device refuses a clone to the map's own device: " + gpu.load().gp_last_error().decode())
    clone = gpu.GaussianVoxelMapGPU(res, _handle=h)
    same(clone, "clone to the same device")
    f = gpu.IntegratedVGICPFactorGPU(0, 1, clone, src)
    rec = gpu._capi.Linearized6()
    gpu._capi.check(f._lib.gp_vgicp_factor_linearize(f._h, gpu.types._pose16(np.eye(4)), C.byref(rec)), "linearize")
    assert gpu.LinearizedSystem6(rec).num_inliers == V

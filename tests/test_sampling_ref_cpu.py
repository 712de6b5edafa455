"""tests/sampling_ref.py checked without a GPU: the restatement is consistent with itself, its helper rejects what it must, and the C entry points refuse bad
arguments before any device work -- so a failure of tests/test_sampling_gpu.py means the kernels.

The optional fixture of the issue -- the output of the reference's own voxelgrid_sampling with num_threads = 1 -- is not recorded: point_cloud_cpu_funcs.cpp does not compile
against the stand-in headers under oracle/ref_shim as they are (their Eigen::Array has no isFinite() and no array-with-scalar operators, which its key computation
at :132-137 uses).  The restatement with line citations stands alone, as normals_ref.py does."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import sampling_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW_SYMBOLS = ("gp_voxelgrid_plan_create", "gp_voxelgrid_plan_info", "gp_voxelgrid_plan_average", "gp_voxelgrid_plan_random_indices", "gp_voxelgrid_plan_destroy",
               "gp_cloud_gather")


def full_scan(name="000000.bin"):
    return np.fromfile(os.path.join(GOLDEN, "kitti_00", name), dtype=np.float32).reshape(-1, 3)


def scan_attrs(cloud, seed=0):
    """all five attributes for a cloud: deterministic, of the magnitudes the real ones have"""
    rng = np.random.default_rng(seed)
    n = len(cloud)
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    a = rng.normal(size=(n, 3, 3)) * 0.05
    covs = a @ a.transpose(0, 2, 1) + 1e-3 * np.eye(3)
    return dict(points=cloud.astype(np.float32), covs=covs.reshape(n, 9).astype(np.float32), normals=nrm.astype(np.float32),
                intensities=rng.uniform(0.0, 255.0, size=(n, 1)).astype(np.float32), times=np.linspace(0.0, 0.1, n, dtype=np.float32).reshape(n, 1))


@pytest.mark.parametrize("resolution", [0.25, 0.5, 1.0])
def test_literal_blocks_collapse_onto_one_row_per_voxel(resolution):
    cloud = full_scan()
    attrs = scan_attrs(cloud)
    lit = sr.voxelgrid_reference(cloud, attrs, resolution, block_size=1024)
    one = sr.voxelgrid_reference(cloud, attrs, resolution, block_size=None)
    extra = len(lit["keys"]) - len(one["keys"])
    assert 0 <= extra <= math.ceil(len(cloud) / 1024) - 1, extra
    col = sr.collapse_blocks(lit)
    assert (col["keys"] == one["keys"]).all() and (col["counts"] == one["counts"]).all()
    for a in attrs:
        # merging the block rows re-associates the f64 sum: m roundings of relative size 2^-53 on sum |x| at most, twice (split sums, weighted merge)
        tol = 4.0 * one["counts"][:, None] * 2.0 ** -53 * one["abs_sums"][a] + 1e-300
        assert (np.abs(col["means"][a] - one["means"][a]) <= tol).all(), a
    print(f"kitti_00/000000.bin at {resolution} m: {len(one['keys'])} voxels, {extra} rows more in the literal form, largest voxel {int(one['counts'].max())} points")


def test_key_order_is_lexicographic_zyx():
    cloud = np.concatenate([full_scan(), -full_scan()[::7]])  # negative coordinates on every axis too
    ref = sr.voxelgrid_reference(cloud, {}, 0.5)
    xyz = sr.key_coords(ref["keys"])
    lex = np.lexsort((xyz[:, 0], xyz[:, 1], xyz[:, 2]))  # last key is the primary one: z, then y, then x
    assert (lex == np.arange(len(xyz))).all()
    assert (np.diff(ref["keys"]) > 0).all()
    # the floor rule on voxel faces: -0.5 at 0.5 m belongs to voxel -1, 0.0 to voxel 0
    k, ok = sr.voxel_keys(np.array([[-0.5, 0.0, 0.5], [-0.50001, -1e-9, 0.49999]], np.float32), 0.5)
    assert ok.all() and (sr.key_coords(k) == [[-1, 0, 1], [-2, -1, 0]]).all()


def test_invalid_rule():
    big = np.float32(0.5 * 2 ** 20)
    pts = np.array([[0, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [big, 0, 0], [np.nextafter(big, np.float32(0)), 0, 0], [-big, 0, 0],
                    [np.nextafter(-big, np.float32(-np.inf)), 0, 0], [3e38, 0, 0]], np.float32)
    _, ok = sr.voxel_keys(pts, 0.5)
    assert ok.tolist() == [True, False, False, False, False, True, True, False, False]
    lit = sr.voxelgrid_reference(pts, {"points": pts}, 0.5, block_size=1024)
    assert lit["keys"][-1] == sr.INVALID_KEY and lit["counts"][-1] == 6  # the reference's trailing invalid group
    assert len(sr.voxelgrid_reference(pts, {"points": pts}, 0.5)["keys"]) == 3


def test_helper_rejects_and_names_the_voxel():
    cloud = full_scan()[::4]
    attrs = scan_attrs(cloud)
    ref = sr.voxelgrid_reference(cloud, attrs, 0.5)
    good = {a: m.astype(np.float32) for a, m in ref["means"].items()}
    figs = sr.assert_voxelgrid(good, ref, what="the restatement itself")
    assert max(figs.values()) <= 1.0
    v = int(np.flatnonzero(ref["counts"] > 3)[5])
    off = {a: g.copy() for a, g in good.items()}
    x = off["points"][v, 1]
    off["points"][v, 1] = np.nextafter(np.nextafter(x, np.float32(np.inf)), np.float32(np.inf))  # 2 f32 ulps
    with pytest.raises(AssertionError, match=f"points: voxel {v} "):
        sr.assert_voxelgrid(off, ref, quiet=True)
    missing = {a: np.delete(g, v, axis=0) for a, g in good.items()}
    with pytest.raises(AssertionError, match=f"voxel {v} "):
        sr.assert_voxelgrid(missing, ref, quiet=True)
    last = {a: g[:-1] for a, g in good.items()}
    with pytest.raises(AssertionError, match=f"voxel {len(ref['keys']) - 1} is missing"):
        sr.assert_voxelgrid(last, ref, quiet=True)
    swapped = {a: g.copy() for a, g in good.items()}
    for g in swapped.values():
        g[[v, v + 1]] = g[[v + 1, v]]
    with pytest.raises(AssertionError, match=f"voxel {v} "):
        sr.assert_voxelgrid(swapped, ref, quiet=True)


def test_randomgrid_restatement_passes_its_own_checks():
    cloud = full_scan()
    for res, rate in [(1.0, 0.1), (0.5, 0.25), (0.1, 0.5), (0.5, 1.0)]:
        figs = sr.randomgrid_figures(cloud, res, rate)
        a = sr.randomgrid_reference(cloud, res, rate, seed=1)
        b = sr.randomgrid_reference(cloud, res, rate, seed=2)
        ka = sr.check_randomgrid(cloud, res, rate, a, what=f"{res} m rate {rate}", figs=figs)
        kb = sr.check_randomgrid(cloud, res, rate, b, figs=figs)
        if rate < 0.99:
            assert not np.array_equal(a, b)
        if not figs["cap_binds"]:
            assert (ka == kb).all()
        print(f"{res} m, rate {rate}: {figs['V']} voxels, points_per_voxel {figs['points_per_voxel']}, cap {figs['cap']}, uncapped {figs['uncapped_total']}, kept {len(a)}")
    # the case tests/test_sampling_gpu.py uses for a binding cap
    f = sr.randomgrid_figures(cloud, 0.1, 0.5)
    assert f["V"] * f["points_per_voxel"] > f["cap"] and f["cap_binds"]
    bad = sr.randomgrid_reference(cloud, 1.0, 0.1, seed=1)
    with pytest.raises(AssertionError, match="strictly ascending"):
        sr.check_randomgrid(cloud, 1.0, 0.1, bad[::-1])
    with pytest.raises(AssertionError, match="keeps"):
        sr.check_randomgrid(cloud, 1.0, 0.1, bad[1:])


def test_rank_hash_matches_the_library_and_is_uniform():
    """the numpy restatement of the rank hash equals the library's (host code), and ranking 64 points by it selects every point equally often over 4096 seeds:
    within 5 sigma of 1024, sigma = sqrt(4096 / 4 * 3 / 4) = 27.7 (the bound the GPU test holds the device to)"""
    from gtsam_points_amd import _capi

    lib = _capi.load()
    idx = np.array([0, 1, 2, 63, 64, 12345, 2 ** 31 - 1, 2 ** 32 - 1], np.uint64)
    for seed in (0, 1, 2, 4095, 2 ** 32, 2 ** 64 - 1, 0x123456789ABCDEF):
        want = [lib.gp_debug_sample_hash(seed, int(i)) for i in idx]
        assert sr.sample_hash(seed, idx).tolist() == want, seed
    counts = np.zeros(64, np.int64)
    for seed in range(4096):
        h = sr.sample_hash(seed, np.arange(64)).astype(np.int64)
        counts[np.lexsort((np.arange(64), h))[:16]] += 1
    worst = sr.check_uniform(counts, 4096, 0.25, what="64 points, 16 kept")
    print(f"rank hash: worst deviation {worst:.2f} sigma")
    with pytest.raises(AssertionError, match="point 3 "):
        skew = np.full(64, 1024)
        skew[3] = 1024 + 140
        sr.check_uniform(skew, 4096, 0.25)


def test_header_and_binding_table_have_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "gtsam_points_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    from gtsam_points_amd import _capi

    for s in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + s + r"\s*\(", hdr), f"{s} is not declared in include/gtsam_points_hip.h"
        assert s in _capi.EXPORTED_SYMBOLS, f"{s} is not in _capi.EXPORTED_SYMBOLS"
    import gtsam_points_amd as gpa

    assert callable(gpa.sample_gpu) and callable(gpa.voxelgrid_sampling_gpu) and callable(gpa.randomgrid_sampling_gpu)


def test_argument_checks_need_no_device():
    """NULL arrays, a resolution that is not positive and finite, width outside 1 .. 16, a sampling rate outside (0, 1]: GP_ERROR_INVALID_ARGUMENT before any device
    work (this host has no device); num_points == 0 gives a valid empty plan"""
    from gtsam_points_amd import _capi

    lib = _capi.load()
    p, o = C.c_void_p(256), C.c_void_p(512)  # never dereferenced
    h = C.c_void_p()
    for res in (0.0, -0.5, float("nan"), float("inf")):
        assert lib.gp_voxelgrid_plan_create(p, 100, res, None, C.byref(h)) == 1 and not h.value
    assert lib.gp_voxelgrid_plan_create(None, 100, 0.5, None, C.byref(h)) == 1 and not h.value
    assert lib.gp_voxelgrid_plan_create(p, -1, 0.5, None, C.byref(h)) == 1 and lib.gp_voxelgrid_plan_create(p, 100, 0.5, None, None) == 1
    assert lib.gp_voxelgrid_plan_create(None, 0, 0.5, None, C.byref(h)) == 0 and h.value
    nv, nd, k = C.c_int(7), C.c_int(7), C.c_int(7)
    assert lib.gp_voxelgrid_plan_info(h, C.byref(nv), C.byref(nd)) == 0 and (nv.value, nd.value) == (0, 0)
    assert lib.gp_voxelgrid_plan_info(None, C.byref(nv), C.byref(nd)) == 1
    for width in (0, 17, -3):
        assert lib.gp_voxelgrid_plan_average(h, p, width, o) == 1
        assert lib.gp_cloud_gather(p, width, p, 10, o, None) == 1
    assert lib.gp_voxelgrid_plan_average(None, p, 3, o) == 1
    assert lib.gp_voxelgrid_plan_average(h, None, 3, None) == 0  # an empty plan reduces nothing
    for rate in (0.0, -0.1, 1.5, float("nan"), float("inf")):
        assert lib.gp_voxelgrid_plan_random_indices(h, rate, 0, o, C.byref(k)) == 1
    assert lib.gp_voxelgrid_plan_random_indices(h, 0.5, 0, o, None) == 1 and lib.gp_voxelgrid_plan_random_indices(None, 0.5, 0, o, C.byref(k)) == 1
    assert lib.gp_voxelgrid_plan_random_indices(h, 0.5, 0, None, C.byref(k)) == 0 and k.value == 0
    for attr, idx, out in [(None, p, o), (p, None, o), (p, p, None)]:
        assert lib.gp_cloud_gather(attr, 3, idx, 10, out, None) == 1
    assert lib.gp_cloud_gather(p, 3, p, -1, o, None) == 1 and lib.gp_cloud_gather(None, 3, None, 0, None, None) == 0
    assert lib.gp_voxelgrid_plan_destroy(h) == 0 and lib.gp_voxelgrid_plan_destroy(None) == 0

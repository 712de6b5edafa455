"""tests/normals_ref.py checked without a GPU: the reference alone passes the helper, so a failure of tests/test_normals_gpu.py means the kernel.

The normals are built here from the C oracle's f64 covariances (and, where oracle/_ref/libref.so exists, from the reference's own estimate_covariances): the
eigenvector of the smallest eigenvalue by numpy.linalg.eigh, the sign rule of features/normal_estimation.cpp:26, rounded to f32 like the device's output.  On
every cloud the GPU tests use, the exempt share stays under knn_ref's cap (the helper fails otherwise).  Prints the worst sin / bound per cloud."""
import os
import re

import numpy as np
import pytest

import knn_ref
import normals_ref
import oracle
from oracle import refcapi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW_SYMBOLS = ("gp_estimate_normals_from_covs", "gp_estimate_normals_covariances")


def full_scan():
    return np.fromfile(os.path.join(GOLDEN, "kitti_00", "000000.bin"), dtype=np.float32).reshape(-1, 3)


def gpu_clouds():
    """(name, cloud, ks): what tests/test_normals_gpu.py runs the k-NN path on (its 1 M-point cloud is sampled there)"""
    return [
        ("kitti_00/000000.bin", full_scan(), (5, 10, 20)),
        ("sparse slab", knn_ref.sparse_slab_cloud(), (5, 10, 20)),
        ("wall and gap", knn_ref.wall_and_gap_cloud(), (10,)),
        ("duplicates and clusters", knn_ref.duplicates_cloud(), (10,)),
    ]


def _sources(cloud, k):
    ref, short = oracle.estimate_covariances(cloud, k, oracle.max_threads())
    assert short == 0
    out = [("oracle", ref)]
    if refcapi.available() and len(cloud) <= 40_000:  # (the reference's own sources, with the stand-in's Jacobi solver; the big scan is left to the oracle)
        out.append(("reference", refcapi.ref_estimate_covariances(cloud, k, oracle.max_threads())))
    return out


def test_reference_normals_pass_the_helper():
    for name, cloud, ks in gpu_clouds():
        for k in ks:
            cls = knn_ref.classify(cloud, k)
            for src, covs in _sources(cloud, k):
                n32 = normals_ref.reference_normals(cloud, covs).astype(np.float32)
                figs = normals_ref.assert_normals(cloud, k, n32, what=f"{src} {name}", cls=cls)
                assert figs["exempt"] <= knn_ref.EXEMPT_CAP * figs["n"]
                assert figs["worst_ratio"] <= 1.0


def test_reference_normals_from_f32_covariances_pass_the_helper(kitti07):
    cases = [(name, cloud, oracle.estimate_covariances(cloud, 10, oracle.max_threads())[0]) for name, cloud, _ in gpu_clouds()]
    cases.append(("kitti07_dec4 golden covariances", kitti07["points_0"], kitti07["covs_0"]))
    for name, cloud, covs in cases:
        c32 = np.ascontiguousarray(np.asarray(covs, dtype=np.float64).reshape(-1, 3, 3).transpose(0, 2, 1)).astype(np.float32).reshape(-1, 9)  # column-major, as stored
        n32 = normals_ref.reference_normals(cloud, normals_ref.stored_covs_as_matrices(c32)).astype(np.float32)
        normals_ref.assert_normals_from_covs(cloud, c32, n32, what=f"eigh of the f32 covariances, {name}")


def test_short_and_non_finite_points_follow_the_identity_rule():
    cloud = knn_ref.scan_cut(full_scan(), 7)
    cloud[2, 0] = 5.0  # p.x > 1: turned round
    cloud[3] = [0.5, 9.0, 9.0]
    got = np.zeros((7, 3), np.float32)
    got[:, 0] = np.where(cloud[:, 0] > 1.0, -1.0, 1.0)
    normals_ref.assert_normals(cloud, 10, got, what="seven points", cap_is_condition=False)
    wrong = got.copy()
    wrong[2, 0] = 1.0
    with pytest.raises(AssertionError, match="point 2: identity covariance"):
        normals_ref.assert_normals(cloud, 10, wrong, what="seven points", quiet=True)
    nan = cloud.copy()
    nan[5, 1] = np.nan
    for sign in (1.0, -1.0):  # a non-finite point: either sign
        g = got.copy()
        g[5, 0] = sign
        normals_ref.assert_normals(nan, 10, g, what="seven points, one NaN", quiet=True)
    eye = np.repeat(np.eye(3, dtype=np.float32).reshape(1, 9), 7, 0)
    normals_ref.assert_normals_from_covs(cloud, eye, got, what="identity covariances", quiet=True)
    with pytest.raises(AssertionError, match="point 2: identity covariance"):
        normals_ref.assert_normals_from_covs(cloud, eye, wrong, quiet=True)


def test_helper_names_a_turned_normal_and_a_tilted_one(kitti00):
    """the helper fails, and names the point, for ONE normal with the wrong sign outside the band and for ONE normal tilted by 1e-5 rad"""
    cloud = kitti00["source_points"]
    cls = knn_ref.classify(cloud, 10)
    covs, _ = oracle.estimate_covariances(cloud, 10, oracle.max_threads())
    good = normals_ref.reference_normals(cloud, covs)
    normals_ref.assert_normals(cloud, 10, good.astype(np.float32), what="oracle kitti00_dec8 source", cls=cls)
    s = np.abs(np.einsum("ni,ni->n", cloud.astype(np.float64), cls["V"][:, :, 0]))
    ok = ~(cls["tie"] | (cls["relgap"] < 1e-3))
    r = int(np.flatnonzero(ok & (s > 1.5))[0])
    turned = good.copy()
    turned[r] *= -1.0
    with pytest.raises(AssertionError, match=f"point {r}: p . v"):
        normals_ref.assert_normals(cloud, 10, turned.astype(np.float32), what="one turned", cls=cls, quiet=True)
    tilted = good.copy()
    t = np.cross(good[r], [0.3, 0.5, 0.8])
    tilted[r] = good[r] + 1e-5 * t / np.linalg.norm(t)
    tilted[r] /= np.linalg.norm(tilted[r])
    with pytest.raises(AssertionError, match=f"point {r}: beyond the per-point bound"):
        normals_ref.assert_normals(cloud, 10, tilted.astype(np.float32), what="one tilted", cls=cls, quiet=True)
    c32 = np.ascontiguousarray(covs.transpose(0, 2, 1)).astype(np.float32).reshape(-1, 9)
    n32 = normals_ref.reference_normals(cloud, normals_ref.stored_covs_as_matrices(c32))
    n32[r] = tilted[r]
    with pytest.raises(AssertionError, match=f"point {r}: beyond the bound"):
        normals_ref.assert_normals_from_covs(cloud, c32, n32.astype(np.float32), quiet=True)


def test_direction_bound_is_the_covariance_bound_on_the_normal():
    """|| (I - 0.999 v v^T) - (I - 0.999 w w^T) ||_F = 0.999 sqrt(2) sin(angle(v, w)), and the f32 store of a unit vector fits the first term"""
    rng = np.random.default_rng(3)
    v = rng.normal(size=(200, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    w = v + 1e-3 * rng.normal(size=(200, 3))
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    C = lambda u: np.eye(3)[None] - 0.999 * u[:, :, None] * u[:, None, :]
    lhs = np.linalg.norm((C(v) - C(w)).reshape(-1, 9), axis=1)
    np.testing.assert_allclose(lhs, normals_ref.SCALE * normals_ref.sin_angle(v, w), rtol=1e-6)
    assert abs(np.linalg.norm(C(v)[0]) - np.sqrt(2.0)) < 3e-4 * np.sqrt(2.0)
    assert np.sqrt(3.0) * 2.0 ** -25 < normals_ref.direction_bound(1.0) and normals_ref.direction_bound(np.inf) == pytest.approx(1.08e-7, rel=5e-3)


def test_header_and_binding_table_have_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "gtsam_points_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    from gtsam_points_amd import _capi

    for s in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + s + r"\s*\(", hdr), f"{s} is not declared in include/gtsam_points_hip.h"
        assert s in _capi.EXPORTED_SYMBOLS, f"{s} is not in _capi.EXPORTED_SYMBOLS"
    import gtsam_points_amd as gpa

    assert callable(gpa.estimate_normals_gpu) and callable(gpa.estimate_normals_covariances_gpu)


def test_argument_checks_need_no_device():
    """k outside 1..32, both outputs NULL, a missing array: GP_ERROR_INVALID_ARGUMENT before any device work (this host has no device); n == 0 is a no-op"""
    import ctypes as C

    from gtsam_points_amd import _capi

    lib = _capi.load()
    p, o = C.c_void_p(256), C.c_void_p(512)  # never dereferenced
    short = C.c_int(7)
    for k, normals, covs in [(0, o, o), (33, o, o), (-1, o, None), (10, None, None)]:
        assert lib.gp_estimate_normals_covariances(p, 100, k, 0.0, normals, covs, C.byref(short), None) == 1
    assert lib.gp_estimate_normals_covariances(None, 100, 10, 0.0, o, o, C.byref(short), None) == 1
    assert lib.gp_estimate_normals_covariances(p, 0, 10, 0.0, o, None, C.byref(short), None) == 0 and short.value == 0
    assert lib.gp_estimate_normals_from_covs(p, None, 100, o, None) == 1 and lib.gp_estimate_normals_from_covs(p, o, 100, None, None) == 1
    assert lib.gp_estimate_normals_from_covs(p, o, 0, o, None) == 0

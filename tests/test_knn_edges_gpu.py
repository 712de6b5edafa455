"""gp_knn.hip at its edges: every covariance of every cloud against the plain reference of tests/knn_ref.py, point by point (knn_ref.assert_covariances: no
statistic, no share of points let through), on every search structure the entry point accepts and every k from 1 to 32; gp_knn_search against exact
neighbours as a multiset of squared distances, where ties excuse nothing.

The structures (gp_estimate_covariances_ex / point_grid_create_impl): 0 binned + per-lane search, heavy queries first, sparse ones handed to the cooperative
far pass (k <= 10; the two-stream launch at k == 10); 1 the hashed multi-level grid; 3 the row-tiled pass + settle kernel first (k <= 10); 4 two binned levels;
6 binned without the heavy-first order; 7 heavy first but every query lane by lane.  k <= 10 runs covariance_kernel<10> (k == 10 its straight-line FULL form),
k >= 11 covariance_kernel<32>.

Figures measured on the MI355X (unmodified library; the [knn_ref] lines this module prints; oracle = the reference side alone, tests/test_knn_ref_cpu.py):
see GPU_FIGURES below.
"""
import numpy as np
import pytest

import knn_ref
import oracle

pytestmark = pytest.mark.gpu

STRUCTURES = (0, 1, 3, 4, 6, 7)
HASHED = 1
GPU_FIGURES = """
worst rel x relgap | worst rel, over the non-exempt points, f32 output against the f64 reference (so 3e-8 of every figure is the output's rounding):
                                   MI355X, structures 0 1 3 4 6 7 (alike to the digits shown)   oracle rounded to f32
  kitti00_dec8 source      k=10    2.8e-8 | 3.7e-8                                              2.8e-8 | 3.7e-8
  kitti_00/000000.bin      k=10    3.2e-8 | 3.7e-8   (1 tie exempt)                             3.2e-8 | 3.7e-8
  sparse slab              k=10    2.5e-8 | 3.7e-8                                              2.5e-8 | 3.7e-8
  wall and gap             k=10    2.7e-8 | 3.0e-8                                              2.7e-8 | 5.9e-8
  duplicates and clusters  k=10    2.4e-8 | 2.7e-6   (5 exempt, relgap < 1e-6)                  2.4e-8 | 9.9e-7
  C5 source, 1 M points    k=10    3.1e-8 | 6.8e-7   (11 ties exempt)                           3.1e-8 | 2.8e-7
  structures 0 and 1, per k:
  kitti_00/000000.bin      k=3     3.2e-8 | 1.6e-5   (484 collinear triples exempt, 0.39 %)     3.2e-8 | 1.7e-5
                           k=5     3.2e-8 | 8.0e-7                                              3.2e-8 | 4.7e-6
                           k=7, 9, 11, 16, 20, 32:  2.9e-8 .. 3.2e-8 | 3.7e-8 .. 1.1e-7         (k = 20, 32: 3.0e-8, 3.2e-8 | 3.7e-8, 3.8e-8)
  sparse slab              k=3 .. 32 (nine values): 2.1e-8 .. 3.1e-8 | 3.7e-8 .. 4.1e-8         (k = 3, 7, 32: 3.1e-8, 2.8e-8, 2.1e-8 | 3.8e-8)
The bound allows 1.5e-7 + 5.6e-7 / relgap: the device sits at the output's rounding on every point, a factor ~20 inside the eta term.
"""


# ---- clouds ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scan():
    import os

    return np.fromfile(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kitti_00", "000000.bin"), dtype=np.float32).reshape(-1, 3)


@pytest.fixture(scope="module")
def clouds(kitti00, scan):
    return {
        "kitti00_dec8 source": kitti00["source_points"],
        "kitti_00/000000.bin": scan,
        "sparse slab": knn_ref.sparse_slab_cloud(),
        "wall and gap": knn_ref.wall_and_gap_cloud(),
        "duplicates and clusters": knn_ref.duplicates_cloud(),
    }


_CLS = {}


def _check(gpu, name, cloud, k, structure, cap_is_condition=True):
    """one estimate_covariances call held to the per-point bound; the classification of (cloud, k) is computed once per module"""
    key = (name, k)
    if key not in _CLS:
        _CLS[key] = knn_ref.classify(cloud, k)
    fr = gpu.PointCloudGPU(cloud)
    short = gpu.estimate_covariances_gpu(fr, k, structure=structure)
    assert short == int(_CLS[key]["short"].sum()), (name, k, structure, short)
    got = fr.download("covs")
    knn_ref.assert_covariances(cloud, k, got, what=f"gpu structure {structure} {name}", cls=_CLS[key], cap_is_condition=cap_is_condition)
    return got


@pytest.mark.parametrize("structure", STRUCTURES)
@pytest.mark.parametrize("name", ["kitti00_dec8 source", "kitti_00/000000.bin", "sparse slab", "wall and gap", "duplicates and clusters"])
def test_covariances_every_structure_every_point(gpu, clouds, name, structure):
    _check(gpu, name, clouds[name], 10, structure)


@pytest.mark.parametrize("structure", [0, HASHED])
@pytest.mark.parametrize("k", [3, 5, 7, 9, 10, 11, 16, 20, 32])
@pytest.mark.parametrize("name", ["kitti_00/000000.bin", "sparse slab"])
def test_covariances_every_list_size(gpu, clouds, name, k, structure):
    """k = 11 .. 32: covariance_kernel<32>; k = 9: the partial list one below the FULL form; k < 10 on structure 0: partial lists through the cooperative far pass.
    The full scan at k = 3 is beyond the exempt cap by the reference alone (0.39 %: three consecutive returns of one ring of the sensor are collinear to 1e-8,
    tests/test_knn_ref_cpu.py::test_full_scan_at_k3_is_beyond_the_cap): there the share is printed, the collinear triples are held to the in-plane rule and
    every other point to the bound."""
    _check(gpu, name, clouds[name], k, structure, cap_is_condition=not (name == "kitti_00/000000.bin" and k == 3))


@pytest.mark.parametrize("structure", STRUCTURES)
@pytest.mark.parametrize("k", [1, 2])
def test_covariances_of_one_and_two_neighbours(gpu, clouds, k, structure):
    """k = 1: the sample covariance is the zero matrix, the closed form returns the identity eigenbasis, the output is diag(1e-3, 1, 1) -- exactly, as the
    oracle's (read off it here).
    k = 2: a rank-one sample covariance, relgap = 0 at every point: knn_ref.assert_two_neighbour_covariances (eigenvalues and the plane of the small
    eigenvector, every point; tests/test_knn_ref_cpu.py holds the oracle to the same).  The distance to the oracle's output is printed, not asserted: which
    vector of the plane comes out is the reference's rounding noise (include/gtsam_points_hip.h, gp_estimate_covariances).  Measured on the MI355X, every
    structure alike: kitti00_dec8 source 15,571 of 15,576 points within 7.1e-7 of the oracle (the bound of relgap = 1), the worst 3.3e-6; sparse slab 29,995 of
    30,003, the worst 2.0e-5."""
    for name in ("kitti00_dec8 source", "sparse slab"):
        cloud = clouds[name]
        fr = gpu.PointCloudGPU(cloud)
        assert gpu.estimate_covariances_gpu(fr, k, structure=structure) == 0
        got = fr.download("covs").astype(np.float64)
        ref, short = oracle.estimate_covariances(cloud, k, oracle.max_threads())
        assert short == 0
        if k == 1:
            assert (ref == np.diag([1e-3, 1.0, 1.0])).all()  # the reference's behaviour, read off the oracle
            np.testing.assert_array_equal(got, np.repeat(np.diag([1e-3, 1.0, 1.0]).astype(np.float32).astype(np.float64)[None], len(cloud), 0))
            continue
        rel = knn_ref.rel_frobenius(got, ref)
        print(f"[knn_ref] gpu structure {structure} {name}: k=2 worst rel vs oracle={rel.max():.3e} points beyond {knn_ref.covariance_bound(1.0):.2e}: "
              f"{int((rel > knn_ref.covariance_bound(1.0)).sum())} of {len(rel)}")
        knn_ref.assert_two_neighbour_covariances(cloud, got, what=f"gpu structure {structure} {name}")


@pytest.mark.parametrize("k", [5, 9, 11, 20])
def test_callers_stream_and_null_stream_give_the_same_bits(gpu, clouds, k):
    """(k = 10, the only k that takes the two-stream launch, is covered by test_side_stream_is_the_candidate_... in test_knn_gicp_gpu.py)"""
    import torch

    cloud = clouds["sparse slab"]
    a = gpu.PointCloudGPU(cloud)
    gpu.estimate_covariances_gpu(a, k)
    b = gpu.PointCloudGPU(cloud)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        gpu.estimate_covariances_gpu(b, k, stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(a.download("covs"), b.download("covs"))
    knn_ref.assert_covariances(cloud, k, b.download("covs"), what=f"gpu caller's stream, sparse slab")


@pytest.mark.parametrize("structure", [0, HASHED])
@pytest.mark.parametrize("k", [10, 20])
def test_covariances_around_the_launch_shapes(gpu, scan, k, structure):
    """n = k (every point is every point's neighbour), k + 1, one workgroup of 128 +- 1, and one query more than the far pass's 8192 workgroups of four hold"""
    for n in (k, k + 1, 127, 128, 129, 4 * 8192 + 1):
        cut = knn_ref.scan_cut(scan, n)
        assert len(cut) == n
        fr = gpu.PointCloudGPU(cut)
        assert gpu.estimate_covariances_gpu(fr, k, structure=structure) == 0
        knn_ref.assert_covariances(cut, k, fr.download("covs"), what=f"gpu structure {structure} scan cut n={n}")
    few = gpu.PointCloudGPU(knn_ref.scan_cut(scan, k - 1))  # one point too few: identity, every point counted
    assert gpu.estimate_covariances_gpu(few, k, structure=structure) == k - 1
    np.testing.assert_array_equal(few.download("covs"), np.repeat(np.eye(3, dtype=np.float32)[None], k - 1, 0))


# ---- gp_knn_search -----------------------------------------------------------------------------------------------------------------------------------
def _d2(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]


def check_knn(res, p, q, k, max_sq_dist=None, what=""):
    """(indices, sq_dists, num_found) of a search against the exact neighbours: the row of distances IS the reference's sorted d2 (a multiset check: a tie
    cannot excuse a wrong distance), every index has the distance written beside it, the indices of a row are distinct, -1 exactly beyond num_found.
    max_sq_dist: strict '<' (KnnResult::push, ann/knn_result.hpp:89-109)."""
    idx, d, nf = res
    rd2, _ = knn_ref.neighbours(p, q, k)
    rd2 = rd2[:, :k]
    want = np.isfinite(rd2) if max_sq_dist is None else (rd2 < max_sq_dist)
    want_nf = want.sum(1)
    bad = np.flatnonzero(nf != want_nf)
    assert len(bad) == 0, f"{what}: num_found differs for {len(bad)} queries, first {bad[:5].tolist()}: got {nf[bad[:5]].tolist()} want {want_nf[bad[:5]].tolist()} reference d2 {rd2[bad[:1]].tolist()}"
    held = np.arange(k)[None] < nf[:, None]
    assert ((idx >= 0) == held).all(), f"{what}: idx == -1 exactly beyond num_found"
    assert idx.max(initial=-1) < len(p)
    d = np.where(held, d, 0.0)  # (what lies beyond num_found is not specified)
    err = np.where(held, np.abs(d - np.where(held, rd2, 0.0)), 0.0)
    r = np.unravel_index(np.argmax(err), err.shape)
    assert err.max(initial=0.0) < 1e-9, f"{what}: query {r[0]} rank {r[1]}: got d2 {d[r]:.12g}, reference {rd2[r]:.12g}\n  got {d[r[0]].tolist()}\n  ref {rd2[r[0]].tolist()}"
    own = _d2(np.asarray(p, np.float32)[np.where(held, idx, 0)], np.asarray(q, np.float32)[:, None, :])
    err2 = np.where(held, np.abs(own - d), 0.0)
    assert err2.max(initial=0.0) < 1e-9, f"{what}: an index does not have the distance written beside it ({err2.max():.3e})"
    srt = np.sort(np.where(held, idx, -1 - np.arange(k)[None]), axis=1)
    assert (np.diff(srt, axis=1) != 0).all(), f"{what}: an index twice in one row"
    return want_nf


@pytest.mark.parametrize("structure", STRUCTURES)
def test_knn_search_every_structure(gpu, kitti00, structure):
    p = kitti00["target_points"]
    rng = np.random.default_rng(41)
    q = np.concatenate([kitti00["source_points"][:2000], rng.uniform(-60, 60, (501, 3)).astype(np.float32) * np.array([1, 1, 0.05], np.float32)])
    tree = gpu.KdTreeGPU(gpu.PointCloudGPU(p), cell_size=0.5, structure=structure)
    for k in (1, 2, 10, 11, 32):
        check_knn(tree.knn_search(q, k), p, q, k, what=f"structure {structure} k={k}")
    check_knn(tree.knn_search(q, 10, max_sq_dist=0.25), p, q, 10, max_sq_dist=0.25, what=f"structure {structure} k=10 bounded")


def _lattice(h):
    g = np.arange(-8, 9, dtype=np.float64) * h
    a = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return np.concatenate([a, a + 0.5 * h]).astype(np.float32)


@pytest.mark.parametrize("structure", [0, HASHED])
@pytest.mark.parametrize("h", [0.5, 0.3])
def test_knn_search_on_a_lattice(gpu, structure, h):
    """points on the faces of the cells, negative ones included, and the same lattice half a cell further; queries on lattice points, on cell faces, edges and
    corners.  Every rank is tied (6 neighbours at h, 12 at sqrt(2) h, ...): only the distances can be compared, and they must be right.  h = 0.5 is exact in
    binary (a point IS on the face), h = 0.3 is not (a point is within an ulp of it, on either side)."""
    p = _lattice(h)
    rng = np.random.default_rng(43)
    cells = rng.integers(-9, 10, size=(1500, 3)).astype(np.float64)
    frac = rng.choice([0.0, 0.0, 0.25, 0.5], size=(1500, 3))  # all three 0: a corner (a lattice point); two: an edge; one: a face
    q = ((cells + frac) * h).astype(np.float32)
    tree = gpu.KdTreeGPU(gpu.PointCloudGPU(p), cell_size=h, structure=structure)
    for k in (1, 7, 10, 32):
        check_knn(tree.knn_search(q, k), p, q, k, what=f"lattice h={h} structure {structure} k={k}")
    r2 = float(np.float32(h)) ** 2  # exactly the squared lattice step (h = 0.5): the six neighbours AT the bound are not found
    check_knn(tree.knn_search(q, 10, max_sq_dist=r2), p, q, 10, max_sq_dist=r2, what=f"lattice h={h} structure {structure} bounded")


@pytest.mark.parametrize("structure", [0, HASHED])
def test_knn_search_tens_of_kilometres_from_the_origin(gpu, scan, kitti00, structure):
    """f32 coordinates have a 2 mm grid at 36 km: the f32 pre-filter's error term (loosened_bound) is what keeps it from rejecting a true neighbour"""
    t = np.array([20000.0, -30000.0, 4000.0], np.float32)
    p = (scan + t).astype(np.float32)
    q = (kitti00["source_points"][:3000] + t).astype(np.float32)
    tree = gpu.KdTreeGPU(gpu.PointCloudGPU(p), cell_size=0.5, structure=structure)
    for k in (1, 10, 32):
        check_knn(tree.knn_search(q, k), p, q, k, what=f"translated scan structure {structure} k={k}")
    check_knn(tree.knn_search(q, 10, max_sq_dist=0.04), p, q, 10, max_sq_dist=0.04, what=f"translated scan structure {structure} bounded")


@pytest.mark.parametrize("structure", [0, HASHED])
def test_knn_search_from_outside_the_bounding_box(gpu, kitti00, structure):
    """queries a kilometre outside the cloud's bounding box (along every axis and every diagonal) and exactly on its faces"""
    p = kitti00["target_points"]
    lo, hi = p.min(0).astype(np.float64), p.max(0).astype(np.float64)
    mid = 0.5 * (lo + hi)
    dirs = [np.array(d, np.float64) for d in np.ndindex(3, 3, 3)]
    far = [np.where(d == 0, lo - 1000.0, np.where(d == 2, hi + 1000.0, mid)) for d in dirs if (d != 1).any()]
    rng = np.random.default_rng(47)
    on_faces = []
    for a in range(3):
        for bound in (lo, hi):
            f = rng.uniform(lo, hi, size=(8, 3))
            f[:, a] = bound[a]
            on_faces.append(f)
    q = np.concatenate([np.array(far), np.concatenate(on_faces), [lo, hi]]).astype(np.float32)
    tree = gpu.KdTreeGPU(gpu.PointCloudGPU(p), cell_size=2.0, structure=structure)
    for k in (1, 10, 32):
        check_knn(tree.knn_search(q, k), p, q, k, what=f"outside structure {structure} k={k}")
    nf = check_knn(tree.knn_search(q, 10, max_sq_dist=1.0), p, q, 10, max_sq_dist=1.0, what=f"outside structure {structure} bounded")
    assert (nf[:26] == 0).all()


@pytest.mark.parametrize("structure", [0, HASHED])
def test_knn_search_small_clouds_and_odd_query_counts(gpu, kitti00, structure):
    p = kitti00["target_points"]
    q = kitti00["source_points"]
    rng = np.random.default_rng(61)
    for n in (1, 5, 31):  # k > n: every point is found, num_found == n
        tree = gpu.KdTreeGPU(gpu.PointCloudGPU(p[:n]), cell_size=0.5, structure=structure)
        # (queries within a few cells of the points: a small cloud has one level of cells, and a query a hundred metres away walks every empty shell between)
        near = (p[np.arange(129) % n] + rng.normal(0.0, 0.7, size=(129, 3))).astype(np.float32)
        for k in (1, 10, 32):
            nf = check_knn(tree.knn_search(near, k), p[:n], near, k, what=f"n={n} structure {structure} k={k}")
            assert (nf == min(k, n)).all()
    tree = gpu.KdTreeGPU(gpu.PointCloudGPU(p), cell_size=0.5, structure=structure)
    for nq in (1, 127, 129):
        for k in (1, 10, 32):
            check_knn(tree.knn_search(q[1000:1000 + nq], k), p, q[1000:1000 + nq], k, what=f"nq={nq} structure {structure} k={k}")


@pytest.mark.parametrize("structure", [0, HASHED])
def test_knn_search_bound_exactly_at_a_neighbour(gpu, structure):
    """max_sq_dist set EXACTLY to the reference's d2 of rank j of a query: KnnResult::push is strict '<', so that query finds j - 1 (ranks from 1).
    oracle.OracleKdTree does the same with the same bound (its kd-tree fills the rest with -1), and the count is compared with it too.  The coordinates are
    multiples of 1/64 within +-8: every difference, square and sum is exact in f64 in any order and with any contraction, so `exactly` means the same number
    on the device as here -- and many other queries have a neighbour exactly at the bound as well."""
    rng = np.random.default_rng(53)
    p = (rng.integers(-512, 513, size=(6000, 3)) / 64.0).astype(np.float32)
    p[:, 2] = (p[:, 2] * 8).round() / 64.0  # a slab: neighbours within a cell or two
    q = np.concatenate([p[:200], (rng.integers(-512, 513, size=(200, 3)) / 64.0).astype(np.float32)])
    rd2, _ = knn_ref.neighbours(p, q, 32)
    otree = oracle.OracleKdTree(p)
    tree = gpu.KdTreeGPU(gpu.PointCloudGPU(p), cell_size=0.5, structure=structure)
    for k, j, row in [(10, 4, 0), (10, 10, 3), (32, 17, 250), (32, 32, 399), (1, 1, 300), (2, 2, 301)]:
        bound = float(rd2[row, j - 1])
        assert bound > 0.0
        res = tree.knn_search(q, k, max_sq_dist=bound)
        nf = check_knn(res, p, q, k, max_sq_dist=bound, what=f"bound at rank {j} of query {row}, structure {structure} k={k}")
        assert nf[row] == (rd2[row, :k] < bound).sum() <= j - 1
        at_bound = (rd2[:, :k] == bound).any(1)
        assert at_bound.sum() >= 1
        oidx, _ = otree.knn(q, k, max_sq_dist=bound, num_threads=4)
        np.testing.assert_array_equal(res[2], (oidx >= 0).sum(1))


@pytest.mark.parametrize("structure", [0, HASHED])
def test_knn_search_with_non_finite_points_and_queries(gpu, kitti00, structure):
    """1 % of the points and 1 % of the queries are not finite (NaN, +inf, -inf in one, two or three coordinates), k = 32: such points are nobody's neighbours,
    such queries find nothing"""
    rng = np.random.default_rng(59)
    p = kitti00["target_points"].copy()
    q = kitti00["source_points"][:4000].copy()
    for a in (p, q):
        rows = rng.choice(len(a), len(a) // 100, replace=False)
        for r in rows:
            a[r, rng.choice(3, rng.integers(1, 4), replace=False)] = rng.choice([np.nan, np.inf, -np.inf])
    tree = gpu.KdTreeGPU(gpu.PointCloudGPU(p), cell_size=0.5, structure=structure)
    for k in (32, 10):
        res = tree.knn_search(q, k)
        nf = check_knn(res, p, q, k, what=f"non-finite structure {structure} k={k}")
        assert (nf[~np.isfinite(q).all(1)] == 0).all() and (nf[np.isfinite(q).all(1)] == k).all()
        assert np.isfinite(p[res[0][res[0] >= 0]]).all()

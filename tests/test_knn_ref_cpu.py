"""The plain k-NN / covariance reference (tests/knn_ref.py) checked without a GPU: the per-point bound, the exempt cap and the tie rule are proven on the
oracle's output (the reference's closed-form solver, rounded to f32 like the device's output) on the clouds the GPU tests use; the neighbour search against
a brute-force argsort.  Prints the measured tau_out, eta and the exempt share per cloud (pytest -s shows them; a failure shows them too)."""
import os

import numpy as np
import pytest

import knn_ref
import oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _full_scan():
    return np.fromfile(os.path.join(GOLDEN, "kitti_00", "000000.bin"), dtype=np.float32).reshape(-1, 3)


def _clouds(kitti00, kitti07):
    return [
        ("kitti00_dec8 source", kitti00["source_points"], (10,)),
        ("kitti00_dec8 target", kitti00["target_points"], (10,)),
        ("kitti07_dec4 points_0", kitti07["points_0"], (10,)),
        ("kitti_00/000000.bin", _full_scan(), (5, 10, 20, 32)),
        ("sparse slab", knn_ref.sparse_slab_cloud(), (3, 7, 10, 32)),
        ("scan cut of 129", knn_ref.scan_cut(_full_scan(), 129), (10, 20)),
        ("wall and gap", knn_ref.wall_and_gap_cloud(), (10,)),
        ("duplicates and clusters", knn_ref.duplicates_cloud(), (10,)),
    ]


def test_neighbours_match_bruteforce():
    rng = np.random.default_rng(5)
    p = rng.uniform(-20, 20, (2000, 3)).astype(np.float32)
    p[:, 2] *= 0.1
    p[100:140] = p[:40]  # exact duplicates
    p[7] = np.nan
    q = np.concatenate([p[:300], rng.uniform(-30, 30, (211, 3)).astype(np.float32)])
    q[17] = np.inf
    keep = np.flatnonzero(np.isfinite(p).all(1))
    for k in (1, 10, 32):
        d2, idx = knn_ref.neighbours(p, q, k)
        assert d2.shape == (len(q), k + 1) and idx.dtype == np.int64
        for b in range(0, len(q), 128):  # blocked brute force
            qq = q[b:b + 128].astype(np.float64)
            diff = p[keep].astype(np.float64)[None] - qq[:, None]
            full = diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1] + diff[..., 2] * diff[..., 2]
            ref = np.sort(full, 1)[:, :k + 1]
            ok = np.isfinite(qq).all(1)
            np.testing.assert_array_equal(d2[b:b + 128][ok], ref[ok])
            assert np.isinf(d2[b:b + 128][~ok]).all() and (idx[b:b + 128][~ok] == -1).all()
            back = ((p[idx[b:b + 128][ok]].astype(np.float64) - qq[ok][:, None]) ** 2).sum(2)
            np.testing.assert_allclose(back, d2[b:b + 128][ok], rtol=1e-15, atol=0)
            assert all(len(set(r)) == k + 1 for r in idx[b:b + 128][ok])
    # fewer points than asked for
    d2, idx = knn_ref.neighbours(p[:4], q[:5], 10)
    assert np.isfinite(d2[:, :4]).all() and np.isinf(d2[:, 4:]).all() and (idx[:, 4:] == -1).all()


def test_classify_tie_rule():
    """a tie between copies of one coordinate is no tie; the same distance to two different coordinates is one"""
    ring = np.array([[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0.0]], np.float32)  # four points at distance 1 of the origin
    far = np.array([[5, 5, 5], [6, 5, 5], [5, 6, 5], [7, 7, 7], [8, 8, 7], [9, 9, 9]], np.float32)
    cloud = np.concatenate([[[0, 0, 0]], ring, far]).astype(np.float32)
    assert knn_ref.classify(cloud, 3)["tie"][0] and knn_ref.classify(cloud, 4)["tie"][0]
    assert not knn_ref.classify(cloud, 5)["tie"][0]  # the four ring points and the origin: rank 6 is far away
    copies = np.concatenate([[[0, 0, 0]], ring[:2], ring[2:3], ring[2:3], ring[2:3], far]).astype(np.float32)
    c = knn_ref.classify(copies, 4)
    assert c["tie"][0]  # ranks 2..6 all at distance 1, three coordinates among them
    copies2 = np.concatenate([[[0, 0, 0]], [[0.5, 0, 0]], ring[2:3], ring[2:3], ring[2:3], far]).astype(np.float32)
    assert not knn_ref.classify(copies2, 3)["tie"][0] and not knn_ref.classify(copies2, 4)["tie"][0]  # only copies of one coordinate at the boundary


def test_bound_is_a_function_of_relgap_alone():
    assert knn_ref.covariance_bound(1.0) == pytest.approx(knn_ref.TAU_OUT + knn_ref.ETA)
    assert knn_ref.TAU_OUT == 4 * knn_ref.TAU_OUT_BASE and knn_ref.ETA <= 100 * 5.6e-9
    assert np.isinf(knn_ref.covariance_bound(0.0))


def test_oracle_covariances_meet_the_per_point_bound(kitti00, kitti07):
    """assert_covariances on the ORACLE's f32-rounded output: every cloud of the GPU tests is within the exempt cap by the reference alone, every point within
    the bound; tau_out and eta as measured here must not exceed the bases the bound was built from"""
    tau, eta = 0.0, 0.0
    for name, cloud, ks in _clouds(kitti00, kitti07):
        for k in ks:
            ref, short = oracle.estimate_covariances(cloud, k, oracle.max_threads())
            assert short == 0
            r32 = ref.astype(np.float32)
            tau = max(tau, float(knn_ref.rel_frobenius(r32, ref).max()))
            cls = knn_ref.classify(cloud, k)
            ok = ~(cls["tie"] | (cls["relgap"] < knn_ref.RELGAP_EXEMPT))
            rel = knn_ref.rel_frobenius(ref, cls["C"])
            e = float((rel[ok] * cls["relgap"][ok]).max())
            eta = max(eta, e)
            print(f"[knn_ref] oracle (f64) {name}: k={k} worst rel x relgap={e:.3e} worst rel={rel[ok].max():.3e} relgap<1e-3: {(cls['relgap'] < 1e-3).sum()}")
            knn_ref.assert_covariances(cloud, k, r32, what=f"oracle {name}")
    print(f"[knn_ref] measured tau_out={tau:.3e} (base {knn_ref.TAU_OUT_BASE:.1e}, bound uses x4)  eta={eta:.3e} (base {knn_ref.ETA_BASE:.1e}, bound uses x{knn_ref.ETA_FACTOR:g})")
    assert tau <= knn_ref.TAU_OUT_BASE and eta <= knn_ref.ETA_BASE * 1.01


def test_two_neighbours_are_rank_one_for_the_reference_too(kitti00):
    """k = 2: every point has relgap < 1e-6 by the reference alone (a rank-one sample covariance), so no point has a per-point bound; the oracle's output
    meets the rule that is left (knn_ref.assert_two_neighbour_covariances).  k = 1: the oracle writes diag(1e-3, 1, 1) exactly."""
    for cloud in (kitti00["source_points"], knn_ref.sparse_slab_cloud()):
        cls = knn_ref.classify(cloud, 2)
        assert (cls["relgap"] < knn_ref.RELGAP_EXEMPT).all() and (cls["topgap"] > 0.999).all()
        ref, short = oracle.estimate_covariances(cloud, 2, oracle.max_threads())
        assert short == 0
        knn_ref.assert_two_neighbour_covariances(cloud, ref.astype(np.float32), what="oracle")
        one, _ = oracle.estimate_covariances(cloud, 1, oracle.max_threads())
        assert (one == np.diag([1e-3, 1.0, 1.0])).all()


def test_full_scan_at_k3_is_beyond_the_cap():
    """three consecutive returns of one ring are collinear to 1e-8: at k = 3 the full scan has 0.39 % of its points below relgap 1e-6, by the reference alone.
    The helper refuses it as a condition; with the condition lifted the oracle's output passes every per-point rule (the in-plane rule for the collinear ones)."""
    cloud = _full_scan()
    ref, _ = oracle.estimate_covariances(cloud, 3, oracle.max_threads())
    with pytest.raises(AssertionError, match="above the cap"):
        knn_ref.assert_covariances(cloud, 3, ref.astype(np.float32), what="oracle full scan", quiet=True)
    figs = knn_ref.assert_covariances(cloud, 3, ref.astype(np.float32), what="oracle kitti_00/000000.bin", cap_is_condition=False)
    assert 0.001 < figs["exempt"] / figs["n"] < 0.01 and figs["ties"] == 0


def test_assert_covariances_names_a_lost_neighbour(kitti00):
    """the helper fails, and names the point, when ONE point of a cloud was computed from neighbour 0 twice in place of its k-th neighbour"""
    cloud = kitti00["source_points"]
    ref, _ = oracle.estimate_covariances(cloud, 10, oracle.max_threads())
    got = ref.astype(np.float32)
    cls = knn_ref.classify(cloud, 10, subset=[4000])
    nb = cloud[cls["idx"][0, :10]].astype(np.float64)
    nb[9] = nb[0]
    got[4000] = knn_ref.reference_covariance(nb[None])[0][0].astype(np.float32)
    with pytest.raises(AssertionError, match="point 4000: beyond the per-point bound"):
        knn_ref.assert_covariances(cloud, 10, got, what="one lost neighbour", quiet=True)
    # and the cap is a condition: a lattice (every rank tied) is refused
    g = np.arange(-4, 5, dtype=np.float32)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    with pytest.raises(AssertionError, match="above the cap"):
        knn_ref.assert_covariances(lattice, 10, np.repeat(np.eye(3)[None], len(lattice), 0), what="lattice", quiet=True)

"""GPU tests of IntensityKdTreeGPU (gp_intensity_grid_*): the exact 1-NN search in (x, y, z, intensity) against the brute-force f64 restatement
color_consistency_ref.nearest_xyzi.

Indices must be EQUAL to the reference's and the squared 4-D distances agree to 1e-12 relative: both sides form them in f64 on the same f32 inputs.  Every comparison
first asserts from the reference that no query sits on a tie or on the cut-off (margins > 1e-9 relative), as tests/test_colored_gicp_gpu.py does.

The scene is color_consistency_ref.textured_scene(): colored_ref.two_plane_cloud() with an intensity field whose texture is at the scale of the point spacing, and
colored_ref.moved_copy of it as queries -- tests/test_color_consistency_ref_cpu.py holds it to the conditions that make the 4-D search differ from the 3-D one."""
import numpy as np
import pytest

import color_consistency_ref as cc

pytestmark = pytest.mark.gpu
MARGIN = 1e-9
DIST_TOL = 1e-12
FMAX = np.finfo(np.float64).max


def _f64(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


@pytest.fixture(scope="module")
def scene(gpu):
    s = cc.textured_scene()
    tgt = gpu.PointCloudGPU(s["tp"], intensities=s["tI"])
    queries = np.concatenate([_f64(s["sp"]), _f64(s["sI"])[:, None]], axis=1)  # the source at the "identity" pose: 10 cm off its target points
    refs = {}
    for scale in (1.0, 0.0):
        for max_sq in (FMAX, 0.09):
            refs[(scale, max_sq)] = cc.nearest_xyzi(_f64(s["tp"]), _f64(s["tI"]), queries[:, :3], queries[:, 3], scale, max_sq)
    return dict(s, tgt=tgt, queries=queries, refs=refs, tree=gpu.IntensityKdTreeGPU(tgt))


def _compare(got, ref, max_sq, what):
    idx, d, found = got
    ridx, rd, tie, cut = ref
    print(f"[xyzi] {what}: {int((ridx >= 0).sum())} of {len(ridx)} matched, smallest tie gap {tie.min():.3e}, smallest cut-off gap {cut.min():.3e}")
    assert tie.min() > MARGIN and cut.min() > MARGIN, f"{what}: a query two f64 implementations could decide differently"
    assert idx.shape == (len(ridx), 1) and idx.dtype == np.int32 and d.dtype == np.float64
    assert np.array_equal(idx[:, 0], ridx), (what, np.flatnonzero(idx[:, 0] != ridx)[:10])
    hit = ridx >= 0
    assert np.array_equal(found, hit.astype(np.int32))
    assert (np.abs(d[hit, 0] - rd[hit]) <= DIST_TOL * rd[hit]).all(), what
    assert (d[~hit, 0] == max_sq).all()


@pytest.mark.parametrize("m", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_matches_brute_force(gpu, scene, m):
    """the edges of a wave, a workgroup and a tile of queries, unbounded and with the 0.3 m cut-off"""
    for max_sq in (FMAX, 0.09):
        ref = tuple(a[:m] for a in scene["refs"][(1.0, max_sq)])
        _compare(scene["tree"].knn_search(scene["queries"][:m], 1, max_sq), ref, max_sq, f"m={m} max_sq={max_sq:.3g}")


def test_the_scene_tells_the_two_searches_apart(gpu, scene):
    """on the device too: at least 10 % of the matched queries have another nearest in XYZI than in 3-D, and some lose their match to the 4-D cut-off"""
    q = scene["queries"]
    i4 = scene["tree"].knn_search(q, 1, 0.09)[0][:, 0]
    i3, d3, _ = gpu.KdTreeGPU(scene["tgt"]).knn_search(q[:, :3].astype(np.float32), 1, 0.09)
    matched = i4 >= 0
    assert (i4[matched] != i3[matched, 0]).mean() >= 0.10
    assert ((i3[:, 0] >= 0) & ~matched).sum() >= 1


@pytest.mark.parametrize("n", [1, 2, 4000])
def test_target_sizes(gpu, scene, n):
    tp, tI = np.ascontiguousarray(scene["tp"][:n]), np.ascontiguousarray(scene["tI"][:n])
    tree = scene["tree"] if n == 4000 else gpu.IntensityKdTreeGPU(gpu.PointCloudGPU(tp, intensities=tI))
    q = scene["queries"][:257]
    for max_sq in (FMAX, 0.5):
        _compare(tree.knn_search(q, 1, max_sq), cc.nearest_xyzi(_f64(tp), _f64(tI), q[:, :3], q[:, 3], 1.0, max_sq), max_sq, f"n={n} max_sq={max_sq:.3g}")


def test_scale_zero_is_the_3d_search(gpu, scene):
    """the scale sits on the stored side only: at 0 every stored intensity vanishes, d4^2 = d3^2 + I_q^2, and the nearest is KdTreeGPU's"""
    q = scene["queries"][:1025]
    tree0 = gpu.IntensityKdTreeGPU(scene["tgt"], intensity_scale=0.0)
    got = tree0.knn_search(q, 1)
    _compare(got, tuple(a[:1025] for a in scene["refs"][(0.0, FMAX)]), FMAX, "scale 0")
    i3, d3, _ = gpu.KdTreeGPU(scene["tgt"]).knn_search(q[:, :3].astype(np.float32), 1)
    assert np.array_equal(got[0], i3)
    assert (np.abs(got[1][:, 0] - (d3[:, 0] + q[:, 3] ** 2)) <= DIST_TOL * got[1][:, 0]).all()


def test_large_scale_reaches_beyond_the_first_shells(gpu):
    """the only target point with a query's (scaled) intensity lies four cells away; fifty nearer points differ strongly in intensity: the far point is returned"""
    rng = np.random.default_rng(5)
    near = rng.uniform(-0.1, 0.1, (50, 3))
    tp = np.vstack([near, [[1.0, 0.02, -0.03]]]).astype(np.float32)
    tI = np.concatenate([np.zeros(50), [0.9]]).astype(np.float32)
    scale = 10.0
    q = np.concatenate([rng.uniform(-0.1, 0.1, (65, 3)).astype(np.float32).astype(np.float64), np.full((65, 1), scale * float(np.float32(0.9)))], axis=1)
    tree = gpu.IntensityKdTreeGPU(gpu.PointCloudGPU(tp, intensities=tI), intensity_scale=scale, cell_size=0.25)
    ref = cc.nearest_xyzi(_f64(tp), _f64(tI), q[:, :3], q[:, 3], scale)
    assert (ref[0] == 50).all() and (ref[1] > 0.7).all()  # 3 cells and more: shells beyond the first
    _compare(tree.knn_search(q, 1), ref, FMAX, "large scale")
    # with a cut-off the 3-D distance alone rules the far point out, nothing matches, although fifty points lie within it in 3-D
    assert (tree.knn_search(q, 1, 0.25)[0] == -1).all()


def test_cut_off_is_strict_on_the_4d_distance(gpu):
    tp, tI = np.array([[0.0, 0.0, 0.0]], np.float32), np.array([0.0], np.float32)
    q = np.array([[_f64(0.3), 0.0, 0.0, _f64(0.4)]])
    d = float(cc.nearest_xyzi(_f64(tp), _f64(tI), q[:, :3], q[:, 3])[1][0])
    assert abs(d - 0.25) < 1e-6
    tree = gpu.IntensityKdTreeGPU(gpu.PointCloudGPU(tp, intensities=tI))
    idx, dist, _ = tree.knn_search(q, 1, np.nextafter(d, np.inf))
    assert idx[0, 0] == 0 and dist[0, 0] == d  # one point, the same f64 expression: the same bits
    assert tree.knn_search(q, 1, d)[0][0, 0] == -1  # strict
    assert tree.knn_search(q, 1, np.nextafter(d, 0.0))[0][0, 0] == -1
    # the 3-D distance alone (0.09) is inside a cut-off of 0.2: it is the 4-D distance that is held against it
    assert tree.knn_search(q, 1, 0.2)[0][0, 0] == -1


def test_wide_bounding_box_takes_the_hashed_grid(gpu, scene):
    """200 points 30 km away make the bounding box too large for the block grid (2^24 blocks of 1 m): the structure falls back to the hashed multi-level grid, on
    which the XYZI search runs too"""
    rng = np.random.default_rng(9)
    far = rng.uniform(-1.0, 1.0, (200, 3)) + np.array([30000.0, -20000.0, 25000.0])
    tp = np.vstack([scene["tp"], far]).astype(np.float32)
    tI = np.concatenate([scene["tI"], rng.uniform(0.0, 1.0, 200)]).astype(np.float32)
    tree = gpu.IntensityKdTreeGPU(gpu.PointCloudGPU(tp, intensities=tI))
    fq = np.concatenate([_f64(far[:63] + rng.normal(0.0, 0.05, (63, 3))), _f64(tI[4000:4063] + 0.01)[:, None]], axis=1)
    q = np.vstack([scene["queries"][:257], fq])
    for max_sq in (1.0, 0.09):
        ref = cc.nearest_xyzi(_f64(tp), _f64(tI), q[:, :3], q[:, 3], 1.0, max_sq)
        assert (ref[0][257:] >= 4000).any()
        _compare(tree.knn_search(q, 1, max_sq), ref, max_sq, f"hashed max_sq={max_sq}")


def test_non_finite_input_is_never_matched(gpu, scene):
    tp, tI = scene["tp"][:300].copy(), scene["tI"][:300].copy()
    q = np.concatenate([_f64(tp[:5]), _f64(tI[:5])[:, None]], axis=1)  # queries ON target points 0 .. 4
    tp[0, 1] = np.nan
    tI[1] = np.inf
    tI[2] = np.nan
    tp[3, 0] = np.inf
    tree = gpu.IntensityKdTreeGPU(gpu.PointCloudGPU(tp, intensities=tI))
    ref =cc.nearest_xyzi(_f64(tp), _f64(tI), q[:, :3], q[:, 3])
    assert not np.isin(ref[0], [0, 1, 2, 3]).any() and ref[0][4] == 4
    idx, d, _ = tree.knn_search(q, 1)
    assert np.array_equal(idx[:, 0], ref[0]) and np.isfinite(d).all()
    bad = q[[4, 4, 4, 4]].copy()
    bad[0, 0], bad[1, 3], bad[2, 2], bad[3, 3] = np.nan, np.nan, np.inf, -np.inf
    for max_sq in (FMAX, 1.0):
        assert (tree.knn_search(bad, 1, max_sq)[0] == -1).all()
    assert tree.knn_search(q[4:5], 1, 1.0)[0][0, 0] == 4


def test_errors(gpu, scene):
    with pytest.raises(gpu.GPError, match="k must be 1"):
        scene["tree"].knn_search(scene["queries"][:4], 2)
    with pytest.raises(gpu.GPError, match="no intensities"):
        gpu.IntensityKdTreeGPU(gpu.PointCloudGPU(scene["tp"]))
    with pytest.raises(gpu.GPError, match="gp_intensity_grid_create"):
        gpu.IntensityKdTreeGPU(scene["tgt"], intensity_scale=float("nan"))
    assert scene["tree"].knn_search(np.zeros((0, 4)), 1)[0].shape == (0, 1)


def test_two_runs_give_identical_bits(gpu, scene):
    q = scene["queries"]
    a = scene["tree"].knn_search(q, 1, 0.09)
    b = scene["tree"].knn_search(q, 1, 0.09)
    c = gpu.IntensityKdTreeGPU(scene["tgt"]).knn_search(q, 1, 0.09)  # a second build of the structure too
    for x, y, z in zip(a, b, c):
        assert x.tobytes() == y.tobytes() == z.tobytes()

"""tests/cloud_ref.py checked without a GPU: the restatement agrees with independent code (oracle/vgicp_oracle_np.py, oracle.merge_frames), meets on its own what
tests/test_cloud_edges_gpu.py asks of the device, and every (input, pose, resolution) combination those tests name lies far enough from a voxel face and from the
surface-validation threshold that two correct f64 evaluations decide alike -- so a failure of the GPU tests means the kernels."""
import numpy as np
import pytest

import cloud_ref as cr
import oracle
from helpers import expmap
from oracle import vgicp_oracle_np as onp


def test_fast_floor_is_a_floor_where_truncation_is_not():
    x = np.array([-0.0, -1e-30, -0.5, -1.0, 0.0, 0.5, 1.0, 2.0**31 - 1.5])
    got = cr.fast_floor(x)
    np.testing.assert_array_equal(got, [0, -1, -1, -1, 0, 0, 1, 2**31 - 2])
    np.testing.assert_array_equal(got, np.floor(x).astype(np.int64))
    differs = np.trunc(x).astype(np.int64) != got
    np.testing.assert_array_equal(differs, [False, True, True, False, False, False, False, False])
    assert (got[differs] == -1).all() and (np.trunc(x)[differs] == 0).all()
    np.testing.assert_array_equal(cr.voxel_coords(np.array([[-0.0, -1e-30, 0.25]]), 0.5), [[0, -1, 0]])


@pytest.mark.parametrize("res", [0.2, 1.0])
def test_voxel_coords_and_merge_equal_the_numpy_map(kitti07, res):
    """oracle.vgicp_oracle_np.VoxelMapNP: coordinates and counts exact, means and covariances to 1e-12"""
    for i in range(3):
        p, c = kitti07[f"points_{i}"], kitti07[f"covs_{i}"]
        np.testing.assert_array_equal(cr.voxel_coords(p.astype(np.float64), res), onp.fast_floor(p.astype(np.float64) * (1.0 / res)))
        m = onp.VoxelMapNP(res)
        m.insert(p, c)
        got = cr.merge(p, cr.covs9(c), None, res)
        idx = np.array([m.index[tuple(k)] for k in got["coords"].tolist()])
        assert len(set(idx.tolist())) == m.num_voxels == len(got["coords"])
        np.testing.assert_array_equal(got["counts"], m.num_points[idx])
        np.testing.assert_array_equal(got["counts"], np.bincount(got["voxel_of"]))
        assert np.abs(got["means"] - m.means[idx]).max() < 1e-12
        assert np.abs(got["covs"].reshape(-1, 3, 3).transpose(0, 2, 1) - m.covs[idx]).max() < 1e-12
        np.testing.assert_array_equal(m.lookup(p.astype(np.float64)), idx[got["voxel_of"]])
        np.testing.assert_array_equal(cr.lookup(m.coords, p, np.eye(4), res), m.lookup(p.astype(np.float64)))


@pytest.mark.parametrize("res", [0.2, 1.0])
def test_transform_then_merge_equals_the_cpu_statement(kitti07, res):
    """oracle.merge_frames (the C map behind it) on the kitti07 frames: same voxels, exact counts, means / covariances to 1e-12, max intensities equal"""
    rng = np.random.default_rng(5)
    poses = [np.asarray(T, dtype=np.float64) for T in kitti07["poses"][:3]]
    host = [(kitti07[f"points_{i}"], kitti07[f"covs_{i}"], (rng.integers(0, 128, len(kitti07[f"points_{i}"])) + 128).astype(np.float32) if i != 1 else None) for i in range(3)]
    coords, means, covs, intens = oracle.merge_frames(poses, host, res)
    t = cr.transform(poses, [(p, cr.covs9(c), it) for p, c, it in host])
    np.testing.assert_array_equal(t["begin"], [0, len(host[0][0]), len(host[0][0]) + len(host[1][0])])
    got = cr.merge(t["points"].astype(np.float32), t["covs"].astype(np.float32), t["intensities"], res)
    order = {tuple(k): i for i, k in enumerate(np.asarray(coords).tolist())}
    idx = np.array([order[tuple(k)] for k in got["coords"].tolist()])
    assert len(set(idx.tolist())) == len(coords) == len(got["coords"])
    assert np.abs(got["means"] - means[idx]).max() < 1e-12
    assert np.abs(got["covs"].reshape(-1, 3, 3).transpose(0, 2, 1) - covs[idx]).max() < 1e-12
    np.testing.assert_array_equal(got["intensities"], np.asarray(intens)[idx].astype(np.float32))


def test_transform_stays_inside_its_half_of_the_bound():
    """the restatement against the same products in extended precision: one evaluation errs by at most 4 * 2^-53 S_p and 6 * 2^-53 S_c, half of what
    transform_bounds allows two evaluations; frame i lies at begin_i; a frame without intensities gives zeros; a transposed product would show"""
    poses, frames = cr.transform_case(expmap)
    t = cr.transform(poses, frames)
    np.testing.assert_array_equal(t["begin"], np.concatenate([[0], np.cumsum(cr.FRAME_SIZES)[:-1]]))
    assert len(t["points"]) == sum(cr.FRAME_SIZES)
    ld = np.longdouble
    assert np.finfo(ld).eps < 2.0**-60  # (an extended type is needed for this check to mean anything)
    worst_p = worst_c = 0.0
    for T, (p, c, it), b, n in zip(poses, frames, t["begin"], cr.FRAME_SIZES):
        if n == 0:
            continue
        R, tr = np.asarray(T[:3, :3], dtype=ld), np.asarray(T[:3, 3], dtype=ld)
        want_p = np.einsum("ij,nj->ni", R, p.astype(ld)) + tr
        C = c.astype(ld).reshape(n, 3, 3).transpose(0, 2, 1)
        want_c = np.einsum("ij,njk,lk->nil", R, C, R).transpose(0, 2, 1).reshape(n, 9)
        rows = slice(b, b + n)
        worst_p = max(worst_p, float((np.abs(t["points"][rows] - want_p) / (4 * cr.U53 * t["S_p"][rows])).max()))
        worst_c = max(worst_c, float((np.abs(t["covs"][rows] - want_c) / (6 * cr.U53 * t["S_c"][rows])).max()))
        wrong = np.einsum("ij,njk,lk->nil", R, C.transpose(0, 2, 1), R).transpose(0, 2, 1).reshape(n, 9)  # C read row-major
        assert (np.abs(wrong - want_c) > 1e3 * cr.transform_bounds(t, t["points"], t["covs"])[1][rows]).any()
        np.testing.assert_array_equal(t["intensities"][rows], np.zeros(n, np.float32) if it is None else it)
    print(f"restatement vs extended precision: worst error / (4 u S_p) = {worst_p:.3f}, / (6 u S_c) = {worst_c:.3f}")
    assert worst_p <= 1.0 and worst_c <= 1.0
    bp, bc = cr.transform_bounds(t, t["points"].astype(np.float32), t["covs"].astype(np.float32))
    assert (np.abs(t["points"].astype(np.float32) - t["points"]) <= bp).all() and (np.abs(t["covs"].astype(np.float32) - t["covs"]) <= bc).all()


def test_lattice_lookup_and_closed_form_counts():
    """the lattice of the exact-arithmetic tests: every point is found in the map of the whole lattice, in the voxel its floor names; the sign cases go where a floor
    sends them (-0.0 to cell 0, the smallest negative normal to cell -1); under the exact pose the merge counts are the closed form"""
    pts = cr.lattice()
    assert len(pts) == 17**3 + 2 * 17**2
    u = pts[: 17**3].astype(np.float64) * 2.0  # q * inv_leaf at leaf 0.5: exact, and more than half of the coordinates sit on a face
    assert (u * 2.0 == np.rint(u * 2.0)).all() and (u == np.floor(u)).mean() > 0.5
    m = cr.merge(pts, np.zeros((len(pts), 9), np.float32), None, 0.5)
    idx = cr.lookup(m["coords"], pts, np.eye(4), 0.5)
    assert (idx >= 0).all()
    np.testing.assert_array_equal(m["coords"][idx], np.floor(pts.astype(np.float64) / 0.5).astype(np.int64))
    neg0 = pts[17**3 : 17**3 + 17**2]
    tiny = pts[17**3 + 17**2 :]
    assert np.signbit(neg0[:, 0]).all() and (cr.voxel_coords(neg0.astype(np.float64), 0.5)[:, 0] == 0).all()
    assert (tiny[:, 0] < 0).all() and (cr.voxel_coords(tiny.astype(np.float64), 0.5)[:, 0] == -1).all()
    hp = cr.lattice_half(pts)
    half = cr.merge(hp, np.zeros((len(hp), 9), np.float32), None, 0.5)
    for T in (np.eye(4), cr.PERM_POSE):
        got = cr.lookup(half["coords"], pts, T, 0.5)
        assert (got >= 0).any() and (got < 0).any()
    grid = pts[: 17**3]
    q = cr.transform_points(cr.PERM_POSE, grid)
    np.testing.assert_array_equal(q, np.stack([-grid[:, 1] + 1.5, grid[:, 0] - 2.0, grid[:, 2] + 0.5], axis=1).astype(np.float64))
    mg = cr.merge(q.astype(np.float32), np.zeros((len(q), 9), np.float32), None, 0.5)
    np.testing.assert_array_equal(mg["counts"], cr.lattice_counts(mg["coords"]))
    assert len(mg["coords"]) == 9**3 and mg["counts"].sum() == 17**3


def test_non_finite_points_and_the_origin():
    """a map that holds voxel (0, 0, 0): no non-finite point is found there or anywhere; the origin itself is found, also under surface validation"""
    coords = np.array([[0, 0, 0], [2, 2, 2], [-1, -1, -1]])
    bad = cr.nonfinite_cases()
    assert len(bad) == 15 and not np.isfinite(bad).all(axis=1).any()
    pts = np.concatenate([[[0.1, 0.2, 0.3]], bad, [[0.0, 0.0, 0.0], [1.1, 1.2, 1.3]]]).astype(np.float32)
    for T in (np.eye(4), expmap(cr.XIS["small"])):
        idx = cr.lookup(coords, pts, T, 0.5)
        assert (idx[1:16] == -1).all()
    idx = cr.lookup(coords, pts, np.eye(4), 0.5)
    np.testing.assert_array_equal(idx[[0, 16, 17]], [0, 0, 1])
    assert cr.overlap_hits([(coords, 0.5, np.eye(4))], pts) == 3
    normals = np.tile(np.float32([0.0, 0.0, 1.0]), (len(pts), 1))
    withn = cr.lookup(coords, pts, np.eye(4), 0.5, normals)
    assert withn[16] == 0  # |q| = 0: not rejected
    assert withn[0] == -1 and withn[17] == -1  # cos = 0.80 and 0.62 > 0.174: rejected


def _assert_face(points, T, res, what):
    m = cr.face_margin(points, T, res)
    assert m > cr.MARGIN, f"{what}: a coordinate lies {m:.2e} cells (relative) from a voxel face: two f64 evaluations could floor it differently"
    return m


def test_every_named_input_keeps_its_margin(kitti00):
    """the margin assertions of tests/test_cloud_edges_gpu.py, for every input it names (identity poses and the exact lattice poses are exempt)"""
    sp = kitti00["source_points"]
    normals = cr.unit_normals(len(sp))
    faces, surfaces = [], []
    for name in ("small", "large"):
        T = expmap(cr.XIS[name])
        for res in (0.5, 1.0, 0.3):
            faces.append(_assert_face(sp, T, res, f"source_points, {name} pose, {res} m"))  # (every slice of the scan is a subset of this)
        s = cr.surface_margin(sp, normals, T)
        assert s > cr.MARGIN, f"{name} pose: a cosine lies {s:.2e} from the threshold"
        surfaces.append(s)
        rejected = (cr._cosines(T, cr.transform_points(T, sp), normals) > cr.SURFACE_THRESH).mean()
        assert 0.3 < rejected < 0.6  # the validation decides something
    assert cr.surface_margin(sp, normals, np.eye(4)) > cr.MARGIN
    for xi, res in zip(cr.UNION_XIS, cr.UNION_RES):
        if np.any(xi):
            faces.append(_assert_face(sp, expmap(xi), res, f"union target at {res} m"))
    us, far = cr.union_source(sp)
    for name, res in (("small", 0.5), ("large", 1.0)):
        faces.append(_assert_face(us, expmap(cr.XIS[name]), res, f"union source with the far points, {name} pose, {res} m"))
    srcs = cr.batch_sources(sp)
    assert [len(s) for s in srcs] == cr.BATCH_SIZES
    for k, name, res in cr.BATCH_PAIRS:
        if name != "identity" and len(srcs[k]):
            faces.append(_assert_face(srcs[k], expmap(cr.XIS[name]), res, f"batch source {k}, {name} pose, {res} m"))
    print(f"smallest relative face margin {min(faces):.2e}, smallest surface margin {min(surfaces):.2e}")

"""numpy restatement, f64 on the f32 inputs, of the per-point index arithmetic around the Gaussian voxel map: the lookup, the overlap counts, the frame transform and
the merge.  A helper, not a test; it reads nothing outside the repository.  (Reference lines relative to the reference's source tree.)

  fast_floor(x)                      include/gtsam_points/util/fast_floor.hpp:12-15      int(x) - (x < int(x)): truncate toward zero, then fix the negatives
  voxel_coords(q, res)               src/gtsam_points/types/gaussian_voxelmap_cpu.cpp:59-61   fast_floor(q * (1.0 / res)) -- the CPU map's rule, which the device
                                     adopts (csrc/gp_device.hpp: fast_floor in double; inv_leaf = 1.0 / resolution, hence the multiplication by the reciprocal)
  lookup(coords, points, delta, ..)  include/gtsam_points/cuda/kernels/lookup_voxels.cuh:34-60   q = R p + t with the 3x3 block as given; with normals the point is
                                     dropped when q.normalized() . (R n) > 0.174 (:42-50, :86); then the voxel that holds q, or -1.  |q| = 0 does not reject: Eigen's
                                     normalized() of a zero vector is the zero vector, the device's 0 * inf is a NaN that compares false.  A non-finite q has no voxel
                                     (csrc/gp_device.hpp finite3; the reference floors it into an undefined integer).
  overlap_hits(targets, points)      src/gtsam_points/types/gaussian_voxelmap_gpu_funcs.cu:156-182,192-236,265-335   a point counts once if it falls into a voxel of
                                     ANY target (bool_or_kernel); the single-target form is a list of one, the pairwise batch (:337-404) one call per pair
  transform(poses, frames)           gaussian_voxelmap_gpu_funcs.cu:42-62,93-114   p' = R p + t, C' = R C R^T (C as stored, not symmetrised), intensities copied, zeros
                                     for a frame without; frame i occupies the rows [begin_i, begin_i + n_i) of the output
  merge(points, covs, ints, res)     gaussian_voxelmap_gpu_funcs.cu:118-149 + gaussian_voxelmap_gpu.cu:92-172   per voxel: count, mean point, mean covariance (the
                                     full 3x3 as given), max intensity

The lookup works on the map's own coordinate list (GaussianVoxelMapGPU.download_f64()[0]): row v of that list is voxel v, so "the right voxel" is an index, not a mask.

A floor and a threshold are discontinuous: two correct f64 evaluations of R p + t (one contracting a * b + c into a fused multiply-add, one not) agree on them only
away from the discontinuity.  face_margin / surface_margin say how far the nearest point is from one; the tests assert the margin before they compare (except where the
arithmetic is exact: identity, axis permutations and sign flips, translations by multiples of the leaf with the points on a power-of-two lattice).

Voxel coordinates at or beyond +-2^31 cells are out of scope: the reference converts them to int, which is undefined there, and nothing here or in the tests goes near.
"""
import numpy as np

SURFACE_THRESH = 0.174  # lookup_voxels.cuh:86
U53 = 2.0 ** -53


def fast_floor(x):
    """fast_floor.hpp:13-14 on an f64 array -> int64"""
    x = np.asarray(x, dtype=np.float64)
    n = np.trunc(x)
    return (n - (x < n)).astype(np.int64)


def _f64(a, width):
    return np.asarray(a, dtype=np.float32).reshape(-1, width).astype(np.float64)


def voxel_coords(q, res):
    """q: f64 (N,3), finite -> int64 (N,3)"""
    return fast_floor(np.asarray(q, dtype=np.float64) * (1.0 / float(res)))


def transform_points(delta, points):
    """R p + t in f64, summed left to right as the kernels write it (three products, three additions); the 3x3 block as given"""
    T = np.asarray(delta, dtype=np.float64)
    p = _f64(points, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([T[r, 0] * x + T[r, 1] * y + T[r, 2] * z + T[r, 3] for r in range(3)], axis=1)


def _cosines(delta, q, normals):
    """q.normalized() . (R n) per point; NaN where |q| = 0"""
    T = np.asarray(delta, dtype=np.float64)
    n = _f64(normals, 3)
    tn = np.stack([T[r, 0] * n[:, 0] + T[r, 1] * n[:, 1] + T[r, 2] * n[:, 2] for r in range(3)], axis=1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return (q * tn).sum(axis=1) / np.sqrt((q * q).sum(axis=1))


def coord_index(coords_of_map):
    """{(x, y, z): row}; a coordinate that appears twice is a broken map"""
    rows = np.asarray(coords_of_map).reshape(-1, 3).tolist()
    index = {tuple(c): i for i, c in enumerate(rows)}
    assert len(index) == len(rows), "the map lists a voxel coordinate twice"
    return index


def lookup(coords_of_map, points, delta, res, normals=None):
    """-> int64 [N]: the row of coords_of_map that holds R p + t, or -1"""
    index = coords_of_map if isinstance(coords_of_map, dict) else coord_index(coords_of_map)
    q = transform_points(delta, points)
    ok = np.isfinite(q).all(axis=1)
    if normals is not None:
        with np.errstate(invalid="ignore"):
            ok &= ~(_cosines(delta, q, normals) > SURFACE_THRESH)  # a NaN cosine (|q| = 0) compares false: not rejected
    out = np.full(len(q), -1, np.int64)
    live = np.flatnonzero(ok)
    out[live] = [index.get(tuple(c), -1) for c in voxel_coords(q[live], res).tolist()]
    return out


def face_margin(points, delta, res):
    """the smallest distance, in cells, of a transformed coordinate from an integer, relative to max(|u|, 1); inf for no finite point"""
    q = transform_points(delta, points)
    u = q[np.isfinite(q).all(axis=1)] * (1.0 / float(res))
    if u.size == 0:
        return np.inf
    return float((np.abs(u - np.rint(u)) / np.maximum(np.abs(u), 1.0)).min())


def surface_margin(points, normals, delta):
    """the smallest |cos - 0.174| over the finite points with |q| > 0"""
    q = transform_points(delta, points)
    c = _cosines(delta, q, normals)
    c = c[np.isfinite(c)]
    return float(np.abs(c - SURFACE_THRESH).min()) if c.size else np.inf


def overlap_mask(targets, points):
    """targets: [(coords_of_map, res, delta)] -> bool [N]: the point falls into a voxel of any target"""
    hit = np.zeros(len(np.asarray(points).reshape(-1, 3)), bool)
    for coords, res, delta in targets:
        hit |= lookup(coords, points, delta, res) >= 0
    return hit


def overlap_hits(targets, points):
    return int(overlap_mask(targets, points).sum())


def transform(poses, frames):
    """frames: [(points f32 (n,3), covs f32 (n,9) column-major as stored, or None, intensities f32 (n,) or None)], one 4x4 pose each.
    -> dict(begin int [F] (row of the frame's first point), points f64 (N,3), covs f64 (N,9) column-major, intensities f32 [N],
            S_p (N,3) = |R||p| + |t|, S_c (N,9) = |R||C||R^T|: the sums of the absolute values of the terms, entry by entry)
    Every sum has three terms and is formed left to right, R C first, then (R C) R^T: a term of p' passes at most four roundings (its product and three
    additions), a three-factor term of C' at most six (product and two additions in R C, the same again in (R C) R^T)."""
    sizes = [len(np.asarray(f[0]).reshape(-1, 3)) for f in frames]
    begin = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64) if frames else np.zeros(0, np.int64)
    P, Cv, I, SP, SC = [np.zeros((0, 3))], [np.zeros((0, 9))], [np.zeros(0, np.float32)], [np.zeros((0, 3))], [np.zeros((0, 9))]
    for T, (pts, covs, ints), n in zip(poses, frames, sizes):
        T = np.asarray(T, dtype=np.float64)
        R, t = T[:3, :3], T[:3, 3]
        p = _f64(pts, 3)
        P.append(transform_points(T, pts))
        SP.append(np.abs(p) @ np.abs(R).T + np.abs(t))
        c = _f64(covs, 9).reshape(n, 3, 3).transpose(0, 2, 1) if covs is not None else np.zeros((n, 3, 3))  # c[:, r, col] = C(r, col)
        RC = np.stack([np.stack([R[r, 0] * c[:, 0, col] + R[r, 1] * c[:, 1, col] + R[r, 2] * c[:, 2, col] for col in range(3)], axis=1) for r in range(3)], axis=1)
        out = np.stack([np.stack([RC[:, r, 0] * R[col, 0] + RC[:, r, 1] * R[col, 1] + RC[:, r, 2] * R[col, 2] for col in range(3)], axis=1) for r in range(3)], axis=1)
        Cv.append(out.transpose(0, 2, 1).reshape(n, 9))
        SC.append(np.einsum("ij,njk,lk->nil", np.abs(R), np.abs(c), np.abs(R)).transpose(0, 2, 1).reshape(n, 9))
        I.append(np.zeros(n, np.float32) if ints is None else np.asarray(ints, dtype=np.float32).reshape(n))
    return dict(begin=begin, sizes=np.asarray(sizes, np.int64), points=np.concatenate(P), covs=np.concatenate(Cv), intensities=np.concatenate(I), S_p=np.concatenate(SP),
                S_c=np.concatenate(SC))


def ulp32(x):
    """the spacing of float32 at |x| (x: f64 array)"""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def transform_bounds(ref, got_points, got_covs=None):
    """|got - ref| per entry may reach half an f32 spacing (the one rounding to f32) plus the f64 roundings of two evaluations: 2 * 4 per term of a point,
    2 * 6 per three-factor term of a covariance, each 2^-53 of the term's absolute value -> (bound_points (N,3), bound_covs (N,9) or None)"""
    gp = np.asarray(got_points, dtype=np.float64)
    bp = 0.5 * ulp32(np.maximum(np.abs(gp), np.abs(ref["points"]))) + 8 * U53 * ref["S_p"]
    bc = None
    if got_covs is not None:
        gc = np.asarray(got_covs, dtype=np.float64)
        bc = 0.5 * ulp32(np.maximum(np.abs(gc), np.abs(ref["covs"]))) + 12 * U53 * ref["S_c"]
    return bp, bc


def merge(points_f32, covs_f32, intensities, res):
    """points (N,3), covs (N,9) column-major as stored, intensities (N,) or None -> dict(coords int64 (V,3) in lexicographic order, counts [V], means f64 (V,3),
    covs f64 (V,9) column-major, intensities f32 [V] (max over the voxel; 0 without intensities), voxel_of int64 [N]).  Every point must be finite."""
    p, c = _f64(points_f32, 3), _f64(covs_f32, 9)
    n = len(p)
    it = np.zeros(n, np.float32) if intensities is None else np.asarray(intensities, dtype=np.float32).reshape(n)
    coords, voxel_of, counts = np.unique(voxel_coords(p, res), axis=0, return_inverse=True, return_counts=True)
    voxel_of = voxel_of.reshape(-1)
    V = len(coords)
    means, covs, imax = np.zeros((V, 3)), np.zeros((V, 9)), np.zeros(V, np.float32)
    np.add.at(means, voxel_of, p)
    np.add.at(covs, voxel_of, c)
    np.maximum.at(imax, voxel_of, it)
    return dict(coords=coords, counts=counts, means=means / counts[:, None], covs=covs / counts[:, None], intensities=imax, voxel_of=voxel_of)


def symmetric_part(covs9):
    """0.5 (C + C^T) of column-major rows: what the device map keeps of a covariance (csrc/gp_voxelmap_kernels.hpp, segmented_stats_kernel)"""
    c = np.asarray(covs9, dtype=np.float64).reshape(-1, 3, 3)
    return (0.5 * (c + c.transpose(0, 2, 1))).reshape(-1, 9)


# ---- the inputs the GPU tests name; tests/test_cloud_ref_cpu.py asserts the margins of every one of them ------------------------------------------------------------
MARGIN = 1e-9  # tests/test_icp_gpu.py
XIS = {"small": [0.01, -0.02, 0.015, 0.10, -0.05, 0.03], "large": [0.2, -0.1, 0.3, 1.0, -2.0, 0.5]}
SIZES = [1, 63, 64, 65, 255, 256, 257, 513]
FRAME_SIZES = [0, 1, 255, 256, 257, 0, 513, 0]
BATCH_SIZES = [257, 0, 1, 256, 0, 513]
UNION_RES = [0.3, 0.5, 1.0, 0.5, 2.0]
UNION_XIS = [XIS["small"], XIS["large"], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0], [-0.05, 0.03, 0.1, -0.4, 0.7, -0.2], [0.3, 0.2, -0.25, 2.0, 1.5, -1.0]]
PERM_POSE = np.array([[0.0, -1.0, 0.0, 1.5], [1.0, 0.0, 0.0, -2.0], [0.0, 0.0, 1.0, 0.5], [0.0, 0.0, 0.0, 1.0]])  # 90 degrees about z, translation = multiples of 0.5


def unit_normals(n, seed=3):
    """normals from default_rng(seed), normalised and rounded to f32"""
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def lattice():
    """k * 0.25 for k in -8..8 per axis (4913 points), then the same lattice's x = 0 plane with x = -0.0 and with x = the smallest negative f32 normal:
    every coordinate, and every coordinate * 2, is exact in f32 and f64"""
    k = np.arange(-8, 9) * 0.25
    g = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3)
    plane = g[g[:, 0] == 0.0]
    neg0, tiny = plane.copy(), plane.copy()
    neg0[:, 0] = -0.0
    tiny[:, 0] = -float(np.finfo(np.float32).tiny)
    return np.concatenate([g, neg0, tiny]).astype(np.float32)


def nonfinite_cases():
    """NaN, +inf and -inf in each coordinate alone, and combined: 15 rows of (x, y, z) with 1.0 where nothing is put"""
    rows = []
    for bad in (np.nan, np.inf, -np.inf):
        for axis in range(3):
            r = [1.0, 1.0, 1.0]
            r[axis] = bad
            rows.append(r)
        rows.append([bad, bad, bad])
    rows += [[np.nan, np.inf, -np.inf], [np.inf, -np.inf, 1.0], [1.0, np.nan, np.inf]]
    return np.array(rows, dtype=np.float32)


def covs9(covs):
    """(N,3,3) indexed (row, col) -> float32 (N,9) column-major, the device layout"""
    return np.ascontiguousarray(np.asarray(covs, dtype=np.float32).reshape(-1, 3, 3).transpose(0, 2, 1)).reshape(-1, 9)


def union_source(source_points):
    """400 points of the scan, then 100 points of it moved 1000 m along x: a target built from those 100 alone is the only one that can hold them.
    -> (points f32 (500,3), indices of the far points)"""
    far = (source_points[400:500] + np.float32([1000.0, 0.0, 0.0])).astype(np.float32)
    return np.concatenate([source_points[:400], far]).astype(np.float32), np.arange(400, 500)


BATCH_STARTS = [0, 0, 305, 306, 0, 557]  # (point 305 lies in a voxel of the 0.5 m map under the identity: the source of one point is a hit)
BATCH_PAIRS = [(0, "small", 0.5), (1, "large", 0.3), (2, "identity", 0.5), (3, "large", 0.3), (4, "small", 0.5), (5, "small", 0.3), (0, "large", 0.3)]  # (source, pose, map)


def batch_sources(source_points):
    """six sources of BATCH_SIZES points (two of them empty), cut from the scan at different offsets"""
    return [np.ascontiguousarray(source_points[s : s + n], dtype=np.float32) for s, n in zip(BATCH_STARTS, BATCH_SIZES)]


def transform_case(expmap, seed=11):
    """the frames of the gp_transform_frames test: FRAME_SIZES points each (three frames empty), random non-symmetric 3x3 covariances, intensities for some frames;
    the non-empty frames get, in order, three rigid poses, one general 3x3 block R (I + 1e-3 G) and one rigid pose with a translation of order 1e4.
    -> (poses [F] of 4x4 f64, frames [F] of (points f32 (n,3), covs f32 (n,9), intensities f32 (n,) or None))"""
    rng = np.random.default_rng(seed)
    general = expmap([0.4, -0.3, 0.2, 3.0, -1.0, 2.0])
    general[:3, :3] = general[:3, :3] @ (np.eye(3) + 1e-3 * rng.normal(size=(3, 3)))
    far = expmap([-0.2, 0.5, 0.1, 0.0, 0.0, 0.0])
    far[:3, 3] = [1.2345e4, -9.8765e3, 4.321e3]
    live = iter([expmap(XIS["small"]), expmap(XIS["large"]), expmap(UNION_XIS[4]), general, far])
    poses, frames = [], []
    for i, n in enumerate(FRAME_SIZES):
        poses.append(next(live) if n else expmap([0.1 * i, 0.0, 0.0, 1.0, 2.0, 3.0]))
        pts = (rng.normal(size=(n, 3)) * 30.0).astype(np.float32)
        cov = rng.normal(size=(n, 9)).astype(np.float32)
        ints = rng.uniform(0.0, 255.0, size=n).astype(np.float32) if i in (2, 4, 5) else None
        frames.append((pts, cov, ints))
    return poses, frames


def lattice_counts(coords, leaf_shift=(3, -4, 1)):
    """points per voxel of the 17^3 lattice k * 0.25 (k = -8..8) at leaf 0.5 after PERM_POSE: along every axis the cells -4..3 (before the translation's shift by
    whole cells) hold two lattice values each and cell 4 holds one (k = 8, or k = -8 where the axis is negated), so a voxel holds 2^(axes not in cell 4) points"""
    base = np.asarray(coords, dtype=np.int64) - np.asarray(leaf_shift, dtype=np.int64)
    assert (base >= -4).all() and (base <= 4).all()
    return np.where(base == 4, 1, 2).prod(axis=1)


def lattice_half(points):
    """the part of the lattice with y < 0: a map built from it misses the other half"""
    return np.ascontiguousarray(points[points[:, 1] < 0.0])

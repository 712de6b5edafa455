"""numpy / math.fsum restatement, f64 on the f32 inputs, of the Gaussian voxel-map BUILD, and the generators of the edge cases the tests of the build use.
A helper, not a test; it reads nothing outside the repository and does not use oracle/.  (Reference lines relative to the reference's source tree.)

  coordinates   floor(float64(p) * (1 / res)), the reciprocal taken once        src/gtsam_points/types/gaussian_voxelmap_cpu.cpp:59-61 + util/fast_floor.hpp:12-15
                (the CPU map's rule, which the device adopts: csrc/gp_device.hpp fast_floor, inv_leaf = 1.0 / resolution)
  valid points  all three |p * (1 / res)| < 1e9 -- false for NaN and +-inf.  The project's rule (csrc/gp_binning.hip point_cell); the reference floors such a
                point into an undefined integer.  An invalid point belongs to no voxel and counts nowhere.
  per voxel     count; mean = sum(p) / n; covariance = sum(sym(C)) / n with sym(C) = (C + C^T) / 2 of the f32 3x3 as stored; every sum by math.fsum (correctly
                rounded whatever the order), one division
  intensity     gaussian_voxelmap_cpu.cpp:34-35 (GaussianVoxel::add): intensity = std::max(intensity, x) from the 0.0 of gaussian_voxelmap_cpu.hpp:21, i.e.
                `cur < x ? x : cur`: a negative value, -0.0 and a NaN all leave +0.0; +inf wins.  The reference's GPU map (gaussian_voxelmap_gpu.cu:138-139) does
                atomicMax on the float's BIT PATTERN from 0 instead, which agrees for x >= +0 only: any negative value, -0.0 or a NaN beats every positive one
                there.  The two reference maps differ, and the project follows the CPU map: it is the parity target of every statistic of the map,
                its rule is an order on the VALUES, and the merge of frames on the CPU states the same rule (gaussian_voxelmap_cpu_funcs.cpp:101).
                Without intensities every voxel has 0.0 (gaussian_voxelmap_gpu.cu:236-242).
  insert        replaces the map: create_bucket_table allocates a new table and insert new arrays, zeroed (gaussian_voxelmap_gpu.cu:217-225,295-296); nothing
                of an earlier cloud survives.  (The CPU map accumulates; the GPU class is the one restated here.)

What the device stores (csrc/gp_voxelmap_kernels.hpp): mean_local = float32(sum(p - centre) / n) with centre = (coord + 0.5) * res in f64; download_f64 returns
centre + float64(mean_local); the f32 arrays are float32(centre + sum(p - centre) / n) and float32(cov).  `Map.means_stored` is that first quantity from fsum.

The build's path (csrc/gp_binning.hip bin_points_once): blocks of 4 x 4 x 4 voxels over the bounding box of the valid points; more than 2^24 blocks -> the hashed
build; else key_bits = the smallest b >= 7 with 2^b - 1 >= 64 * blocks, and the radix sort runs (key_bits + 7) // 8 passes.
"""
import math

import numpy as np

LIMIT = 1.0e9               # gp_binning.hip point_cell
MAX_GRID_BLOCKS = 1 << 24   # gp_binning.hpp kMaxGridBlocks
STATS_BATCH = 512           # gp_voxelmap_kernels.hpp kStatsBatch
STATS_GROUP = 16            # lanes per voxel = voxels per workgroup of segmented_stats_kernel
POPULATIONS = (1, 15, 16, 17, 31, 33, 511, 512, 513, 1025, 5000)
FACE_RESOLUTIONS = (0.5, 0.1, 0.3, 1e-3, 100.0)
FAR_DISTANCES = (0.0, 1e2, 1e3, 1e4, 1e5)


def coord_hash(coord):
    """vector3i_hash of cuda/kernels/vector3_hash.cuh:14-39 (csrc/gp_device.hpp coord_hash): boost-style hash_combine of the three sign-extended coordinates in uint64"""
    M, mask = 0xC6A4A7935BD1E995, (1 << 64) - 1
    h = 0
    for c in coord:
        k = ((int(c) & mask) * M) & mask
        k ^= k >> 47
        k = (k * M) & mask
        h = (((h ^ k) * M) & mask) + 0xE6546B64 & mask
    return h


def entry_bucket_count(init_num_buckets, num_voxels, load_percent=33):
    """csrc/gp_voxelmap.hip entry_bucket_count: where the binned build and the incremental insert enter the doubling sequence of the bucket table"""
    n = init_num_buckets
    while n * load_percent < 100 * num_voxels:
        n *= 2
    return n


def buckets_can_place(coords, num_buckets, max_scan):
    """insert_voxels_kernel's claim in any order: with max_scan == 1 every voxel has ONE bucket, so the table holds them iff their home buckets are distinct; for longer
    chains a greedy first-fit in list order (the device's order is not fixed, so only max_scan == 1 is order-free: the callers use that)"""
    taken = set()
    for c in coords:
        h = coord_hash(c)
        for i in range(max_scan):
            b = ((h + i) & ((1 << 64) - 1)) % num_buckets
            if b not in taken:
                taken.add(b)
                break
        else:
            return False
    return True


def fast_floor(x):
    """fast_floor.hpp:13-14 on an f64 array -> int64"""
    x = np.asarray(x, dtype=np.float64)
    n = np.trunc(x)
    return (n - (x < n)).astype(np.int64)


def _p64(points):
    return np.asarray(points, dtype=np.float32).reshape(-1, 3).astype(np.float64)


def scaled(points, res):
    with np.errstate(invalid="ignore", over="ignore"):
        return _p64(points) * (1.0 / float(res))


def valid_mask(points, res):
    with np.errstate(invalid="ignore"):
        return (np.abs(scaled(points, res)) < LIMIT).all(axis=1)


def voxel_coords(points, res):
    """int64 (N,3); rows of invalid points are 0 and mean nothing"""
    u = scaled(points, res)
    return fast_floor(np.where(valid_mask(points, res)[:, None], u, 0.0))


def intensity_max(values):
    """std::max from 0.0f over f32 values, in order: cur < x ? x : cur"""
    cur = np.float32(0.0)
    for x in np.asarray(values, dtype=np.float32).tolist():
        if cur < x:
            cur = np.float32(x)
    return np.float32(cur)


def sym6(covs9):
    """f32 (N,9) column-major 3x3 -> f64 (N,6): xx xy xz yy yz zz of the symmetric part"""
    c = np.asarray(covs9, dtype=np.float32).reshape(-1, 9).astype(np.float64)
    return np.stack([c[:, 0], 0.5 * (c[:, 3] + c[:, 1]), 0.5 * (c[:, 6] + c[:, 2]), c[:, 4], 0.5 * (c[:, 7] + c[:, 5]), c[:, 8]], axis=1)


def _full(c6):
    xx, xy, xz, yy, yz, zz = (c6[:, k] for k in range(6))
    return np.stack([xx, xy, xz, xy, yy, yz, xz, yz, zz], axis=1).reshape(-1, 3, 3)


class Map:
    """coords int64 (V,3) in lexicographic order, counts, means / covs f64, intensities f32, point_voxel int64 (N,) (-1 = invalid point)"""

    def __init__(self, points, covs9, intensities, res, order=None):
        p = _p64(points)
        s6 = sym6(covs9)
        ok = valid_mask(points, res)
        coords = voxel_coords(points, res)
        self.res = float(res)
        self.n = len(p)
        uniq, inv = np.unique(coords[ok], axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        self.coords = uniq.reshape(-1, 3)
        V = len(self.coords)
        self.point_voxel = np.full(len(p), -1, dtype=np.int64)
        self.point_voxel[ok] = inv
        self.index = {tuple(c): i for i, c in enumerate(self.coords.tolist())}
        self.counts = np.bincount(inv, minlength=V).astype(np.int64)
        self.means = np.zeros((V, 3))
        self.means_stored = np.zeros((V, 3))
        self.max_abs_cov = np.zeros(V)
        c6 = np.zeros((V, 6))
        self.intensities = np.zeros(V, dtype=np.float32)
        rows = np.flatnonzero(ok)[np.argsort(inv, kind="stable")]
        if order is not None:  # another order of summation and of the intensity maximum: the result must not depend on it
            rows = order(rows, inv)
        starts = np.concatenate([[0], np.cumsum(self.counts)])
        it = None if intensities is None else np.asarray(intensities, dtype=np.float32).reshape(-1)
        centre = (self.coords.astype(np.float64) + 0.5) * self.res
        for v in range(V):
            r = rows[starts[v] : starts[v + 1]]
            n = float(len(r))
            for k in range(3):
                self.means[v, k] = math.fsum(p[r, k].tolist()) / n
                self.means_stored[v, k] = centre[v, k] + float(np.float32(math.fsum((p[r, k] - centre[v, k]).tolist()) / n))
            for k in range(6):
                c6[v, k] = math.fsum(s6[r, k].tolist()) / n
            self.max_abs_cov[v] = np.abs(s6[r]).max()
            if it is not None:
                self.intensities[v] = intensity_max(it[r])
        self.covs = _full(c6)
        self.centres = centre

    @property
    def num_voxels(self):
        return len(self.coords)


def reversed_rows(rows, inv):
    """an `order` for Map: every voxel's rows back to front"""
    inv_sorted = np.sort(inv, kind="stable")
    out = rows.copy()
    starts = np.flatnonzero(np.concatenate([[True], inv_sorted[1:] != inv_sorted[:-1], [True]]))
    for a, b in zip(starts[:-1], starts[1:]):
        out[a:b] = rows[a:b][::-1]
    return out


def predicted_path(points, res):
    """"hashed", or the number of radix passes of the binned build (gp_binning.hip bin_points_once); None for a cloud without a valid point"""
    ok = valid_mask(points, res)
    if not ok.any():
        return None
    blocks = voxel_coords(points, res)[ok] >> 2
    dims = blocks.max(axis=0) - blocks.min(axis=0) + 1
    nb = int(dims[0]) * int(dims[1]) * int(dims[2])
    if nb > MAX_GRID_BLOCKS:
        return "hashed"
    key_bits = 7
    while (1 << key_bits) - 1 < nb * 64:
        key_bits += 1
    return (key_bits + 7) // 8


def face_margin_ulps(points, res):
    """per point: the smallest distance of a p * (1 / res) to an integer, in ulps of it; 0 where it IS an integer.  inf for invalid points"""
    u = scaled(points, res)
    with np.errstate(invalid="ignore"):
        d = np.abs(u - np.rint(u)) / np.spacing(np.maximum(np.abs(u), 1.0))
    d = np.where(np.isfinite(d), d, np.inf)
    return d.min(axis=1)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------------------------------


def _case(points, covs, intensities, res, path, **extra):
    points = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    covs = np.ascontiguousarray(covs, dtype=np.float32).reshape(-1, 9)
    assert len(points) == len(covs)
    if intensities is not None:
        intensities = np.ascontiguousarray(intensities, dtype=np.float32).reshape(-1)
        assert len(intensities) == len(points)
    return dict(points=points, covs=covs, intensities=intensities, res=float(res), path=path, **extra)


def general_covs(rng, n):
    """f32 3x3, positive diagonal, NOT symmetric (the build takes the symmetric part)"""
    a = rng.normal(size=(n, 3, 3)) * 0.05
    c = a @ a.transpose(0, 2, 1) + np.eye(3) * 1e-3 + rng.normal(size=(n, 3, 3)) * 1e-4
    return c.transpose(0, 2, 1).reshape(n, 9).astype(np.float32)


def integer_covs(rng, n):
    return rng.integers(-3, 4, size=(n, 9)).astype(np.float32)


def case_exact_phases(reverse=False):
    """(a): every voxel population of POPULATIONS behind k = 0 .. 16 one-point voxels of its own workgroup.

    Leaf 0.5; voxels only at cz = 0, cy = 0 .. 3, so a block of 4 x 4 x 4 voxels holds exactly sixteen, numbered by (cy & 3) << 2 | (cx & 3), and the blocks lie
    along x: block g holds voxels 16 g .. 16 g + 15 = the sixteen voxels of workgroup g of segmented_stats_kernel.  Slot k of a block holds the large voxel, the
    other slots one point each: the large voxel starts k rows into the workgroup's 512-row batches, so its rows meet every batch boundary at lane phase -k mod 16.
    k = 16 is a block of sixteen one-point voxels in front of a block that starts with the large one.  x starts at block -100: half the cloud is at negative
    coordinates.  Points are multiples of 2^-6, covariance entries integers in [-3, 3], intensities integers in [0, 7]: every f64 sum is exact in any order.
    Returns the expected (block, bit) order of the voxels in `voxel_order` (coords) and the population of each in `voxel_counts`."""
    rng = np.random.default_rng(20240)
    pts, order, counts = [], [], []
    block = -100

    def voxel(bx, slot, n):
        cx, cy = 4 * bx + (slot & 3), slot >> 2
        f = rng.integers(0, 32, size=(n, 3)) / 64.0
        pts.append(np.array([cx, cy, 0]) * 0.5 + f)
        order.append((cx, cy, 0))
        counts.append(n)

    for pop in POPULATIONS:
        for k in range(STATS_GROUP + 1):
            if k == STATS_GROUP:
                for slot in range(STATS_GROUP):
                    voxel(block, slot, 1)
                block += 1
            for slot in range(STATS_GROUP):
                voxel(block, slot, pop if slot == k % STATS_GROUP else 1)
            block += 1
    points = np.concatenate(pts)
    n = len(points)
    covs, ints = integer_covs(rng, n), rng.integers(0, 8, size=n)
    if reverse:
        points, covs, ints = points[::-1], covs[::-1], ints[::-1]
    return _case(points, covs, ints, 0.5, 2, voxel_order=np.array(order, dtype=np.int64), voxel_counts=np.array(counts, dtype=np.int64))


def _neighbours32(v):
    v = np.float32(v)
    return [v, np.nextafter(v, np.float32(np.inf)), np.nextafter(v, np.float32(-np.inf))]


def case_faces(res):
    """(b): points on voxel faces (m * res rounded to f32), one f32 ulp either side, +0.0 and -0.0, on one axis and on all three; a candidate whose
    p * (1 / res) lies within 2 ulp of an integer without being one is left out (the case is about the floor, not about the reciprocal's rounding)"""
    vals = [np.float32(0.0), np.float32(-0.0)]
    for m in (-1000, -3, -2, -1, 1, 2, 3, 1000):
        vals += _neighbours32(np.float32(m * res))
    vals += _neighbours32(np.float32(0.0))[1:]
    vals = np.array(vals, dtype=np.float32)
    mids = np.array([(m + 0.37) * res for m in (-2, 0, 5)], dtype=np.float32)
    pts = []
    for v in vals:
        pts.append([v, v, v])
        for a in range(3):
            for b in mids:
                p = [b, b, b]
                p[a] = v
                pts.append(p)
    pts = np.array(pts, dtype=np.float32)
    m = face_margin_ulps(pts, res)
    pts = pts[(m == 0) | (m > 2)]
    rng = np.random.default_rng(7)
    return _case(pts, general_covs(rng, len(pts)), rng.uniform(0, 100, len(pts)), res, predicted_path(pts, res))


def far_patch():
    """(c): 4096 points of a 3 m cube, f64"""
    return np.random.default_rng(11).uniform(0.0, 3.0, size=(4096, 3))


def case_far(distance, res):
    rng = np.random.default_rng(12)
    pts = (far_patch() + float(distance)).astype(np.float32)  # shifted in f64, rounded once
    return _case(pts, general_covs(rng, len(pts)), rng.uniform(0, 255, len(pts)), res, predicted_path(pts, res))


def case_width(name):
    """(d): a box per sort width.  Leaf 0.5 (a block is 2 m) unless stated."""
    rng = np.random.default_rng(13)
    res = 0.5

    def cube(n, lo, hi):
        return rng.uniform(lo, hi, size=(n, 3))

    if name == "1 pass":  # one block
        pts, want = cube(700, 0.01, 1.99), 1
    elif name == "2 passes":  # 8^3 blocks
        pts, want = cube(6000, -8.0, 7.99), 2
    elif name == "3 passes":  # 40^3 blocks
        pts, want = cube(12000, -40.0, 39.99), 3
    elif name == "4 passes":  # 4096 x 4096 x 1 = 2^24 blocks exactly: a patch and a second one 8.19 km away along x and y
        a, b = cube(3000, 0.01, 1.99), cube(2000, 0.01, 1.99)
        b[:, :2] += 4095 * 2.0
        pts, want = np.concatenate([a, b]), 4
    elif name == "fallback":  # 4097 x 4097 x 1 blocks: one block further
        a, b = cube(3000, 0.01, 1.99), cube(2000, 0.01, 1.99)
        b[:, :2] += 4096 * 2.0
        pts, want = np.concatenate([a, b]), "hashed"
    elif name == "thin x":  # leaf 0.01 (a block is 0.04 m): about 2^20 blocks along x, one along y and z
        res = 0.01
        pts = cube(5000, 0.001, 0.039)
        pts[:, 0] = rng.uniform(0.0, 0.04 * (1 << 20), size=len(pts))
        want = 4
    elif name == "thin z":
        res = 0.01
        pts = cube(5000, 0.001, 0.039)
        pts[:, 2] = rng.uniform(-0.02 * (1 << 20), 0.02 * (1 << 20), size=len(pts))
        want = 4
    else:
        raise KeyError(name)
    return _case(pts, general_covs(rng, len(pts)), rng.uniform(0, 255, len(pts)), res, want)


WIDTH_CASES = ("1 pass", "2 passes", "3 passes", "4 passes", "fallback", "thin x", "thin z")


def bad_rows():
    """(e): rows that belong to no voxel at leaf 0.5"""
    nan, inf = np.nan, np.inf
    return np.array(
        [[nan, 1.0, 1.0], [nan, nan, nan], [1.0, inf, 1.0], [1.0, 1.0, -inf], [6.0e8, 1.0, 1.0], [1.0, 1.0, -5.0e8], [inf, -inf, nan], [1.0, -3.0e38, 1.0]],
        dtype=np.float32,
    )


BAD_AT = (0, 1, 2, 4094, 4095, 4096, 4097, -3, -2, -1)


def case_invalid(fallback):
    """(e): 8200 points of a 10 m cube with rows of bad_rows() at the start, at the end and either side of the 4096-point tile boundary; with `fallback` one valid
    point just inside the 1e9 limit forces the hashed fallback.  Returns the rows that stay in `keep`."""
    rng = np.random.default_rng(14)
    n = 8200
    pts = rng.uniform(-5.0, 5.0, size=(n, 3)).astype(np.float32)
    bad = bad_rows()
    keep = np.ones(n, bool)
    for j, at in enumerate(BAD_AT):
        pts[at] = bad[j % len(bad)]
        keep[at] = False
    if fallback:
        pts[2000] = [np.nextafter(np.float32(5.0e8), np.float32(0.0)), 0.25, -0.25]
    return _case(pts, general_covs(rng, n), rng.uniform(0, 255, n), 0.5, "hashed" if fallback else predicted_path(pts, 0.5), keep=keep)


def case_all_invalid():
    n = 5000
    pts = np.tile(bad_rows(), (n // len(bad_rows()) + 1, 1))[:n]
    rng = np.random.default_rng(15)
    return _case(pts, general_covs(rng, n), rng.uniform(0, 255, n), 0.5, None)


INTENSITY_VALUES = (-5.0, -0.0, 0.0, 1e-30, 3.0, 255.0, 3.0e38, np.inf, -np.inf, np.nan, -np.nan, -1e-30)


def case_intensities():
    """(f): 48 voxels of 1 .. 40 points; voxel j draws from a subset of INTENSITY_VALUES chosen by the bits of j, so that there are voxels with only negative
    values, only NaN, only -0.0, and every mixture"""
    rng = np.random.default_rng(16)
    vals = np.array(INTENSITY_VALUES, dtype=np.float32)
    pts, ints = [], []
    for j in range(48):
        n = int(rng.integers(1, 41))
        c = np.array([j % 7 - 3, j // 7 - 3, (j % 3) - 1])
        pts.append((c + rng.uniform(0.05, 0.95, size=(n, 3))) * 0.5)
        if j < len(vals):
            pool = vals[j : j + 1]
        else:
            pool = vals[rng.random(len(vals)) < 0.35]
            pool = pool if len(pool) else vals[:2]
        ints.append(rng.choice(pool, size=n))
    pts = np.concatenate(pts)
    return _case(pts, general_covs(rng, len(pts)), np.concatenate(ints), 0.5, predicted_path(pts.astype(np.float32), 0.5))


def case_reinsert(which):
    """(g): clouds A and B that share part of their voxels"""
    rng = np.random.default_rng(17)
    na, nb = (6000, 1500) if which == "A larger" else (1500, 6000)
    a = rng.uniform(-6.0, 2.0, size=(na, 3))
    b = rng.uniform(-2.0, 6.0, size=(nb, 3))
    ca = _case(a, general_covs(rng, na), rng.uniform(0, 255, na), 0.5, None)
    cb = _case(b, general_covs(rng, nb), rng.uniform(0, 255, nb), 0.5, None)
    return ca, cb


def case_file(res, far):
    """(h): 5000 points of a 12 m cube, at the origin or 20 km out"""
    rng = np.random.default_rng(18)
    pts = rng.uniform(-6.0, 6.0, size=(5000, 3)) + (np.array([20000.0, -20000.0, 300.0]) if far else 0.0)
    return _case(pts, general_covs(rng, len(pts)), rng.uniform(0, 255, len(pts)), res, None)

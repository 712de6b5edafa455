"""numpy f64 / math.fsum restatement of the INCREMENTAL Gaussian voxel map with LRU eviction, and the frame sequences its tests use.  A helper, not a test; it reads
nothing outside the repository and does not use oracle/.  (Reference lines relative to the reference's source tree.)

The semantics are GaussianVoxelMapCPU's, an IncrementalVoxelMap<GaussianVoxel> (src/gtsam_points/types/gaussian_voxelmap_cpu.cpp:23-47,
include/gtsam_points/ann/impl/incremental_voxelmap_impl.hpp:31-68).  State: lru_counter (from 0), lru_horizon, lru_clear_cycle (10 / 10), and per voxel the terms of
its sums, its max intensity and its stamp.  One insert(frame):
  1. every valid point (tests/voxelmap_ref.py: all three |p * (1 / res)| < 1e9) goes to voxel floor(float64(p) * (1 / res)), created empty when absent:
     count += 1, the point and the symmetric part of its covariance join the voxel's terms, intensity = max(intensity, I) by `cur < x ? x : cur` from 0.0 when the
     frame has intensities, stamp = lru_counter.  A voxel the frame does not touch keeps everything, stamp included.
  2. ++lru_counter; if lru_counter % lru_clear_cycle == 0 every voxel with stamp + lru_horizon < lru_counter is removed (with lru_horizon = 0 the ones just touched
     too); a removed voxel that reappears starts from zero.
  3. mean = sum(p) / count, cov = sum(sym(C)) / count -- here by math.fsum over ALL the terms the voxel holds, so the restatement carries one rounding per entry
     whatever the number of inserts (the reference multiplies its finalized mean back by the count at the next insert and so rounds per insert).
An empty frame runs steps 2 and 3."""
import math

import numpy as np

import voxelmap_ref as vr


class Voxel:
    __slots__ = ("points", "covs6", "intensity", "stamp")

    def __init__(self):
        self.points, self.covs6, self.intensity, self.stamp = [], [], np.float32(0.0), 0


class Snapshot:
    """the finalized map: coords int64 (V,3) in lexicographic order, index {coord: row}, counts, means / covs f64, max_abs_cov, intensities f32, stamps int64"""

    def __init__(self, res, voxels):
        self.res = float(res)
        keys = sorted(voxels)
        V = len(keys)
        self.coords = np.array(keys, dtype=np.int64).reshape(V, 3)
        self.index = {k: i for i, k in enumerate(keys)}
        self.counts = np.zeros(V, dtype=np.int64)
        self.means = np.zeros((V, 3))
        self.max_abs_cov = np.zeros(V)
        self.intensities = np.zeros(V, dtype=np.float32)
        self.stamps = np.zeros(V, dtype=np.int64)
        c6 = np.zeros((V, 6))
        for i, k in enumerate(keys):
            v = voxels[k]
            p, c = np.array(v.points), np.array(v.covs6)
            n = float(len(p))
            self.counts[i] = len(p)
            self.means[i] = [math.fsum(p[:, a].tolist()) / n for a in range(3)]
            c6[i] = [math.fsum(c[:, a].tolist()) / n for a in range(6)]
            self.max_abs_cov[i] = np.abs(c).max()
            self.intensities[i] = v.intensity
            self.stamps[i] = v.stamp
        self.covs = vr._full(c6) if V else np.zeros((0, 3, 3))

    @property
    def num_voxels(self):
        return len(self.coords)


class IncrementalMap:
    def __init__(self, res, lru_horizon=10, lru_clear_cycle=10):
        self.res = float(res)
        self.lru_horizon, self.lru_clear_cycle, self.lru_counter = int(lru_horizon), int(lru_clear_cycle), 0
        self.voxels = {}
        self.evicted = []  # the coordinates the last insert removed

    def insert(self, points, covs9, intensities=None):
        points = np.asarray(points, dtype=np.float32).reshape(-1, 3)
        p = points.astype(np.float64)
        s6 = vr.sym6(np.asarray(covs9, dtype=np.float32).reshape(-1, 9))
        ok = vr.valid_mask(points, self.res) if len(points) else np.zeros(0, bool)
        coords = vr.voxel_coords(points, self.res) if len(points) else np.zeros((0, 3), np.int64)
        it = None if intensities is None else np.asarray(intensities, dtype=np.float32).reshape(-1)
        for i in np.flatnonzero(ok).tolist():
            key = tuple(coords[i].tolist())
            v = self.voxels.get(key)
            if v is None:
                v = self.voxels[key] = Voxel()
            v.points.append(p[i])
            v.covs6.append(s6[i])
            if it is not None and v.intensity < it[i]:
                v.intensity = np.float32(it[i])
            v.stamp = self.lru_counter
        self.lru_counter += 1
        self.evicted = []
        if self.lru_counter % self.lru_clear_cycle == 0:
            self.evicted = [k for k, v in self.voxels.items() if v.stamp + self.lru_horizon < self.lru_counter]
            for k in self.evicted:
                del self.voxels[k]

    @property
    def num_voxels(self):
        return len(self.voxels)

    def snapshot(self):
        return Snapshot(self.res, self.voxels)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------------------------------


def symmetric_covs(rng, n):
    """f32 3x3, symmetric to the last bit (the reference's CPU map sums the matrix as it is)"""
    a = (rng.normal(size=(n, 3, 3)) * 0.05).astype(np.float32)
    c = np.einsum("nij,nkj->nik", a, a) + np.eye(3, dtype=np.float32) * np.float32(1e-3)
    c = (c + c.transpose(0, 2, 1)) * np.float32(0.5)
    assert (c == c.transpose(0, 2, 1)).all()
    return np.ascontiguousarray(c.reshape(n, 9), dtype=np.float32)


SLIDING_RES = 0.5
SLIDING_FRAMES = 21


def sliding_frames(points_per_frame=160, seed=23):
    """21 frames of a 2 m cube sliding 1 m per frame along x from x = -5 (voxel coordinates cross zero on every axis); the LAST frame is back where the first one was.
    At lru_horizon = lru_clear_cycle = 10 the 20th insert removes what frames 0 .. 9 alone touched (x below 5 m), so the map's box, which grew for nineteen inserts,
    shrinks, and the 21st insert revisits removed coordinates.  Returns [(points f32 (n,3), covs f32 (n,9) symmetric, intensities f32 (n,))]."""
    rng = np.random.default_rng(seed)
    frames = []
    for k in range(SLIDING_FRAMES):
        x0 = -5.0 + (k if k < SLIDING_FRAMES - 1 else 0)
        n = points_per_frame + 7 * k
        pts = rng.uniform([x0, -1.0, -1.0], [x0 + 2.0, 1.0, 1.0], size=(n, 3)).astype(np.float32)
        frames.append((pts, symmetric_covs(rng, n), rng.uniform(0, 255, n).astype(np.float32)))
    return frames


PHASE_POPULATIONS = (1, 15, 16, 17, 511, 512, 513)


def phase_frames(seed=29):
    """two frames at leaf 0.5: the first puts 3 points into each of eight voxels along x (cy = cz = 0, cx = -3 .. 4); the second delivers PHASE_POPULATIONS points
    to the first seven -- the lane phases of the sixteen-lane sum and either side of its 512-row batch -- and nothing to the eighth.  The seven voxels are
    consecutive cells of the second frame, so the large ones start at different rows of the workgroup's batches."""
    rng = np.random.default_rng(seed)

    def cloud(counts):
        pts = np.concatenate([(np.array([cx, 0, 0]) + rng.uniform(0.05, 0.95, size=(n, 3))) * 0.5 for cx, n in counts])
        n = len(pts)
        perm = rng.permutation(n)
        return pts[perm].astype(np.float32), vr.general_covs(rng, n), rng.uniform(0, 255, n).astype(np.float32)

    first = cloud([(cx, 3) for cx in range(-3, 5)])
    second = cloud([(cx, n) for cx, n in zip(range(-3, 4), PHASE_POPULATIONS)])
    return first, second

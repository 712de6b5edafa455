"""f64 numpy restatement of the reference's global registration, for tests/test_ransac_ref_cpu.py and the GPU tests of the occupancy set, the feature matching and RANSAC.

Written from the reference sources (paths relative to the reference tree):
  occupancy set     include/gtsam_points/ann/fast_occupancy_grid.hpp:13-113, ann/impl/fast_occupancy_grid_impl.hpp:14-74, src/gtsam_points/ann/fast_occupancy_grid.cpp:12-93
                    cell = fast_floor((pose * p) * inv_resolution) + 2^20 (impl:18); blocks of 8^3 cells keyed by three 21-bit block coordinates (cpp:23-27).  Here: a
                    Python set of integers key * 512 + bit.  The reference's table gives up after 10 probes and rehashes: an implementation detail, the SET is this one.
  sampling          include/gtsam_points/registration/impl/ransac_impl.hpp:39-48: distinct indices, a duplicate is drawn again.  The generator is the device's
                    (include/gtsam_points_hip.h, gp_ransac_estimate_pose), restated in Python integers: mt19937 parity is neither possible nor wanted.
  invalid feature   :57  source_f.isZero(1e-3): every |f_j| <= 1e-3
  matching          :62  1-NN of the feature row among the target's rows (brute force here; squared distances summed serially in ascending j)
  polygon error     :73-88
  alignment         src/gtsam_points/registration/alignment.cpp:11-40 (3 points), :42-65 (2 points, 4 DoF), :67-139 (weighted N points), through numpy.linalg.svd
  taboo rule        ransac_impl.hpp:149-156; the angle of Eigen::AngleAxisd(R) as atan2(|2 sin|, 2 cos) from R's skew part and trace
  selection         :158-169 made deterministic: iterations in chunks, in order; behind a chunk in which a scored hypothesis has inliers > size(source) * rate (:163)
                    every later iteration is SKIPPED; the result is the scored hypothesis with the most inliers, ties to the lowest iteration; inlier_rate over
                    size(target) (:190)

pose * p is evaluated as ((r0 x + r1 y) + r2 z) + t in plain f64 (Eigen's coefficient order; no fused multiply-add), which the device reproduces to the bit.
"""
import functools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SCORED, SAMPLE_FAILED, INVALID_FEATURE, POLY_REJECTED, TABOO, SKIPPED = 0, 1, 2, 3, 4, 5
OFFSET = 1 << 20
MASK21 = (1 << 21) - 1
M64 = (1 << 64) - 1
MAX_REDRAWS = 64


def scan(name="000000.bin"):
    return np.fromfile(os.path.join(GOLDEN, "kitti_00", name), dtype=np.float32).reshape(-1, 3)


# ---- occupancy -------------------------------------------------------------------------------------------------------------------------------------------------------
def transform(points32, pose):
    """(N, 3) f64: pose * p, each row ((r0 x + r1 y) + r2 z) + t"""
    p = np.asarray(points32, np.float32).reshape(-1, 3).astype(np.float64)
    T = np.asarray(pose, np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], axis=1)


def cell_keys(points32, pose, resolution):
    """(int64 keys [N] = block key * 512 + bit, valid mask): the cell of every point; a point with a non-finite transformed coordinate has none"""
    q = transform(points32, pose)
    ok = np.isfinite(q).all(axis=1)
    with np.errstate(invalid="ignore"):
        g = np.floor(np.where(ok[:, None], q, 0.0) * (1.0 / resolution)).astype(np.int64) + OFFSET
    b = (g >> 3) & MASK21
    key = b[:, 0] | (b[:, 1] << 21) | (b[:, 2] << 42)  # < 2^63
    bit = (g[:, 0] & 7) | ((g[:, 1] & 7) << 3) | ((g[:, 2] & 7) << 6)
    return [int(k) * 512 + int(c) for k, c in zip(key.tolist(), bit.tolist())], ok


def band_count(points32, pose, resolution, tol=1e-10):
    """points with a transformed coordinate / resolution within tol of an integer: the only points about which two roundings of the transform could disagree"""
    v = transform(points32, pose) * (1.0 / resolution)
    return int((np.abs(v - np.round(v)) < tol).any(axis=1).sum())


def occ_hash(key):
    """gp_occupancy.hpp occ_hash: key * 0x9E3779B97F4A7C15 mod 2^64, xor with itself shifted right by 32, the low 32 bits"""
    h = (int(key) * 0x9E3779B97F4A7C15) & M64
    return (h ^ (h >> 32)) & 0xFFFFFFFF


def home_slot(key, slots):
    """the slot a block key's probe chain starts at in a table of `slots` (a power of two)"""
    return occ_hash(key) & (slots - 1)


def block_key(bx, by, bz):
    """the key of the block with (unmasked) block coordinates cell >> 3, the cell counted from -2^20"""
    return (int(bx) & MASK21) | ((int(by) & MASK21) << 21) | ((int(bz) & MASK21) << 42)


def probe_table(block_keys, slots):
    """linear probing of the keys, in this order, into `slots` slots: the list of slots' keys (None = free).  The device's table holds the same keys whatever the
    order (the slots differ with the order of the claims, the SET does not); this is for the conditions on planted collisions only."""
    table = [None] * slots
    for k in block_keys:
        s = home_slot(k, slots)
        for _ in range(slots):
            if table[s] is None or table[s] == k:
                table[s] = k
                break
            s = (s + 1) & (slots - 1)
        else:
            raise AssertionError("table full")
    return table


class OccupancySet:
    def __init__(self, resolution):
        self.resolution = float(resolution)
        self.cells = set()

    def insert(self, points32, pose=np.eye(4)):
        keys, ok = cell_keys(points32, pose, self.resolution)
        self.cells.update(k for k, v in zip(keys, ok.tolist()) if v)
        return self

    def get_overlaps(self, points32, pose=np.eye(4)):
        keys, ok = cell_keys(points32, pose, self.resolution)
        return np.array([v and (k in self.cells) for k, v in zip(keys, ok.tolist())], np.uint8).reshape(-1)

    def calc_overlap(self, points32, pose=np.eye(4)):
        return int(self.get_overlaps(points32, pose).sum())

    def num_occupied_cells(self):
        return len(self.cells)

    def num_blocks(self):
        return len({k >> 9 for k in self.cells})


# ---- feature matching ------------------------------------------------------------------------------------------------------------------------------------------------
def match_features(target_features, source_features, rows=None):
    """(index int64 [nq], squared distance f64 [nq], number of targets at exactly the minimum [nq]); the sum over j serial in ascending j.
    Among targets at exactly the minimum the LOWEST index is returned (np.argmin returns the first occurrence): the device's rule, which the determinism of RANSAC
    rests on.  A target whose sum is NaN or +inf is never `<` the best so far and is never returned (a NaN feature on either side makes the sum NaN); a query that no
    target compares below +inf with -- a NaN query row, every target row NaN or infinite, a row index outside the source rows -- gives (-1, +inf, 0)."""
    T = np.asarray(target_features, np.float32).astype(np.float64)
    S = np.asarray(source_features, np.float32).astype(np.float64)
    rows = np.arange(len(S)) if rows is None else np.asarray(rows, np.int64).reshape(-1)
    idx, sq, ties = np.zeros(len(rows), np.int64), np.zeros(len(rows)), np.zeros(len(rows), np.int64)
    for i, r in enumerate(rows.tolist()):
        acc = np.full(len(T), np.nan)
        if 0 <= r < len(S):
            acc = np.zeros(len(T))
            with np.errstate(invalid="ignore", over="ignore"):
                for j in range(T.shape[1]):
                    d = S[r, j] - T[:, j]
                    acc = acc + d * d
        below = acc < np.inf  # (False for NaN)
        if not below.any():
            idx[i], sq[i], ties[i] = -1, np.inf, 0
            continue
        idx[i] = int(np.argmin(np.where(below, acc, np.inf)))
        sq[i] = acc[idx[i]]
        ties[i] = int((acc == sq[i]).sum())
    return idx, sq, ties


# ---- the generator -----------------------------------------------------------------------------------------------------------------------------------------------------
def mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def sample_index(seed, iteration, draw, n):
    G = 0x9E3779B97F4A7C15
    r = mix((mix((seed + G * (iteration + 1)) & M64) + G * (draw + 1)) & M64)
    return ((r >> 32) * n) >> 32


def draw_samples(seed, iteration, n, samples):
    """the iteration's distinct indices, or None after more than MAX_REDRAWS redraws"""
    idx, draw, redraws = [], 0, 0
    while len(idx) < samples:
        c = sample_index(seed, iteration, draw, n)
        draw += 1
        if c in idx:
            redraws += 1
            if redraws > MAX_REDRAWS:
                return None
            continue
        idx.append(c)
    return idx


# ---- per-hypothesis rules ---------------------------------------------------------------------------------------------------------------------------------------------
def poly_error(t, s):
    """t, s: (k, 3) f64 points of the sample in the target and the source; the largest relative difference of corresponding edge lengths"""
    k = len(t)
    worst = 0.0
    for j in range(k):
        n = (j + 1) % k
        a, b = t[j] - t[n], s[j] - s[n]
        dt = np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
        ds = np.sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2])
        worst = max(worst, abs(dt - ds) / max(max(dt, ds), 1e-6))
    return worst


def cross_covariance(t, s, w=None):
    """(H 3x3, mean_t, mean_s) as alignment.cpp forms them: sample means by ((a + b) + c) / k, weighted ones serially"""
    t, s = np.asarray(t, np.float64), np.asarray(s, np.float64)
    if w is None:
        mt, ms = t[0].copy(), s[0].copy()
        for j in range(1, len(t)):
            mt, ms = mt + t[j], ms + s[j]
        mt, ms = mt / float(len(t)), ms / float(len(s))
        w = np.ones(len(t))
    else:
        w = np.asarray(w, np.float64)
        sw, mt, ms = 0.0, np.zeros(3), np.zeros(3)
        for j in range(len(t)):
            sw, mt, ms = sw + w[j], mt + w[j] * t[j], ms + w[j] * s[j]
        mt, ms = mt / sw, ms / sw
    H = np.zeros((3, 3))
    for j in range(len(t)):
        H = H + np.outer(w[j] * (t[j] - mt), s[j] - ms)
    return H, mt, ms


def pose_from(H, mt, ms, dof):
    T = np.eye(4)
    if dof == 6:
        U, _, Vt = np.linalg.svd(H)
        S = np.ones(3)
        if np.linalg.det(U) * np.linalg.det(Vt) < 0.0:
            S[2] = -1.0
        T[:3, :3] = U @ np.diag(S) @ Vt
    else:
        U, _, Vt = np.linalg.svd(H[:2, :2])
        S = np.ones(2)
        if np.linalg.det(U) * np.linalg.det(Vt) < 0.0:
            S[1] = -1.0
        T[:2, :2] = U @ np.diag(S) @ Vt
    T[:3, 3] = mt - T[:3, :3] @ ms
    return T


def align_points_se3(t, s, w=None):
    return pose_from(*cross_covariance(t, s, w), 6)


def align_points_4dof(t, s, w=None):
    return pose_from(*cross_covariance(t, s, w), 4)


def rotation_bound(H, dof):
    """(conditioned, bound): the Frobenius bound on the rotation between two correctly working methods, 1e-12 x the sensitivity of the rotation to rounding in H.
    dof 6: sigma1 / sigma2 of the 3x3 H (a sample's H has rank 2: the third pair follows from the first two), conditioned when sigma2 / sigma1 >= 1e-6.
    dof 4: the rotation is atan2(h10 - h01, h00 + h11): sensitivity |H2|_F / hypot(.,.), conditioned when that ratio's inverse is >= 1e-6."""
    if dof == 6:
        sv = np.linalg.svd(H, compute_uv=False)
        if sv[0] == 0.0 or sv[1] / sv[0] < 1e-6:
            return False, np.inf
        return True, 1e-12 * sv[0] / sv[1]
    n = np.hypot(H[0, 0] + H[1, 1], H[1, 0] - H[0, 1])
    f = np.linalg.norm(H[:2, :2])
    if f == 0.0 or n / f < 1e-6:
        return False, np.inf
    return True, 1e-12 * f / n


def pose_inverse(T):
    Ti = np.eye(4)
    Ti[:3, :3] = T[:3, :3].T
    Ti[:3, 3] = -(Ti[:3, :3] @ T[:3, 3])
    return Ti


def taboo_delta(T, taboo):
    """(angle, translation norm) of taboo^-1 * T"""
    d = pose_inverse(np.asarray(taboo, np.float64)) @ T
    R = d[:3, :3]
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return float(np.arctan2(np.linalg.norm(v), np.trace(R) - 1.0)), float(np.linalg.norm(d[:3, 3]))


def is_taboo(T, taboo_list, thresh_rot, thresh_trans):
    return any(a < thresh_rot and t < thresh_trans for a, t in (taboo_delta(T, b) for b in taboo_list))


# ---- the iterations ----------------------------------------------------------------------------------------------------------------------------------------------------
def hypotheses(target32, source32, target_features, source_features, iterations, dof=6, seed=5489, poly_error_thresh=0.5, taboo_list=(), taboo_thresh_rot=0.5 * np.pi / 180.0,
               taboo_thresh_trans=0.25, sample_indices=None):
    """every iteration up to the score, nothing skipped: dict of status [H], source_indices / target_indices [H][3] (-1), poses [H][4][4] (zeros before the alignment), H
    matrices, poly errors, taboo deltas (for the conditions on the inputs)"""
    tp = np.asarray(target32, np.float32).astype(np.float64)
    sp = np.asarray(source32, np.float32).astype(np.float64)
    sf = np.asarray(source_features, np.float32)
    samples = 3 if dof == 6 else 2
    out = {"status": np.zeros(iterations, np.int32), "source_indices": np.full((iterations, 3), -1, np.int32), "target_indices": np.full((iterations, 3), -1, np.int32),
           "poses": np.zeros((iterations, 4, 4)), "H": np.zeros((iterations, 3, 3)), "poly": np.full(iterations, np.nan), "taboo": [[] for _ in range(iterations)],
           "match_ties": np.zeros(iterations, np.int64)}
    alive = []
    for it in range(iterations):
        idx = draw_samples(seed, it, len(sp), samples) if sample_indices is None else [int(v) for v in np.asarray(sample_indices)[it][:samples]]
        if idx is None:
            out["status"][it] = SAMPLE_FAILED
            continue
        out["source_indices"][it, :samples] = idx
        if any((np.abs(sf[i].astype(np.float64)) <= 1e-3).all() for i in idx):
            out["status"][it] = INVALID_FEATURE
            continue
        alive.append(it)
    rows = [int(i) for it in alive for i in out["source_indices"][it, :samples]]
    m_idx, _, m_ties = match_features(target_features, source_features, rows)
    for k, it in enumerate(alive):
        si = out["source_indices"][it, :samples]
        ti = np.maximum(m_idx[samples * k : samples * k + samples], 0)  # a sampled row without a match takes target 0 (ransac_impl.hpp:64)
        out["target_indices"][it, :samples] = ti
        out["match_ties"][it] = int(m_ties[samples * k : samples * k + samples].max())
        t, s = tp[ti], sp[si]
        out["poly"][it] = poly_error(t, s)
        if out["poly"][it] > poly_error_thresh:
            out["status"][it] = POLY_REJECTED
            continue
        H, mt, ms = cross_covariance(t, s)
        T = pose_from(H, mt, ms, dof)
        out["H"][it], out["poses"][it] = H, T
        out["taboo"][it] = [taboo_delta(T, b) for b in taboo_list]
        if any(a < taboo_thresh_rot and d < taboo_thresh_trans for a, d in out["taboo"][it]):
            out["status"][it] = TABOO
    return out


def select(status, inliers, chunk_iterations, num_source, early_stop_inlier_rate):
    """the chunked selection on per-iteration statuses (nothing skipped yet) and inlier counts: (final status, best iteration or -1, best inliers)"""
    status = np.array(status, np.int32)
    best, best_it, stop = -1, -1, False
    for begin in range(0, len(status), chunk_iterations):
        sl = slice(begin, min(begin + chunk_iterations, len(status)))
        if stop:
            status[sl] = SKIPPED
            continue
        for it in range(sl.start, sl.stop):
            if status[it] != SCORED:
                continue
            if inliers[it] > best:
                best, best_it = int(inliers[it]), it
            if inliers[it] > num_source * early_stop_inlier_rate:
                stop = True
    return status, best_it, max(best, 0)


def estimate_pose_ransac(target32, source32, target_features, source_features, iterations, chunk_iterations=1024, early_stop_inlier_rate=0.8, inlier_voxel_resolution=1.0, **kw):
    """the whole restatement on its own poses: (inlier_rate, T_target_source, final status, inliers, hypotheses dict)"""
    hyp = hypotheses(target32, source32, target_features, source_features, iterations, **kw)
    grid = OccupancySet(inlier_voxel_resolution).insert(target32)
    inl = np.full(iterations, -1, np.int64)
    for it in np.flatnonzero(hyp["status"] == SCORED):
        inl[it] = grid.calc_overlap(source32, hyp["poses"][it])
    status, best_it, best = select(hyp["status"], inl, chunk_iterations, len(source32), early_stop_inlier_rate)
    T = hyp["poses"][best_it] if best_it >= 0 else np.eye(4)
    return best / float(len(target32)), T, status, np.where(status == SCORED, inl, -1), hyp


# ---- the inputs of tests/test_ransac_gpu.py (tests/test_ransac_ref_cpu.py holds them to the conditions the exact comparisons rest on) -----------------------------------
def rot(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


CASE_ITERATIONS = 256
CASE_DIM = 33
CASE_ZERO_ROWS = tuple(range(7, 2048, 50))  # 41 rows: 256 iterations x 3 draws from 2048 rows hit about 15 of them


@functools.lru_cache(maxsize=None)
def make_case(dof, seed=1):
    """target: a golden scan cut to at most 4096 points (every 31st); source: 2048 of them moved by the inverse of a known T_target_source and rounded to f32; D = 33 descriptors, the source
    row = the target row + noise for ~60 % of the points, random otherwise, 41 all-zero rows"""
    rng = np.random.default_rng(seed + 10 * dof)
    full = scan()
    target = np.ascontiguousarray(full[:: len(full) // 4096 + 1][:4096])
    pick = np.sort(rng.choice(len(target), 2048, replace=False))
    T = np.eye(4)
    T[:3, :3] = rot([0.2, -0.1, 1.0], 0.6) if dof == 6 else rot([0, 0, 1], 0.6)
    T[:3, 3] = [3.0, -2.0, 0.5]
    Ti = pose_inverse(T)
    source = (target[pick].astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)
    tf = rng.normal(size=(len(target), CASE_DIM)).astype(np.float32)
    sf = rng.normal(size=(len(source), CASE_DIM)).astype(np.float32)
    good = rng.random(len(source)) < 0.6
    sf[good] = tf[pick[good]] + (0.01 * rng.normal(size=(int(good.sum()), CASE_DIM))).astype(np.float32)
    sf[list(CASE_ZERO_ROWS)] = 0.0
    return {"target": target, "source": source, "target_features": tf, "source_features": sf, "T_true": T, "pick": pick, "dof": dof}


# ---- the small inputs of tests/test_ransac_edges_gpu.py (tests/test_ransac_edges_ref_cpu.py holds them to their conditions) ------------------------------------------------
SMALL_DIM = 8
SMALL_ZERO_ROWS = (3, 40, 77, 114, 151, 188)
SMALL_ROW_1E3, SMALL_ROW_2M10, SMALL_ROW_NAN = 10, 20, 30  # float32(1e-3) in one entry (valid: it widens to just above 1e-3); every entry 2^-10 (invalid); every entry NaN


@functools.lru_cache(maxsize=None)
def make_small_case(dof, far=0.0, seed=2):
    """make_case in small: the target a golden scan cut to at most 512 points, moved by (far, far, 0) and rounded to f32; the source 256 of them moved by the inverse of a
    known pose; D = 8 descriptors, ~70 % true matches, six all-zero rows and the three special rows above"""
    rng = np.random.default_rng(seed + 10 * dof)
    full = scan()
    target = (full[:: len(full) // 512 + 1][:512].astype(np.float64) + [far, far, 0.0]).astype(np.float32)
    pick = np.sort(rng.choice(len(target), 256, replace=False))
    T = np.eye(4)
    T[:3, :3] = rot([0.2, -0.1, 1.0], 0.6) if dof == 6 else rot([0, 0, 1], 0.6)
    T[:3, 3] = [3.0, -2.0, 0.5]
    Ti = pose_inverse(T)
    source = (target[pick].astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)
    tf = rng.normal(size=(len(target), SMALL_DIM)).astype(np.float32)
    sf = rng.normal(size=(len(source), SMALL_DIM)).astype(np.float32)
    good = rng.random(len(source)) < 0.7
    sf[good] = tf[pick[good]] + (0.01 * rng.normal(size=(int(good.sum()), SMALL_DIM))).astype(np.float32)
    sf[list(SMALL_ZERO_ROWS)] = 0.0
    sf[SMALL_ROW_1E3] = 0.0
    sf[SMALL_ROW_1E3, 5] = np.float32(1e-3)
    sf[SMALL_ROW_2M10] = np.float32(2.0 ** -10)
    sf[SMALL_ROW_NAN] = np.nan
    return {"target": np.ascontiguousarray(target), "source": np.ascontiguousarray(source), "target_features": tf, "source_features": sf, "T_true": T, "pick": pick, "dof": dof,
            "good": good}


def alignment_residual(T, s, t):
    """sum |T s - t|^2 over the sample's points (rows of s and t), in f64"""
    s, t = np.asarray(s, np.float64), np.asarray(t, np.float64)
    d = s @ T[:3, :3].T + T[:3, 3] - t
    return float((d * d).sum())

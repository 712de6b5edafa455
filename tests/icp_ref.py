"""IntegratedICPFactor_ (factors/impl/integrated_icp_factor_impl.hpp) restated in numpy, f64 on the f32 inputs.  A helper, not a test.

  update_correspondences(delta)   :128-157  the tolerance rule, then a brute-force 1-NN of T p among the target points (no search structure: every squared
                                            distance is formed, (q - t)^2 summed coordinate by coordinate in f64); a correspondence needs sq_dist < max (the
                                            strict '<' of the device library's search, KnnResult::push; the reference's own kd-tree prunes at the same bound)
  evaluate(delta)                 :180-248  q = T p, d = mu_B - q, r = n_B o d (element-wise) or r = d; error = sum r^T r (no 1/2);
                                            J_t = diag(n_B) [-[q]x, I], J_s = diag(n_B) [R [p]x, -R] with R = delta's 3x3 block AS GIVEN; H = sum J^T J, b = sum J^T r
  linearize(delta)                          update_correspondences + evaluate (IntegratedMatchingCostFactor::linearize)
  error(delta)                              evaluate on the stored correspondences; a search at delta only when none are stored (:188-190)
  margins(delta)                            per source point, how far its decision is from flipping: the relative gap between the nearest and the second-nearest
                                            squared distance, and the relative gap between the nearest squared distance and the cut-off

The 1-NN results are cached per (target, transformed queries): tests that share a pose share the search.
"""
import hashlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

_CACHE = {}


def hat(v):
    """[v]x for rows of v: (N,3) -> (N,3,3)"""
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    out = np.zeros((len(v), 3, 3))
    out[:, 0, 1], out[:, 0, 2] = -v[:, 2], v[:, 1]
    out[:, 1, 0], out[:, 1, 2] = v[:, 2], -v[:, 0]
    out[:, 2, 0], out[:, 2, 1] = -v[:, 1], v[:, 0]
    return out


def transform(delta, p):
    """T p with the 3x3 block as given (no re-orthonormalisation)"""
    delta = np.asarray(delta, dtype=np.float64)
    return p @ delta[:3, :3].T + delta[:3, 3]


def nearest_two(target, q, chunk=512):
    """brute force in f64: (index of the nearest target point, its squared distance, the second-smallest squared distance or inf) per row of q"""
    key = (hashlib.blake2b(target.tobytes(), digest_size=16).digest(), hashlib.blake2b(np.ascontiguousarray(q).tobytes(), digest_size=16).digest())
    if key in _CACHE:
        return _CACHE[key]
    idx = np.full(len(q), -1, np.int64)
    d1 = np.full(len(q), np.inf)
    d2 = np.full(len(q), np.inf)

    def rows(a):
        qq = q[a : a + chunk]
        d = (qq[:, None, 0] - target[None, :, 0]) ** 2
        d += (qq[:, None, 1] - target[None, :, 1]) ** 2
        d += (qq[:, None, 2] - target[None, :, 2]) ** 2
        i = np.argmin(d, axis=1)
        r = np.arange(len(qq))
        idx[a : a + chunk] = i
        d1[a : a + chunk] = d[r, i]
        if len(target) > 1:
            d[r, i] = np.inf
            d2[a : a + chunk] = d.min(axis=1)

    if len(target):
        starts = range(0, len(q), chunk)
        if len(q) * len(target) > (1 << 24):  # (numpy releases the interpreter lock inside these array operations; the chunks write disjoint rows)
            with ThreadPoolExecutor(max_workers=8) as pool:
                list(pool.map(rows, starts))
        else:
            for a in starts:
                rows(a)
    _CACHE[key] = (idx, d1, d2)
    return _CACHE[key]


def pose_difference(delta, last):
    """(rotation angle, translation norm) of delta^-1 * last, delta^-1 the isometry inverse (:131-133).  The angle from the skew part (sin) and the trace (cos):
    Eigen::AngleAxisd(R).angle() of a rotation, in [0, pi]"""
    delta, last = np.asarray(delta, dtype=np.float64), np.asarray(last, dtype=np.float64)
    R = delta[:3, :3].T @ last[:3, :3]
    t = delta[:3, :3].T @ (last[:3, 3] - delta[:3, 3])
    s = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return float(np.arctan2(np.linalg.norm(s), 0.5 * (np.trace(R) - 1.0))), float(np.linalg.norm(t))


class ICPFactorRef:
    def __init__(self, target_points, source_points, target_normals=None, use_point_to_plane=False, max_correspondence_distance=1.0):
        self.target = np.asarray(target_points, dtype=np.float32).reshape(-1, 3).astype(np.float64)
        self.source = np.asarray(source_points, dtype=np.float32).reshape(-1, 3).astype(np.float64)
        self.use_point_to_plane = bool(use_point_to_plane)
        if self.use_point_to_plane and target_normals is None:
            raise ValueError("error: target frame doesn't have required attributes for icp")  # :37-40
        self.normals = None if target_normals is None else np.asarray(target_normals, dtype=np.float32).reshape(-1, 3).astype(np.float64)  # (what the device reads)
        self.max_sq = float(max_correspondence_distance) ** 2  # :30
        self.tol_rot = self.tol_trans = 0.0                    # :32-33
        self.correspondences = None
        self.last_correspondence_point = None
        self.searches = 0

    def set_correspondence_update_tolerance(self, angle, trans):
        self.tol_rot, self.tol_trans = float(angle), float(trans)

    def keeps_correspondences(self, delta):
        """:129-137"""
        if self.correspondences is None or not (self.tol_trans > 0.0 or self.tol_rot > 0.0):
            return False
        diff_rot, diff_trans = pose_difference(delta, self.last_correspondence_point)
        return diff_rot < self.tol_rot and diff_trans < self.tol_trans

    def update_correspondences(self, delta):
        if self.keeps_correspondences(delta):
            return
        self.last_correspondence_point = np.array(delta, dtype=np.float64)
        idx, d1, _ = nearest_two(self.target, transform(delta, self.source))
        self.correspondences = np.where(d1 < self.max_sq, idx, -1)  # :146-157
        self.searches += 1

    def margins(self, delta):
        """(tie gap, cut-off gap) per source point, both relative: (d_second - d_first) / d_second and |d_first - max| / max on squared distances"""
        _, d1, d2 = nearest_two(self.target, transform(delta, self.source))
        with np.errstate(invalid="ignore", divide="ignore"):
            tie = np.where(np.isfinite(d2), (d2 - d1) / np.maximum(d2, 1e-300), np.inf)
        return tie, np.abs(d1 - self.max_sq) / self.max_sq

    def evaluate(self, delta, derivatives=True):
        delta = np.asarray(delta, dtype=np.float64)
        if self.correspondences is None:
            self.update_correspondences(delta)  # :188-190
        sel = np.flatnonzero(self.correspondences >= 0)
        c = self.correspondences[sel]
        p = self.source[sel]
        q = transform(delta, p)
        r = self.target[c] - q
        n = self.normals[c] if self.use_point_to_plane else np.ones_like(r)
        r = n * r  # :210-213, element-wise
        out = dict(error=float((r * r).sum()), num_inliers=int(len(sel)))
        if not derivatives:
            return out
        R = delta[:3, :3]
        Jt = np.concatenate([-hat(q), np.broadcast_to(np.eye(3), (len(sel), 3, 3))], axis=2)  # :220-222
        Js = np.concatenate([R[None] @ hat(p), np.broadcast_to(-R, (len(sel), 3, 3))], axis=2)  # :224-226
        Jt, Js = n[:, :, None] * Jt, n[:, :, None] * Js  # :228-232
        out["H_target"] = np.einsum("nki,nkj->ij", Jt, Jt)
        out["H_source"] = np.einsum("nki,nkj->ij", Js, Js)
        out["H_target_source"] = np.einsum("nki,nkj->ij", Jt, Js)
        out["b_target"] = np.einsum("nki,nk->i", Jt, r)
        out["b_source"] = np.einsum("nki,nk->i", Js, r)
        return out

    def linearize(self, delta):
        self.update_correspondences(delta)
        return self.evaluate(delta)

    def error(self, delta):
        return self.evaluate(delta, derivatives=False)["error"]

    def residuals(self, delta):
        """(N_matched, 3) residual rows on the stored correspondences (for differencing)"""
        sel = np.flatnonzero(self.correspondences >= 0)
        c = self.correspondences[sel]
        r = self.target[c] - transform(delta, self.source[sel])
        return self.normals[c] * r if self.use_point_to_plane else r

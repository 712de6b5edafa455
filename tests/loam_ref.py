"""IntegratedPointToEdgeFactor_, IntegratedPointToPlaneFactor_ and IntegratedLOAMFactor_ (factors/impl/integrated_loam_factor_impl.hpp) restated in numpy, f64 on
the f32 inputs.  A helper, not a test.

  update_correspondences(delta)   :80-124 (plane, K = 3), :235-279 (edge, K = 2)  the tolerance rule, then a brute-force K-NN of T p among the target points (every
                                  squared distance formed coordinate by coordinate in f64); the K nearest in ascending order when all K lie within sq_dist < max
                                  (the strict '<' of the device library's search), otherwise no correspondence
  evaluate(delta)                 edge :300-365  r = (q - x_j) x (q - x_l) / |x_j - x_l| -- the reference's CROSS-PRODUCT form, not the M-form the kernel sums --,
                                                 J = J_e J_t / |x_j - x_l| with J_e = [x_j - x_l]x
                                  plane :127-194 n = normalize((x_j - x_l) x (x_j - x_m)), r = n o (x_j - q), J = diag(n) J_t
                                  error = sum r^T r, H = sum J^T J, b = sum J^T r; J_t = [-[q]x, I], J_s = [R [p]x, -R], R = delta's 3x3 block AS GIVEN
  LOAMFactorRef                   :444-529  both parts searched, then validate_correspondences when enabled (also when the tolerance kept them), the record the
                                  edge part's plus the plane part's
  linearize(delta) / error(delta) update_correspondences + evaluate / evaluate on the stored correspondences (a search at delta only when none are stored)
  margins(delta)                  per source point, how far each decision is from flipping (see PartRef.margins)

The K+1 nearest are cached per (target, transformed queries, K): tests that share a pose share the search.
"""
import hashlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from icp_ref import hat, pose_difference, transform

_CACHE = {}
THETA = 0.1 * np.pi / 180.0       # :505, :525 first bound
THETA_PLANE_2 = 0.1 * np.pi * 180.0  # :525 second bound AS WRITTEN (about 56.5 rad: always holds)
BLOCKS = ["H_target", "H_source", "H_target_source", "b_target", "b_source"]


def nearest_k(target, q, k, chunk=512):
    """brute force in f64: (indices (N, k) of the k nearest target points in ascending order of distance, -1 where the target has fewer; squared distances (N, k),
    inf there)"""
    key = (hashlib.blake2b(target.tobytes(), digest_size=16).digest(), hashlib.blake2b(np.ascontiguousarray(q).tobytes(), digest_size=16).digest(), k)
    if key in _CACHE:
        return _CACHE[key]
    idx = np.full((len(q), k), -1, np.int64)
    dist = np.full((len(q), k), np.inf)
    kk = min(k, len(target))

    def rows(a):
        qq = q[a : a + chunk]
        d = (qq[:, None, 0] - target[None, :, 0]) ** 2
        d += (qq[:, None, 1] - target[None, :, 1]) ** 2
        d += (qq[:, None, 2] - target[None, :, 2]) ** 2
        if kk < len(target):
            part = np.argpartition(d, kk - 1, axis=1)[:, :kk]
        else:
            part = np.broadcast_to(np.arange(len(target)), (len(qq), len(target)))
        dp = np.take_along_axis(d, part, axis=1)
        o = np.argsort(dp, axis=1, kind="stable")
        idx[a : a + chunk, :kk] = np.take_along_axis(part, o, axis=1)
        dist[a : a + chunk, :kk] = np.take_along_axis(dp, o, axis=1)

    if kk and len(q):
        starts = range(0, len(q), chunk)
        if len(q) * len(target) > (1 << 24):
            with ThreadPoolExecutor(max_workers=8) as pool:
                list(pool.map(rows, starts))
        else:
            for a in starts:
                rows(a)
    _CACHE[key] = (idx, dist)
    return _CACHE[key]


def theta(p):
    """the vertical angle of :501-502, :520-522"""
    return np.arctan2(p[..., 2], np.hypot(p[..., 0], p[..., 1]))


class PartRef:
    """one of the two single factors: K = 2 (edge) or K = 3 (plane)"""

    def __init__(self, K, target_points, source_points, max_correspondence_distance=1.0):
        assert K in (2, 3)
        self.K = K
        self.target = np.asarray(target_points, dtype=np.float32).reshape(-1, 3).astype(np.float64)
        self.source = np.asarray(source_points, dtype=np.float32).reshape(-1, 3).astype(np.float64)
        self.max_sq = float(max_correspondence_distance) ** 2  # :27, :205
        self.tol_rot = self.tol_trans = 0.0
        self.correspondences = None  # (N, K), a row of -1 where there is none
        self.last_correspondence_point = None
        self.searches = 0

    def set_correspondence_update_tolerance(self, angle, trans):
        self.tol_rot, self.tol_trans = float(angle), float(trans)

    def keeps_correspondences(self, delta):
        """:81-88, :236-243"""
        if self.correspondences is None or not (self.tol_trans > 0.0 or self.tol_rot > 0.0):
            return False
        diff_rot, diff_trans = pose_difference(delta, self.last_correspondence_point)
        return diff_rot < self.tol_rot and diff_trans < self.tol_trans

    def update_correspondences(self, delta):
        if self.keeps_correspondences(delta):
            return
        self.last_correspondence_point = np.array(delta, dtype=np.float64)
        idx, dist = nearest_k(self.target, transform(delta, self.source), self.K + 1)
        ok = dist[:, self.K - 1] < self.max_sq  # all K found within the cut-off (inf where the target has fewer)
        self.correspondences = np.where(ok[:, None], idx[:, : self.K], -1)
        self.searches += 1

    def validate(self):
        """this part's share of validate_correspondences (:492-528); returns how many it rejected"""
        sel = np.flatnonzero(self.correspondences[:, 0] >= 0)
        t = theta(self.target[self.correspondences[sel]])  # (n, K)
        reject = np.abs(t[:, 0] - t[:, 1]) < THETA
        if self.K == 3:
            reject &= np.abs(t[:, 0] - t[:, 2]) < THETA_PLANE_2
        self.correspondences[sel[reject]] = -1
        return int(reject.sum())

    def margins(self, delta, validation=False):
        """dict of per-source-point margins at `delta`: `tie` the smallest relative gap between consecutive squared distances up to the (K+1)-th, `cut` the relative
        gap of the K-th to the cut-off, and over the points that get a correspondence: `length` |x_j - x_l|, `sine` between x_j - x_l and x_j - x_m (plane), and with
        validation `theta` the distance of |theta_j - theta_l| from the threshold in radians"""
        idx, dist = nearest_k(self.target, transform(delta, self.source), self.K + 1)
        out = {}
        with np.errstate(invalid="ignore", divide="ignore"):
            gaps = np.where(np.isfinite(dist[:, 1:]), (dist[:, 1:] - dist[:, :-1]) / np.maximum(dist[:, 1:], 1e-300), np.inf)
            out["tie"] = gaps.min(axis=1) if len(dist) else np.zeros(0)
            dk = dist[:, self.K - 1]
            out["cut"] = np.where(np.isfinite(dk), np.abs(dk - self.max_sq) / self.max_sq, np.inf)
        sel = dk < self.max_sq
        x = self.target[idx[sel][:, : self.K]]
        a = x[:, 0] - x[:, 1]
        out["length"] = np.linalg.norm(a, axis=1)
        if self.K == 3:
            b = x[:, 0] - x[:, 2]
            out["sine"] = np.linalg.norm(np.cross(a, b), axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
        if validation:
            t = theta(x)
            out["theta"] = np.abs(np.abs(t[:, 0] - t[:, 1]) - THETA)
        return out

    def _rows(self, delta):
        """(sel, p, q, r (n,3), A (n,3,3)): the residual rows and the matrices with dr = A d(x_j - q)-side Jacobians J = A J_t"""
        sel = np.flatnonzero(self.correspondences[:, 0] >= 0)
        c = self.correspondences[sel]
        p = self.source[sel]
        q = transform(delta, p)
        xj, xl = self.target[c[:, 0]], self.target[c[:, 1]]
        with np.errstate(invalid="ignore", divide="ignore"):
            if self.K == 2:
                c_inv = 1.0 / np.linalg.norm(xj - xl, axis=1)  # :330
                r = np.cross(q - xj, q - xl) * c_inv[:, None]    # :331-335
                A = c_inv[:, None, None] * hat(xj - xl)          # :350-356
            else:
                n = np.cross(xj - xl, xj - self.target[c[:, 2]])  # :158
                n = n / np.linalg.norm(n, axis=1)[:, None]       # :159
                r = (xj - q) * n                                 # :161-162
                A = n[:, :, None] * np.eye(3)[None]              # :177-178
        return sel, p, q, r, A

    def residuals(self, delta):
        return self._rows(np.asarray(delta, dtype=np.float64))[3]

    def jacobians(self, delta):
        """(J_target, J_source), each (n, 3, 6), at `delta` on the stored correspondences"""
        delta = np.asarray(delta, dtype=np.float64)
        sel, p, q, r, A = self._rows(delta)
        R = delta[:3, :3]
        Jt = np.concatenate([-hat(q), np.broadcast_to(np.eye(3), (len(sel), 3, 3))], axis=2)
        Js = np.concatenate([R[None] @ hat(p), np.broadcast_to(-R, (len(sel), 3, 3))], axis=2)
        return A @ Jt, A @ Js

    def evaluate(self, delta, derivatives=True):
        delta = np.asarray(delta, dtype=np.float64)
        if self.correspondences is None:
            self.update_correspondences(delta)
        sel, p, q, r, A = self._rows(delta)
        with np.errstate(invalid="ignore", over="ignore"):
            out = dict(error=float((r * r).sum()), num_inliers=int(len(sel)))
            if not derivatives:
                return out
            Jt, Js = self.jacobians(delta)
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

    @property
    def parts(self):
        return [self]


def EdgeFactorRef(target, source, max_correspondence_distance=1.0):
    return PartRef(2, target, source, max_correspondence_distance)


def PlaneFactorRef(target, source, max_correspondence_distance=1.0):
    return PartRef(3, target, source, max_correspondence_distance)


class LOAMFactorRef:
    """IntegratedLOAMFactor_: an edge part and a plane part; validation off by default (:385)"""

    def __init__(self, target_edges, target_planes, source_edges, source_planes, max_correspondence_distance=1.0):
        self.edge = PartRef(2, target_edges, source_edges, max_correspondence_distance)
        self.plane = PartRef(3, target_planes, source_planes, max_correspondence_distance)
        self.enable_correspondence_validation = False
        self.rejected = (0, 0)  # (edges, planes) of the last validation

    @property
    def parts(self):
        return [self.edge, self.plane]

    @property
    def searches(self):
        assert self.edge.searches == self.plane.searches
        return self.edge.searches

    def set_max_correspondence_distance(self, dist_edge, dist_plane):
        self.edge.max_sq, self.plane.max_sq = float(dist_edge) ** 2, float(dist_plane) ** 2

    def set_enable_correspondence_validation(self, enable):
        self.enable_correspondence_validation = bool(enable)

    def set_correspondence_update_tolerance(self, angle, trans):
        for p in self.parts:
            p.set_correspondence_update_tolerance(angle, trans)

    def update_correspondences(self, delta):
        """:444-449"""
        for p in self.parts:
            p.update_correspondences(delta)
        if self.enable_correspondence_validation:
            self.rejected = (self.edge.validate(), self.plane.validate())

    def evaluate(self, delta, derivatives=True):
        """:452-478: the edge part's result plus the plane part's"""
        e, p = self.edge.evaluate(delta, derivatives), self.plane.evaluate(delta, derivatives)
        with np.errstate(invalid="ignore"):
            return {k: e[k] + p[k] for k in e}

    def linearize(self, delta):
        self.update_correspondences(delta)
        return self.evaluate(delta)

    def error(self, delta):
        if self.edge.correspondences is None:
            self.update_correspondences(delta)
        return self.evaluate(delta, derivatives=False)["error"]

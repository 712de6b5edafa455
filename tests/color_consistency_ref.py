"""IntensityKdTree::knn_search (ann/intensity_kdtree.hpp, k = 1) and IntegratedColorConsistencyFactor_ (factors/impl/integrated_color_consistency_factor_impl.hpp)
restated in numpy, f64 on the f32 inputs.  A helper, not a test.

  nearest_xyzi(target, target_I, q, q_I, scale, max_sq)   brute force: per query the target index j that minimises d4^2(j) = |q - x_j|^2 + (I_q - scale I_j)^2 -- the
                                            scale on the STORED side only, as kdtree_get_pt writes it -- kept when d4^2 < max_sq (strict; the test the factors apply,
                                            :133), else -1.  Targets or queries with a non-finite coordinate or intensity never match.  Also each query's margins:
                                            to the runner-up, (d2 - d1) / d2, and to the cut-off, |d1 - max_sq| / max_sq (relative, squared distances).
  ColorConsistencyFactorRef
    update_correspondences(delta) :101-135  the tolerance rule, then the 3-D brute-force 1-NN (search="3d": what a plain KdTree does with pt[3]) or nearest_xyzi
                                            (search=("xyzi", scale)) of (T p, I_A), kept when the squared distance of THAT search is < max
    evaluate(delta)               :176-222  AS WRITTEN, in the reference's signs: r = T p_A - mu_B, projected - mu_B = r - (r . n_B) n_B, e = I_B + g_B . (projected -
                                            mu_B) - I_A, error = sum w e^2, J_e = g_B^T (I - n_B n_B^T) J with J_target = [[q]x, -I], J_source = [-R [p]x, R],
                                            H = sum J_e^T w J_e, b = sum J_e^T w e; w = photometric_term_weight (default 1.0, :31), R = delta's 3x3 block as given
  ColoredGICPXyziRef                        colored_ref.ColoredGICPFactorRef with the correspondences of nearest_xyzi (integrated_colored_gicp_factor_impl.hpp:121-127)

  textured_intensities(points)              the intensity field of the XYZI tests: texture at the scale of the point spacing of colored_ref.two_plane_cloud()
  textured_scene()                          that cloud with this field and a colored_ref.moved_copy of it: where the 4-D nearest and the 3-D nearest part ways
"""
import hashlib

import numpy as np

import colored_ref
from icp_ref import hat, nearest_two, pose_difference, transform

_CACHE = {}


def _f32_as_f64(a, shape):
    return np.asarray(a, dtype=np.float32).reshape(shape).astype(np.float64)


def nearest_xyzi(target, target_I, q, q_I, scale=1.0, max_sq=np.finfo(np.float64).max, chunk=256):
    """(index or -1 (Q,), d4^2 of the nearest (Q,; inf where no target is comparable), tie margin (Q,), cut-off margin (Q,)); inputs are taken as given (f64)"""
    target, q = np.asarray(target, dtype=np.float64).reshape(-1, 3), np.asarray(q, dtype=np.float64).reshape(-1, 3)
    stored = float(scale) * np.asarray(target_I, dtype=np.float64).reshape(-1)
    q_I = np.asarray(q_I, dtype=np.float64).reshape(-1)
    key = tuple(hashlib.blake2b(np.ascontiguousarray(a).tobytes(), digest_size=16).digest() for a in (target, stored, q, q_I))
    if key not in _CACHE:  # (the brute force is shared among the tests that ask for the same search, as icp_ref.nearest_two's is)
        idx, d1, d2 = np.full(len(q), -1, dtype=np.int64), np.full(len(q), np.inf), np.full(len(q), np.inf)
        for b in range(0, len(q) if len(target) else 0, chunk):
            e = min(b + chunk, len(q))
            with np.errstate(invalid="ignore", over="ignore"):
                d = (target[None, :, 0] - q[b:e, None, 0]) ** 2
                d += (target[None, :, 1] - q[b:e, None, 1]) ** 2
                d += (target[None, :, 2] - q[b:e, None, 2]) ** 2
                d += (q_I[b:e, None] - stored[None, :]) ** 2
            d[~np.isfinite(d)] = np.inf
            rows = np.arange(e - b)
            i = np.argmin(d, axis=1)  # the first of equals: the lowest index
            idx[b:e] = i
            d1[b:e] = d[rows, i]
            if d.shape[1] > 1:
                d[rows, i] = np.inf
                d2[b:e] = d.min(axis=1)
        _CACHE[key] = (idx, d1, d2)
    idx, d1, d2 = _CACHE[key]
    with np.errstate(invalid="ignore", divide="ignore"):
        tie = np.where(np.isfinite(d2), (d2 - d1) / np.maximum(d2, 1e-300), np.inf)
        cut = np.where(np.isfinite(d1), np.abs(d1 - max_sq) / max_sq, np.inf)
    return np.where(d1 < max_sq, idx, -1), d1, tie, cut


class ColorConsistencyFactorRef:
    def __init__(self, target_points, target_normals, target_intensities, target_gradients, source_points, source_intensities, max_correspondence_distance=1.0,
                 photometric_term_weight=1.0, search="3d"):
        self.target = _f32_as_f64(target_points, (-1, 3))
        self.normals = _f32_as_f64(target_normals, (-1, 3))
        self.target_intensities = _f32_as_f64(target_intensities, (-1,))
        self.gradients = _f32_as_f64(target_gradients, (-1, 3))
        self.source = _f32_as_f64(source_points, (-1, 3))
        self.source_intensities = _f32_as_f64(source_intensities, (-1,))
        self.max_sq = float(max_correspondence_distance) ** 2  # :30
        self.photometric_term_weight = float(photometric_term_weight)  # :31
        self.tol_rot = self.tol_trans = 0.0  # :32-33
        self.search = search
        self.correspondences = None
        self.last_correspondence_point = None
        self.searches = 0

    def set_correspondence_update_tolerance(self, angle, trans):
        self.tol_rot, self.tol_trans = float(angle), float(trans)

    def _search(self, delta):
        """(index or -1, tie margin, cut-off margin) of every source point at delta"""
        q = transform(delta, self.source)
        if self.search == "3d":
            idx, d1, d2 = nearest_two(self.target, q)
            with np.errstate(invalid="ignore", divide="ignore"):
                tie = np.where(np.isfinite(d2), (d2 - d1) / np.maximum(d2, 1e-300), np.inf)
            return np.where(d1 < self.max_sq, idx, -1), tie, np.abs(d1 - self.max_sq) / self.max_sq
        idx, _, tie, cut = nearest_xyzi(self.target, self.target_intensities, q, self.source_intensities, self.search[1], self.max_sq)
        return idx, tie, cut

    def update_correspondences(self, delta):
        delta = np.asarray(delta, dtype=np.float64)
        keep = self.correspondences is not None and (self.tol_trans > 0.0 or self.tol_rot > 0.0)  # :103
        if keep:
            diff_rot, diff_trans = pose_difference(delta, self.last_correspondence_point)
            keep = diff_rot < self.tol_rot and diff_trans < self.tol_trans
        if not keep:
            self.last_correspondence_point = np.array(delta)
            self.correspondences = self._search(delta)[0]  # :125-134
            self.searches += 1

    def margins(self, delta):
        _, tie, cut = self._search(np.asarray(delta, dtype=np.float64))
        return tie, cut

    def evaluate(self, delta, derivatives=True):
        delta = np.asarray(delta, dtype=np.float64)
        if self.correspondences is None:
            self.update_correspondences(delta)  # :146-148
        sel = np.flatnonzero(self.correspondences >= 0)
        c = self.correspondences[sel]
        p = self.source[sel]
        q = transform(delta, p)
        n, g = self.normals[c], self.gradients[c]
        r = q - self.target[c]
        offset = r - (r * n).sum(axis=1)[:, None] * n  # projected - mean_B, :193-194
        e = self.target_intensities[c] + (g * offset).sum(axis=1) - self.source_intensities[sel]  # :195
        w = self.photometric_term_weight
        out = dict(error=float((e * w * e).sum()), num_inliers=int(len(sel)))  # :197
        if not derivatives:
            return out
        R = delta[:3, :3]
        Jt = np.concatenate([hat(q), np.broadcast_to(-np.eye(3), (len(sel), 3, 3))], axis=2)   # :203-205
        Js = np.concatenate([-(R[None] @ hat(p)), np.broadcast_to(R, (len(sel), 3, 3))], axis=2)  # :207-209
        P = np.eye(3)[None] - n[:, :, None] * n[:, None, :]  # :212-214
        ge = np.einsum("ni,nij->nj", g, P)  # J_ephoto_transed, :216-217
        Jet, Jes = np.einsum("nk,nkj->nj", ge, Jt), np.einsum("nk,nkj->nj", ge, Js)  # :219-220
        out["H_target"] = w * np.einsum("ni,nj->ij", Jet, Jet)
        out["H_source"] = w * np.einsum("ni,nj->ij", Jes, Jes)
        out["H_target_source"] = w * np.einsum("ni,nj->ij", Jet, Jes)
        out["b_target"] = w * np.einsum("ni,n->i", Jet, e)
        out["b_source"] = w * np.einsum("ni,n->i", Jes, e)
        return out

    def linearize(self, delta):
        self.update_correspondences(delta)
        return self.evaluate(delta)

    def error(self, delta):
        return self.evaluate(delta, derivatives=False)["error"]


class ColoredGICPXyziRef(colored_ref.ColoredGICPFactorRef):
    """the colored GICP restatement on XYZI correspondences: only the search differs"""

    def __init__(self, *args, intensity_scale=1.0, **kw):
        super().__init__(*args, **kw)
        self.intensity_scale = float(intensity_scale)

    def _search(self, delta):
        return nearest_xyzi(self.target, self.target_intensities, transform(delta, self.source), self.source_intensities, self.intensity_scale, self.max_sq)

    def update_correspondences(self, delta):
        delta = np.asarray(delta, dtype=np.float64)
        keep = self.correspondences is not None and (self.tol_trans > 0.0 or self.tol_rot > 0.0)
        if keep:
            diff_rot, diff_trans = pose_difference(delta, self.last_correspondence_point)
            keep = diff_rot < self.tol_rot and diff_trans < self.tol_trans
        if not keep:
            self.last_correspondence_point = np.array(delta)
            self.correspondences = self._search(delta)[0]
            self.searches += 1
        sel = np.flatnonzero(self.correspondences >= 0)
        R = delta[:3, :3]
        self.mahalanobis = np.linalg.inv(self.target_covs[self.correspondences[sel]] + R[None] @ self.source_covs[sel] @ R.T[None])

    def margins(self, delta):
        _, _, tie, cut = self._search(np.asarray(delta, dtype=np.float64))
        return tie, cut


# ---- the scene of the XYZI tests ------------------------------------------------------------------------------------------------------------------------------------
# two_plane_cloud() holds 2,000 points per 4 m x 4 m plane: a mean spacing of 9 cm.  The field below varies over WAVELENGTH = 20 cm in every direction, so neighbouring
# points differ in intensity by a good part of AMPLITUDE.  With AMPLITUDE = 0.5 an intensity difference between neighbours (up to 1.0) outweighs their 9 cm (0.008 m^2)
# in d4^2, so that a source point 10 cm off its own target point -- the GPU tests' "identity" pose -- is nearer in XYZI to the point it was copied from than to the
# stranger beside it.  Chosen on the CPU; tests/test_color_consistency_ref_cpu.py holds the scene to what the GPU tests need of it.
WAVELENGTH = 0.2
AMPLITUDE = 0.5
XI = np.array([0.01, -0.02, 0.015, 0.10, -0.05, 0.03])  # tests/test_colored_gicp_gpu.py's T_GT = Expmap(XI)


def textured_intensities(points, amplitude=AMPLITUDE, wavelength=WAVELENGTH):
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    k = 2.0 * np.pi / wavelength
    return np.ascontiguousarray(0.5 + amplitude * np.sin(k * p[:, 0] + 0.7) * np.sin(k * p[:, 1] + 0.3) * np.cos(k * p[:, 2]), dtype=np.float32)


def textured_scene():
    """dict(tp, tI, sp, sI, T_GT): colored_ref.two_plane_cloud() under textured_intensities and colored_ref.moved_copy of it by T_GT (seeds fixed there)"""
    from helpers import expmap

    tp, _ = colored_ref.two_plane_cloud()
    tI = textured_intensities(tp)
    T_GT = expmap(XI)
    sp, sI = colored_ref.moved_copy(tp, tI, T_GT)
    return dict(tp=tp, tI=tI, sp=sp, sI=sI, T_GT=T_GT)

"""numpy statement of gtsam::Pose3 (GTSAM 4.2, default build: GTSAM_POSE3_EXPMAP on, GTSAM_SLOW_BUT_CORRECT_BETWEENFACTOR off) and of the two factors the device
linearises (csrc/gp_pose_factors.hpp): SO3::Logmap, Pose3::Logmap, AdjointMap, BetweenFactor<Pose3> and PriorFactor<Pose3> with a Gaussian noise model, written out
here independently of the kernel, plus a host LM graph of them in bench_lm's back-end shape."""
import numpy as np

import bench_lm


def skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def expmap(xi):
    return bench_lm.expmap_many(np.asarray(xi, dtype=np.float64).reshape(1, 6))[0]


def inverse(T):
    return bench_lm.inv_many(np.asarray(T, dtype=np.float64)[None])[0]


def so3_logmap(R):
    """SO3::Logmap, so3.cpp: near pi from the largest diagonal entry; the series near 0; acos otherwise"""
    (R11, R12, R13), (R21, R22, R23), (R31, R32, R33) = R
    tr = R11 + R22 + R33
    if tr + 1.0 < 1e-3:
        if R33 > R22 and R33 > R11:
            W, Q1, Q2, Q3 = R21 - R12, 2.0 + 2.0 * R33, R31 + R13, R23 + R32
            order = lambda a, b, c: (b, c, a)  # noqa: E731  (Q2, Q3, Q1)
        elif R22 > R11:
            W, Q1, Q2, Q3 = R13 - R31, 2.0 + 2.0 * R22, R23 + R32, R12 + R21
            order = lambda a, b, c: (c, a, b)  # noqa: E731  (Q3, Q1, Q2)
        else:
            W, Q1, Q2, Q3 = R32 - R23, 2.0 + 2.0 * R11, R12 + R21, R31 + R13
            order = lambda a, b, c: (a, b, c)  # noqa: E731
        r = np.sqrt(Q1)
        norm = np.sqrt(Q1 * Q1 + Q2 * Q2 + Q3 * Q3 + W * W)
        sgn_w = -1.0 if W < 0 else 1.0
        mag = np.pi - (2 * sgn_w * W) / norm
        scale = 0.5 / r * mag
        return sgn_w * scale * np.array(order(Q1, Q2, Q3))
    tr_3 = tr - 3.0
    if tr_3 < -1e-6:
        theta = np.arccos((tr - 1.0) / 2.0)
        magnitude = theta / (2.0 * np.sin(theta))
    else:
        magnitude = 0.5 - tr_3 / 12.0 + tr_3 * tr_3 / 60.0
    return magnitude * np.array([R32 - R23, R13 - R31, R21 - R12])


def pose3_logmap(T):
    """Pose3::Logmap, pose3.cpp: (w, t - 1/2 theta W t + (1 - theta / (2 tan(theta / 2))) W W t), W = skew(w / theta)"""
    w = so3_logmap(T[:3, :3])
    t = T[:3, 3]
    th = np.linalg.norm(w)
    if th < 1e-10:
        return np.concatenate([w, t])
    W = skew(w / th)
    WT = W @ t
    return np.concatenate([w, t - (0.5 * th) * WT + (1 - th / (2.0 * np.tan(0.5 * th))) * (W @ WT)])


def adjoint(T):
    """Pose3::AdjointMap in (omega, v) order"""
    R, t = T[:3, :3], T[:3, 3]
    A = np.zeros((6, 6))
    A[:3, :3] = R
    A[3:, :3] = skew(t) @ R
    A[3:, 3:] = R
    return A


def between_error(Ta, Tb, Z):
    return pose3_logmap(inverse(Z) @ (inverse(Ta) @ Tb))


def between_jacobians(Ta, Tb):
    """BetweenFactor<Pose3>::evaluateError's H1, H2 (without LogmapDerivative(e): GTSAM's default)"""
    return -adjoint(inverse(inverse(Ta) @ Tb)), np.eye(6)


def prior_error(Ta, Z):
    return pose3_logmap(inverse(Z) @ Ta)


def record(kind, Ta, Tb, Z, Lam):
    """the gp_linearized6 record of a factor (kind 0 between, 1 prior; Tb unused for a prior) as a [122] array"""
    rec = np.zeros(122)
    if kind == 0:
        e = between_error(Ta, Tb, Z)
        Ja, Jb = between_jacobians(Ta, Tb)
        Ht, Hs, Hts, bt, bs = Ja.T @ Lam @ Ja, Jb.T @ Lam @ Jb, Ja.T @ Lam @ Jb, Ja.T @ Lam @ e, Jb.T @ Lam @ e
    else:
        e = prior_error(Ta, Z)
        Ht, Hs, Hts, bt, bs = np.zeros((6, 6)), Lam, np.zeros((6, 6)), np.zeros(6), Lam @ e
    rec[1] = 0.5 * e @ Lam @ e
    rec[2:38], rec[38:74], rec[74:110] = Ht.T.ravel(), Hs.T.ravel(), Hts.T.ravel()
    rec[110:116], rec[116:122] = bt, bs
    return rec


def factor_record(f, values):
    """record of a BetweenFactorPose3 / PriorFactorPose3 at values [N, 4, 4]"""
    if len(f.keys) == 2:
        return record(0, values[f.keys[0]], values[f.keys[1]], f.measured, f.information)
    return record(1, values[f.keys[0]], None, f.measured, f.information)


def factor_error(f, values):
    return float(factor_record(f, values)[1])


def factor_slots(pose_factors, slot):
    return np.array([(slot[f.keys[0]], slot[f.keys[1]]) if len(f.keys) == 2 else (-1, slot[f.keys[0]]) for f in pose_factors], dtype=np.int32).reshape(-1, 2)


class HostPoseGraph(bench_lm._Graph):
    """run_lm's back-end over numpy pose factors and, optionally, VGICP records linearised host-driven on the GPU (`vgicp`: a bench_lm.GpuGraph with solver="host"
    over the same poses); every pose a variable (fixed = -1); solve = numpy on A + lambda I, as bench_lm's host solver"""

    name = "host-pose"

    def __init__(self, pose_factors, num_poses, vgicp=None):
        pairs = vgicp.pairs if vgicp is not None else np.zeros((0, 2), dtype=np.int64)
        super().__init__(pairs, num_poses, fixed=-1)
        self.pf = list(pose_factors)
        self.vgicp = vgicp
        self.slots_all = np.concatenate([self.factor_slots, factor_slots(self.pf, self.slot)]).astype(np.int32)

    def close(self):
        if self.vgicp is not None:
            self.vgicp.close()

    def linearize(self, values):
        recs = [factor_record(f, values) for f in self.pf]
        if self.vgicp is not None:
            self.vgicp.linearize(values)
            recs = list(self.vgicp.rec_host) + recs
        self.rec = np.array(recs)
        self.A, self.b, c = bench_lm.host_system(self.rec, self.slots_all, self.num_slots)
        return c

    def solve(self, lam):
        return np.linalg.solve(self.A + lam * np.eye(len(self.b)), self.b), self.b, None

    def error(self, values):
        e = self.vgicp.error(values) if self.vgicp is not None else 0.0
        return e + float(sum(factor_error(f, values) for f in self.pf))

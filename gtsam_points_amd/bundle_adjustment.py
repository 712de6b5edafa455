"""BALM bundle adjustment by eigenvalue minimisation on the device (gp_ba_factors_*, csrc/gp_ba_factors.hip).

  PlaneEVMFactorGPU / EdgeEVMFactorGPU <- PlaneEVMFactor / EdgeEVMFactor (factors/bundle_adjustment_factor_evm.hpp, balm_feature.hpp)
  BundleAdjustmentFactorsGPU           -- any number of them linearised in two launches into gp_linearized6 records for DenseLinearSystemGPU / SparseLinearSystemGPU

A factor is one feature (a plane or an edge) seen from K poses with N points p_i; with q_i = T_key(i) p_i its error is an eigenvalue of cov(q).  The Hessian
factor is the reference's, (keys, scale D^T H D, -scale J D, scale lambda) with D_i = [-[q_i]x, I]: the derivative for a world-frame (left) perturbation, tangent
order (omega, v).  The solvers' step xi therefore updates T <- Exp(xi) T.
"""
import ctypes as C

import numpy as np

from . import _capi
from .factors import HessianFactor
from .solver import _values16

GP_BA_PLANE, GP_BA_EDGE = 0, 1


class _EVMFactorGPU:
    kind = None

    def __init__(self):
        self._keys = []  # first-seen order, as the reference's keys_
        self.point_keys = []
        self.points = []
        self.error_scale = 1.0
        self._set = None

    def add(self, point, key):
        key = int(key)
        if key not in self._keys:
            self._keys.append(key)
        self.point_keys.append(key)
        self.points.append(np.asarray(point, dtype=np.float64).reshape(3).copy())
        self._set = None

    def set_scale(self, scale):
        self.error_scale = float(scale)
        self._set = None

    def num_points(self):
        return len(self.points)

    def keys(self):
        return list(self._keys)

    def _own_set(self):
        """a set of this factor alone over its own poses, numbered in ascending key order (the order of gp_ba_factors_feature_hessian)"""
        if self._set is None:
            self._sorted_keys = sorted(self._keys)
            index = {k: i for i, k in enumerate(self._sorted_keys)}
            self._set = BundleAdjustmentFactorsGPU([self], len(index), _pose_of_key=index)
        return self._set

    def _own_values(self, values):
        self._own_set()
        return np.stack([np.asarray(values[k], dtype=np.float64).reshape(4, 4) for k in self._sorted_keys])

    def error(self, values):
        """values: key -> 4 x 4 pose (a dict or an array indexed by key)"""
        v = self._own_values(values)
        return float(self._set.errors(v)[0])

    def linearize(self, values):
        """-> HessianFactor over the K keys in first-seen order: G[(i, j)] for i <= j, g, f"""
        v = self._own_values(values)
        G, g, f = self._set.feature_hessian(0, v)
        at = [self._sorted_keys.index(k) for k in self._keys]
        blocks = {(i, j): G[6 * at[i]:6 * at[i] + 6, 6 * at[j]:6 * at[j] + 6].copy() for i in range(len(at)) for j in range(i, len(at))}
        return HessianFactor(self._keys, blocks, [g[6 * a:6 * a + 6].copy() for a in at], f)


class PlaneEVMFactorGPU(_EVMFactorGPU):
    """PlaneEVMFactor: error = error_scale x the smallest eigenvalue of the covariance of the transformed points"""

    kind = GP_BA_PLANE


class EdgeEVMFactorGPU(_EVMFactorGPU):
    """EdgeEVMFactor: error = the sum of the two smallest eigenvalues.  As in the reference, set_scale has NO effect on an edge factor: EdgeEVMFactor::error and
    ::linearize do not apply error_scale, and neither does the device."""

    kind = GP_BA_EDGE


class BundleAdjustmentFactorsGPU:
    """PlaneEVMFactorGPU / EdgeEVMFactorGPU objects whose keys are pose indices 0..num_poses-1.  linearize writes R = len(self) records: a unary record per pose that a
    factor touches (in pose order), then a pair record per co-observed pose pair a < b; factor_slots(slot) gives the (target, source) slots the linear systems take
    for them.  A factor's points may have been added in any key order."""

    def __init__(self, factors, num_poses, stream=None, _pose_of_key=None):
        self._lib = _capi.load()
        self.factors = list(factors)
        self.num_poses = int(num_poses)
        self.stream = stream
        if not self.factors:
            raise ValueError("no factors")
        pose_of = (lambda k: k) if _pose_of_key is None else _pose_of_key.__getitem__
        kinds = np.array([f.kind for f in self.factors], dtype=np.int32)
        scales = np.array([f.error_scale for f in self.factors], dtype=np.float64)
        offsets = np.zeros(len(self.factors) + 1, dtype=np.int32)
        offsets[1:] = np.cumsum([f.num_points() for f in self.factors])
        point_pose = np.array([pose_of(k) for f in self.factors for k in f.point_keys], dtype=np.int32)
        points = np.ascontiguousarray(np.array([p for f in self.factors for p in f.points], dtype=np.float64).reshape(-1, 3))
        h = C.c_void_p()
        _capi.check(self._lib.gp_ba_factors_create(kinds.ctypes.data, scales.ctypes.data, offsets.ctypes.data, point_pose.ctypes.data, points.ctypes.data, len(self.factors),
                                                   len(points), self.num_poses, stream, C.byref(h)), "gp_ba_factors_create")
        self._h = h
        self.num_records = self._lib.gp_ba_factors_num_records(h)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.gp_ba_factors_destroy(self._h)
            self._h = None

    __del__ = close

    def __len__(self):
        return self.num_records

    def factor_slots(self, slot):
        s = np.ascontiguousarray(slot, dtype=np.int32)
        if s.shape != (self.num_poses,):
            raise ValueError(f"slot must have {self.num_poses} entries")
        out = np.zeros((self.num_records, 2), dtype=np.int32)
        _capi.check(self._lib.gp_ba_factors_factor_slots(self._h, s.ctypes.data, out.ctypes.data), "gp_ba_factors_factor_slots")
        return out

    def errors(self, values):
        """-> [F] each factor's error(), synchronous"""
        out = np.zeros(len(self.factors))
        v = _values16(values, self.num_poses)
        _capi.check(self._lib.gp_ba_factors_compute_errors(self._h, v.ctypes.data, out.ctypes.data), "gp_ba_factors_compute_errors")
        return out

    def linearize(self, values):
        """-> [R, 122] float64 records (host), synchronous"""
        out = np.zeros((self.num_records, _capi.LINEARIZED6_DOUBLES))
        v = _values16(values, self.num_poses)
        _capi.check(self._lib.gp_ba_factors_linearize(self._h, v.ctypes.data, out.ctypes.data), "gp_ba_factors_linearize")
        return out

    def linearize_on_device(self, values, device="cuda:0"):
        """-> [R, 122] float64 CUDA tensor of records (nothing is copied to the host); values: [num_poses, 4, 4] host array or [num_poses, 16] column-major CUDA tensor"""
        import torch

        if isinstance(values, torch.Tensor):
            poses = values.to(dtype=torch.float64).contiguous()
        else:
            poses = torch.from_numpy(_values16(values, self.num_poses)).to(device)
        if tuple(poses.shape) != (self.num_poses, 16):
            raise ValueError(f"device values must be [{self.num_poses}, 16] (column-major 4x4)")
        out = torch.zeros((self.num_records, _capi.LINEARIZED6_DOUBLES), dtype=torch.float64, device=poses.device)
        torch.cuda.current_stream(out.device).synchronize()
        _capi.check(self._lib.gp_ba_factors_issue_linearize_dev(self._h, C.c_void_p(poses.data_ptr()), C.c_void_p(out.data_ptr())), "gp_ba_factors_issue_linearize_dev")
        _capi.check(self._lib.gp_stream_synchronize(self.stream), "gp_stream_synchronize")
        return out

    def feature_hessian(self, i, values):
        """factor i's own dense Hessian factor over its poses in ascending pose order: (G [6K, 6K], g [6K], f)"""
        K = self._lib.gp_ba_factors_feature_num_poses(self._h, int(i))
        G, g, f = np.zeros((6 * K, 6 * K)), np.zeros(6 * K), np.zeros(1)
        v = _values16(values, self.num_poses)
        _capi.check(self._lib.gp_ba_factors_feature_hessian(self._h, int(i), v.ctypes.data, G.ctypes.data, g.ctypes.data, f.ctypes.data), "gp_ba_factors_feature_hessian")
        return G.T.copy(), g, float(f[0])

"""The step after the path: the damped normal equations of a graph of VGICP factors, assembled and solved on the device.

  DenseLinearSystemGPU  <- DenseLinearSystemBuilder (optimizers/linear_system_builder.cpp:39-48)
                           + buildDampedSystem       (optimizers/levenberg_marquardt_ext.cpp:146-161)
                           + DenseLinearSolver::solve (optimizers/linear_solver.hpp:18-22)
  SparseLinearSystemGPU <- SparseLinearSystemBuilder<6> (optimizers/linear_system_builder.hpp:41-72) + buildDampedSystem
                           + SparseLinearSolver::solve (optimizers/linear_solver.hpp:24-29): block-sparse LL^T over the pose graph
  linearize_on_device   -- one batched linearise whose records stay in HBM (what the solver consumes)
  BetweenFactorPose3 / PriorFactorPose3 / PoseFactorsGPU
                        <- gtsam::BetweenFactor<Pose3> / gtsam::PriorFactor<Pose3> with a Gaussian noise model, linearised on the device into the same records

Poses that are variables get a slot (0..num_slots-1); a factor key without a slot (a fixed pose) drops out of the system.
"""
import ctypes as C

import numpy as np

from . import _capi


def linearize_on_device(factors, values, device="cuda:0", stream=None):
    """Batched linearise of IntegratedVGICPFactorGPU objects; returns a [F, 122] float64 CUDA tensor of gp_linearized6
    records (nothing is copied to the host)."""
    import torch

    lib = _capi.load()
    F = len(factors)
    poses = np.zeros((F, 16))
    for i, f in enumerate(factors):
        f.set_linearization_point(values, poses[i])
    arr = (C.c_void_p * F)(*[f._h.value for f in factors])
    batch = C.c_void_p()
    _capi.check(lib.gp_vgicp_batch_create(arr, F, stream, C.byref(batch)), "gp_vgicp_batch_create")
    out = torch.zeros((F, _capi.LINEARIZED6_DOUBLES), dtype=torch.float64, device=device)
    torch.cuda.current_stream(out.device).synchronize()
    try:
        _capi.check(lib.gp_vgicp_batch_issue_linearize(batch, poses.ctypes.data, C.c_void_p(out.data_ptr())), "gp_vgicp_batch_issue_linearize")
        _capi.check(lib.gp_vgicp_batch_sync(batch), "gp_vgicp_batch_sync")
    finally:
        lib.gp_vgicp_batch_destroy(batch)
    return out


def _information(information, sigmas):
    """Lambda in (omega, v) order: `information` as given, or diag(sigmas^-2) (noiseModel::Diagonal::Sigmas); neither = the unit model"""
    if information is not None and sigmas is not None:
        raise ValueError("give information or sigmas, not both")
    if sigmas is not None:
        s = np.asarray(sigmas, dtype=np.float64).reshape(-1)
        if s.shape != (6,):
            raise ValueError("sigmas must have 6 entries (omega, v)")
        return np.diag(1.0 / (s * s))
    lam = np.eye(6) if information is None else np.asarray(information, dtype=np.float64)
    if lam.shape != (6, 6):
        raise ValueError("information must be 6 x 6")
    return lam


class BetweenFactorPose3:
    """gtsam::BetweenFactor<Pose3>(key1, key2, measured, Gaussian noise): e = Logmap(measured^-1 T_key1^-1 T_key2), GTSAM's default Jacobians.
    information: Lambda 6 x 6 in (omega, v) order (noiseModel->R()^T R()); sigmas: noiseModel::Diagonal::Sigmas instead."""

    kind = _capi.GP_POSE_FACTOR_BETWEEN

    def __init__(self, key1, key2, measured, information=None, sigmas=None):
        self.keys = (int(key1), int(key2))
        self.measured = np.asarray(measured, dtype=np.float64).reshape(4, 4).copy()
        self.information = _information(information, sigmas)

    def _struct(self):
        f = _capi.PoseFactor()
        f.kind, f.pose_a, f.pose_b = self.kind, self.keys[0], self.keys[1] if len(self.keys) > 1 else -1
        f.measured[:] = np.ascontiguousarray(self.measured.T).reshape(16)
        f.information[:] = np.ascontiguousarray(self.information.T).reshape(36)
        return f


class PriorFactorPose3(BetweenFactorPose3):
    """gtsam::PriorFactor<Pose3>(key, prior, Gaussian noise): e = Logmap(prior^-1 T_key), J = I"""

    kind = _capi.GP_POSE_FACTOR_PRIOR

    def __init__(self, key, prior, information=None, sigmas=None):
        self.keys = (int(key),)
        self.measured = np.asarray(prior, dtype=np.float64).reshape(4, 4).copy()
        self.information = _information(information, sigmas)


def _pose_factor_array(pose_factors):
    arr = (_capi.PoseFactor * max(len(pose_factors), 1))()
    for i, f in enumerate(pose_factors):
        arr[i] = f._struct()
    return arr


def _values16(values, num_poses):
    v = np.asarray(values, dtype=np.float64)
    if v.shape != (num_poses, 4, 4):
        raise ValueError(f"values must be [{num_poses}, 4, 4]")
    return np.ascontiguousarray(v.transpose(0, 2, 1)).reshape(num_poses, 16)


class PoseFactorsGPU:
    """BetweenFactorPose3 / PriorFactorPose3 objects over poses 0..num_poses-1, linearised on the device (gp_pose_factors_*) into gp_linearized6 records: a between
    factor's target is key1 and its source key2, a prior is a unary record on its source side.  factor_slots(slot) gives the (target, source) slots that
    DenseLinearSystemGPU / SparseLinearSystemGPU take for these records: (slot[key1], slot[key2]) and (-1, slot[key])."""

    def __init__(self, factors, num_poses, stream=None):
        self._lib = _capi.load()
        self.factors = list(factors)
        self.num_poses = int(num_poses)
        self.stream = stream
        h = C.c_void_p()
        _capi.check(self._lib.gp_pose_factors_create(_pose_factor_array(self.factors), len(self.factors), self.num_poses, stream, C.byref(h)), "gp_pose_factors_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.gp_pose_factors_destroy(self._h)
            self._h = None

    __del__ = close

    def __len__(self):
        return len(self.factors)

    def factor_slots(self, slot):
        slot = np.asarray(slot)
        return np.array([(slot[f.keys[0]], slot[f.keys[1]]) if len(f.keys) == 2 else (-1, slot[f.keys[0]]) for f in self.factors], dtype=np.int32).reshape(-1, 2)

    def linearize(self, values):
        """-> [P, 122] float64 records (host), synchronous"""
        out = np.zeros((len(self.factors), _capi.LINEARIZED6_DOUBLES))
        v = _values16(values, self.num_poses)  # (held: the library reads it through its raw pointer)
        _capi.check(self._lib.gp_pose_factors_linearize(self._h, v.ctypes.data, out.ctypes.data), "gp_pose_factors_linearize")
        return out

    def error(self, values):
        """-> [P] the factors' error() = 1/2 e^T Lambda e, synchronous"""
        out = np.zeros(len(self.factors))
        v = _values16(values, self.num_poses)
        _capi.check(self._lib.gp_pose_factors_compute_error(self._h, v.ctypes.data, out.ctypes.data), "gp_pose_factors_compute_error")
        return out

    def linearize_on_device(self, values, device="cuda:0"):
        """-> [P, 122] float64 CUDA tensor of records (nothing is copied to the host); values: [num_poses, 4, 4] host array or [num_poses, 16] column-major CUDA tensor"""
        import torch

        if isinstance(values, torch.Tensor):
            poses = values.to(dtype=torch.float64).contiguous()
        else:
            poses = torch.from_numpy(_values16(values, self.num_poses)).to(device)
        if tuple(poses.shape) != (self.num_poses, 16):
            raise ValueError(f"device values must be [{self.num_poses}, 16] (column-major 4x4)")
        out = torch.zeros((len(self.factors), _capi.LINEARIZED6_DOUBLES), dtype=torch.float64, device=poses.device)
        torch.cuda.current_stream(out.device).synchronize()
        _capi.check(self._lib.gp_pose_factors_issue_linearize_dev(self._h, C.c_void_p(poses.data_ptr()), C.c_void_p(out.data_ptr())), "gp_pose_factors_issue_linearize_dev")
        _capi.check(self._lib.gp_stream_synchronize(self.stream), "gp_stream_synchronize")
        return out


class _LinearSystemGPU:
    """What the dense and the sparse system share: the C entry points gp_<prefix>_*, keyed by _PREFIX and bound once per system, so that a
    call costs no more host time than a direct one (no name formatting or lookup per call)."""

    _PREFIX = None

    def _create(self, num_slots, factor_slots, stream, *extra):
        lib = self._lib = _capi.load()
        self._create_fn, self._destroy, self._build, self._download, self._solve, self._step = (
            getattr(lib, f"{self._PREFIX}_{op}") for op in ("create", "destroy", "build", "download", "solve", "step"))
        self.num_slots = int(num_slots)
        self.factor_slots = np.ascontiguousarray(np.asarray(factor_slots, dtype=np.int32).reshape(-1, 2))
        self.stream = stream
        h = C.c_void_p()
        _capi.check(self._create_fn(self.num_slots, self.factor_slots.ctypes.data, len(self.factor_slots), *extra, stream, C.byref(h)), self._create_fn.__name__)
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._destroy(h)
            self._h = None

    @property
    def size(self):
        return 6 * self.num_slots

    def _check_args(self, records_dev, prior_diag):
        """-> the prior as a contiguous float64 array (or None) after the checks of records_dev and prior_diag"""
        if tuple(records_dev.shape) != (len(self.factor_slots), _capi.LINEARIZED6_DOUBLES) or not records_dev.is_contiguous():
            raise ValueError("records_dev must be a contiguous [num_factors, 122] float64 device tensor")
        if prior_diag is None:
            return None
        prior = np.ascontiguousarray(prior_diag, dtype=np.float64)
        if prior.shape != (self.size,):
            raise ValueError("prior_diag must have 6 * num_slots entries")
        return prior

    def build(self, records_dev, lam=0.0, diagonal_damping=False, min_diagonal=1e-6, max_diagonal=1e32, prior_diag=None):
        """records_dev: [F, 122] float64 CUDA tensor.  lam / diagonal_damping: buildDampedSystem; prior_diag: optional
        extra diagonal (length 6 * num_slots)."""
        prior = self._check_args(records_dev, prior_diag)
        _capi.check(
            self._build(self._h, C.c_void_p(records_dev.data_ptr()), float(lam), int(bool(diagonal_damping)), float(min_diagonal), float(max_diagonal),
                              prior.ctypes.data if prior is not None else None),
            self._build.__name__,
        )
        return self

    def download(self):
        """(A dense symmetric [n, n], b, c) in slot order -- for checkers"""
        n = self.size
        A, b, c = np.zeros((n, n)), np.zeros(n), np.zeros(1)
        _capi.check(self._download(self._h, A.ctypes.data, b.ctypes.data, c.ctypes.data), self._download.__name__)
        return A.T.copy(), b, float(c[0])  # column-major -> numpy (symmetric anyway)

    def solve(self):
        """x with A x = b (consumes the built system); raises GPError when A is not positive definite."""
        x = np.zeros(self.size)
        _capi.check(self._solve(self._h, x.ctypes.data, None), self._solve.__name__)
        return x

    def step(self, records_dev, lam=0.0, diagonal_damping=False, min_diagonal=1e-6, max_diagonal=1e32, prior_diag=None, out=None):
        """build + download(b, c) + solve as ONE call with one synchronisation -- two with a prior_diag -- (gp_*_system_step): -> (x, b, c); the optimizer's tryLambda
        (levenberg_marquardt_ext.cpp:188-260).  out: optional (x, b, c) float64 arrays to fill ([n], [n], [1]) instead of new ones.  Raises GPError (indeterminate) when the
        damped system is not positive definite; out's b and c are filled even then."""
        prior = self._check_args(records_dev, prior_diag)
        x, b, c = _step_out(out, self.size)
        _capi.check(
            self._step(self._h, C.c_void_p(records_dev.data_ptr()), float(lam), int(bool(diagonal_damping)), float(min_diagonal), float(max_diagonal),
                             prior.ctypes.data if prior is not None else None, x.ctypes.data, b.ctypes.data, c.ctypes.data),
            self._step.__name__,
        )
        return x, b, float(c[0])


class DenseLinearSystemGPU(_LinearSystemGPU):
    """A x = b over 6-dof pose slots, built from stacked device-resident gp_linearized6 records.

    factor_slots: [(target_slot, source_slot)] per factor; a negative slot = that pose is not a variable."""

    _PREFIX = "gp_dense_system"

    def __init__(self, num_slots, factor_slots, stream=None):
        self._create(num_slots, factor_slots, stream)

    def set_one_launch(self, enable=True):
        """a system of ONE pose runs step() as one launch (default); False: the multi-launch path (bit-identical: tests, A/B).  -> what the next step() runs"""
        return bool(self._lib.gp_dense_system_set_one_launch(self._h, 1 if enable else 0))


def _step_out(out, n):
    """(x, b, c) buffers of a step() call: the C entry points memcpy n, n and 1 doubles into them through their raw pointers, so anything that is not a
    C-contiguous float64 array of exactly that shape is refused here"""
    if out is None:
        return np.zeros(n), np.zeros(n), np.zeros(1)
    if len(out) != 3:
        raise ValueError("out must be (x, b, c)")
    for arr, shape, name in zip(out, ((n,), (n,), (1,)), "xbc"):
        if not (isinstance(arr, np.ndarray) and arr.dtype == np.float64 and arr.shape == shape and arr.flags.c_contiguous and arr.flags.writeable):
            raise ValueError(f"out[{name}] must be a writable C-contiguous float64 array of shape {shape}")
    return out


def sparse_symbolic(num_slots, factor_slots, ordering=0):
    """The symbolic phase of SparseLinearSystemGPU alone (host code, no device needed): dict(perm, parent, nnz_a_blocks,
    nnz_l_blocks, num_subtrees, top_columns)."""
    lib = _capi.load()
    fs = np.ascontiguousarray(np.asarray(factor_slots, dtype=np.int32).reshape(-1, 2))
    perm, parent = np.zeros(num_slots, np.int32), np.zeros(num_slots, np.int32)
    na, nl, ns, nt = C.c_int64(), C.c_int64(), C.c_int(), C.c_int()
    _capi.check(lib.gp_sparse_symbolic(int(num_slots), fs.ctypes.data, len(fs), int(ordering), perm.ctypes.data, parent.ctypes.data, C.byref(na), C.byref(nl), C.byref(ns),
                                       C.byref(nt)), "gp_sparse_symbolic")
    lv, cc, wl = C.c_int(), C.c_int(), C.c_int()
    _capi.check(lib.gp_sparse_symbolic_schedule(int(num_slots), fs.ctypes.data, len(fs), int(ordering), C.byref(lv), C.byref(cc), C.byref(wl)), "gp_sparse_symbolic_schedule")
    arr = [np.zeros(max(wl.value, 1), np.int32) for _ in range(4)]
    _capi.check(lib.gp_debug_sparse_work_lists(int(num_slots), fs.ctypes.data, len(fs), int(ordering), len(arr[0]), *[a.ctypes.data for a in arr]), "gp_debug_sparse_work_lists")
    lists = [dict(level=int(arr[0][i]), columns=int(arr[1][i]), products=int(arr[2][i]), max_column_products=int(arr[3][i])) for i in range(wl.value)]
    return dict(perm=perm, parent=parent, nnz_a_blocks=na.value, nnz_l_blocks=nl.value, num_subtrees=ns.value, top_columns=nt.value, num_levels=lv.value,
                critical_columns=cc.value, num_lists=wl.value, work_lists=lists)


class SparseLinearSystemGPU(_LinearSystemGPU):
    """A x = b over 6-dof pose slots as a block-sparse lower triangle, solved by a block-sparse LL^T on the device.

    factor_slots as for DenseLinearSystemGPU; ordering: "natural" (slot order = elimination order), "nd" (nested dissection), "amd" (minimum degree by
    multiple elimination: the fill of the COLAMD-class orderings GTSAM gives the reference), "amd1" (the same with a slack of one on the degree) or
    "auto" (default: "nd" and "amd1" are both tried, the schedule with the shorter critical path is kept)."""

    ORDERINGS = {"natural": 0, "nd": 1, "amd": 2, "amd1": 3, "auto": 4}
    _PREFIX = "gp_sparse_system"

    def __init__(self, num_slots, factor_slots, ordering="auto", stream=None):
        self._create(num_slots, factor_slots, stream, self.ORDERINGS[ordering])

    def set_one_launch(self, enable=True):
        """step() of a system whose factor fits one compute unit's LDS (<= 128 poses, <= ~440 blocks of L) runs as ONE launch by default; False selects the multi-launch
        form, "teams" the one-launch step's first form (every list a team of waves in lock step), "lone-waves" its second (a work list per wave; the default gives a list a team of
        waves that meet without workgroup barriers where the level has at most four lists, and a lone wave otherwise) -- all bit-identical: the switch is for the test that
        says so and for timing.  Returns what the next step() runs (True: one launch)."""
        return bool(self._lib.gp_sparse_system_set_one_launch(self._h, 2 if enable == "teams" else (3 if enable == "lone-waves" else (1 if enable else 0))))

    def info(self):
        na, nl, bp, ns, nt = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int(), C.c_int()
        _capi.check(self._lib.gp_sparse_system_info(self._h, C.byref(na), C.byref(nl), C.byref(bp), C.byref(ns), C.byref(nt)), "gp_sparse_system_info")
        return dict(nnz_a_blocks=na.value, nnz_l_blocks=nl.value, block_products=bp.value, num_subtrees=ns.value, top_columns=nt.value)


class LevenbergMarquardtGraphGPU:
    """The optimizer's trial with the VALUES in device memory (gp_lm_graph_*, csrc/gp_lm.hip): what LevenbergMarquardtOptimizerExt does with its GPU factor set
    per trial (optimizers/levenberg_marquardt_ext.cpp: linearization_hook_->linearize(values) :352-392, buildDampedSystem + solve + retract + linearization_hook_->error(newValues)
    :188-350) as linearize() / try_lambda() / accept(), one wait per trial; optimize() runs the reference's loop over them natively.

    factors: IntegratedVGICPFactorGPU objects; pairs[i] = (target pose, source pose) of factor i, poses 0..num_poses-1; fixed: indices of held poses.
    pose_factors: BetweenFactorPose3 / PriorFactorPose3 objects over the same poses (gp_lm_graph_create_with_pose_factors): their records follow the VGICP ones,
    `factors` may then be empty (a pose graph) and `fixed` may be () (the priors fix the gauge).  values are [num_poses, 4, 4] float64 arrays (rigid).
    corr_factors: IntegratedGICPFactorGPU / IntegratedICPFactorGPU / LOAM factor / IntegratedColoredGICPFactorGPU objects, corr_pairs[i] = (target pose, source pose) of corr_factors[i]
    (gp_lm_graph_create_with_factors): the graph builds and owns a CorrespondenceFactorBatchGPU over them; their records lie between the VGICP ones and the pose
    factors', in the batch's record order (GICP factors first, then ICP, then LOAM, then colored GICP, each in the order given: `corr_order`).  The trials evaluate them on the correspondences
    of the linearisation point, whether or not a linearise at a trial's values was queued ahead (two correspondence sets)."""

    def __init__(self, factors, pairs, num_poses, fixed=(0,), ordering="auto", stream=None, pose_factors=(), corr_factors=(), corr_pairs=()):
        self._lib = _capi.load()
        self.factors = list(factors)  # (kept alive: the batch holds their handles)
        self.pose_factors = list(pose_factors)
        self.corr_factors = list(corr_factors)
        self._corr = None
        self.corr_order = []
        self._stream = stream
        F = len(self.factors)
        self.pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
        if len(self.pairs) != F:
            raise ValueError(f"{F} factors, {len(self.pairs)} pose pairs")
        self.num_poses = int(num_poses)
        held = np.zeros(self.num_poses, dtype=np.uint8)
        held[list(fixed)] = 1
        self._batch, self._h = C.c_void_p(), C.c_void_p()
        cp = np.ascontiguousarray(np.asarray(corr_pairs, dtype=np.int32).reshape(-1, 2))
        if len(cp) != len(self.corr_factors):
            raise ValueError(f"{len(self.corr_factors)} correspondence factors, {len(cp)} pose pairs")
        if self.corr_factors:
            from .features import CorrespondenceFactorBatchGPU

            self._corr = CorrespondenceFactorBatchGPU(self.corr_factors, stream=stream)
            self.corr_order = list(self._corr.order)
            self.corr_pairs = np.ascontiguousarray(cp[self.corr_order])  # in record order
        if F > 0 or not (self.pose_factors or self.corr_factors):
            arr = (C.c_void_p * F)(*[f._h.value for f in self.factors])
            _capi.check(self._lib.gp_vgicp_batch_create(arr, F, stream, C.byref(self._batch)), "gp_vgicp_batch_create")
        else:
            self._batch = None
        try:  # (one create for every mix: it takes a null correspondence batch and zero pose factors)
            _capi.check(self._lib.gp_lm_graph_create_with_factors(self._batch, self.pairs.ctypes.data, self._corr._h if self._corr is not None else None,
                                                                 self.corr_pairs.ctypes.data if self._corr is not None else None,
                                                                 _pose_factor_array(self.pose_factors) if self.pose_factors else None, len(self.pose_factors),
                                                                 self.num_poses, held.ctypes.data, SparseLinearSystemGPU.ORDERINGS[ordering], stream, C.byref(self._h)),
                        "gp_lm_graph_create_with_factors")
        except Exception:
            self.close()
            raise
        self.n = self._lib.gp_lm_graph_num_variables(self._h)
        self._x, self._b, self._c, self._e = np.zeros(self.n), np.zeros(self.n), np.zeros(1), np.zeros(1)
        self._v = np.zeros((self.num_poses, 16))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.gp_lm_graph_destroy(self._h)
            self._h = None
        if getattr(self, "_batch", None):
            self._lib.gp_vgicp_batch_destroy(self._batch)
            self._batch = None
        if getattr(self, "_corr", None) is not None:
            self._corr.close()
            self._corr = None

    __del__ = close

    @staticmethod
    def _to16(values):
        v = np.asarray(values, dtype=np.float64)
        return np.ascontiguousarray(v.transpose(0, 2, 1)).reshape(len(v), 16)

    def set_values(self, values):
        v = self._to16(values)
        if v.shape != (self.num_poses, 16):
            raise ValueError(f"values must be [{self.num_poses}, 4, 4]")
        _capi.check(self._lib.gp_lm_graph_set_values(self._h, v.ctypes.data), "gp_lm_graph_set_values")

    def values(self):
        _capi.check(self._lib.gp_lm_graph_get_values(self._h, self._v.ctypes.data), "gp_lm_graph_get_values")
        return self._v.reshape(self.num_poses, 4, 4).transpose(0, 2, 1).copy()

    def linearize(self):
        """asynchronous: records at the current values stay in HBM"""
        _capi.check(self._lib.gp_lm_graph_linearize(self._h), "gp_lm_graph_linearize")

    def sync(self):
        if self._batch:
            _capi.check(self._lib.gp_vgicp_batch_sync(self._batch), "gp_vgicp_batch_sync")
        elif self._corr is not None:
            _capi.check(self._lib.gp_corr_batch_sync(self._corr._h), "gp_corr_batch_sync")
        else:
            _capi.check(self._lib.gp_stream_synchronize(self._stream), "gp_stream_synchronize")

    def records(self):
        """-> [F + G + P, 122] float64 CUDA tensor: a copy of the records of the last linearise (the VGICP factors', then the correspondence factors' in the
        batch's record order -- corr_factors[corr_order[r]] --, then the pose factors')"""
        import torch

        p = C.c_void_p()
        _capi.check(self._lib.gp_lm_graph_records(self._h, C.byref(p), None), "gp_lm_graph_records")
        self.sync()
        n = (len(self.factors) + len(self.corr_factors) + len(self.pose_factors)) * _capi.LINEARIZED6_DOUBLES
        out = torch.zeros(n, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        _capi.check(self._lib.gp_memcpy_d2d(C.c_void_p(out.data_ptr()), p, 8 * n, None), "gp_memcpy_d2d")
        _capi.check(self._lib.gp_stream_synchronize(None), "gp_stream_synchronize")
        return out.reshape(-1, _capi.LINEARIZED6_DOUBLES)

    def try_lambda(self, lam, diagonal=False, min_diagonal=1e-6, max_diagonal=1e32, want_values=False):
        """-> (dx, b, cost at the linearisation point, cost at the trial values[, trial values]); GPError (code 5) on an indeterminate system.
        The arrays are the object's own buffers: valid until the next call."""
        _capi.check(self._lib.gp_lm_graph_try_lambda(self._h, float(lam), int(bool(diagonal)), float(min_diagonal), float(max_diagonal), self._x.ctypes.data, self._b.ctypes.data,
                                                     self._c.ctypes.data, self._e.ctypes.data, self._v.ctypes.data if want_values else None), "gp_lm_graph_try_lambda")
        out = (self._x, self._b, float(self._c[0]), float(self._e[0]))
        return out + (self._v.reshape(self.num_poses, 4, 4).transpose(0, 2, 1).copy(),) if want_values else out

    def accept(self):
        _capi.check(self._lib.gp_lm_graph_accept(self._h), "gp_lm_graph_accept")

    def set_one_launch(self, enable=True):
        """the graph's own damped system: False = its multi-launch step with the retract as a kernel of its own behind it (same bits) -> what the next trial runs"""
        return int(self._lib.gp_lm_graph_set_one_launch(self._h, int(bool(enable))))

    def set_speculation(self, enable):
        """queue the linearise at the trial values behind each trial (default on; same results either way) -> previous setting"""
        return bool(self._lib.gp_lm_graph_set_speculation(self._h, int(bool(enable))))

    def optimize(self, values=None, **params):
        """the reference's loop, natively; params: fields of gp_lm_params (GTSAM's defaults otherwise).  -> (values, summary dict)"""
        if values is not None:
            self.set_values(values)
        p, s = _capi.LmParams(), _capi.LmSummary()
        self._lib.gp_lm_params_default(C.byref(p))
        for k, v in params.items():
            if not hasattr(p, k):
                raise TypeError(f"unknown parameter {k}")
            setattr(p, k, v)
        _capi.check(self._lib.gp_lm_graph_optimize(self._h, C.byref(p), C.byref(s)), "gp_lm_graph_optimize")
        return self.values(), {k: getattr(s, k) for k, _ in s._fields_ if k != "reserved_"}

"""Global registration on the device, over the C-ABI (csrc/gp_occupancy.hip, csrc/gp_feature_match.hip, csrc/gp_registration.hip, csrc/gp_gnc.hip):

  OccupancyGridGPU           <- ann/fast_occupancy_grid.hpp:51-113 FastOccupancyGrid
  match_features_gpu         <- the 1-NN feature search estimate_pose_ransac runs on its target_features_tree (registration/impl/ransac_impl.hpp:62)
  estimate_pose_ransac_gpu   <- registration/ransac.hpp:41-48 estimate_pose_ransac (impl/ransac_impl.hpp:24-191)
  align_points_se3_gpu       <- registration/alignment.hpp, the weighted N-point overload (alignment.cpp:67-102)
  align_points_4dof_gpu      <- ... (alignment.cpp:104-139)
  estimate_pose_gnc_gpu      <- registration/graduated_non_convexity.hpp:49-58 estimate_pose_gnc (impl/graduated_non_convexity_impl.hpp:13-201), with its stages alone:
  find_feature_correspondences_gpu  (impl :27-131: reciprocal matches, tuple test)   gnc_align_correspondences_gpu  (impl :133-198: the loop, one launch)

CPU-only upstream; these are device counterparts, not ports (include/gtsam_points_hip.h states what is and is not reproduced: the occupancy SET and every
per-hypothesis rule are the reference's, the random numbers and the order in which hypotheses compete are this library's own and deterministic).
"""
import ctypes as C
import math
from dataclasses import dataclass, field

import numpy as np

from . import _capi
from .types import GaussianVoxelMapGPU, PointCloudGPU, _pose16

STATUS_NAMES = ("SCORED", "SAMPLE_FAILED", "INVALID_FEATURE", "POLY_REJECTED", "TABOO", "SKIPPED")


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def _points(frame, what):
    if frame.points_gpu is None:
        raise _capi.GPError(f"{what}: the frame has no points on the device")
    GaussianVoxelMapGPU._sync_torch(frame)
    return frame.points_gpu, frame.size()


class OccupancyGridGPU:
    """FastOccupancyGrid on the device: the set of cells fast_floor((pose * p) / resolution) of every point inserted, kept in blocks of 8 x 8 x 8 cells.  As a set it is
    exact (the reference's hash table gives up after 10 probes and rehashes; this one's probe loops are bounded by the table size and its table is sized from the
    point count).  Coordinates beyond +-2^20 blocks alias, as in the reference; a point with a non-finite coordinate has no cell."""

    def __init__(self, resolution, stream=None):
        self._lib = _capi.load()
        self._h = None
        self.resolution = float(resolution)
        self.stream = stream
        h = C.c_void_p()
        _capi.check(self._lib.gp_occupancy_grid_create(self.resolution, stream, C.byref(h)), "gp_occupancy_grid_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.gp_occupancy_grid_destroy(self._h)
            self._h = None

    __del__ = close

    def insert(self, frame: PointCloudGPU, pose=None):
        """insert(points, pose): adds the cells of pose * p; any number of calls, the result is the union"""
        pts, n = _points(frame, "OccupancyGridGPU.insert")
        _capi.check(self._lib.gp_occupancy_grid_insert(self._h, _ptr(pts), n, None if pose is None else _pose16(pose)), "gp_occupancy_grid_insert")
        return self

    def calc_overlap(self, frame: PointCloudGPU, pose=None):
        """the number of points of the frame whose cell, at `pose`, is occupied"""
        pts, n = _points(frame, "OccupancyGridGPU.calc_overlap")
        out = C.c_int(0)
        _capi.check(self._lib.gp_occupancy_grid_overlap(self._h, _ptr(pts), n, None if pose is None else _pose16(pose), C.byref(out)), "gp_occupancy_grid_overlap")
        return out.value

    def calc_overlap_rate(self, frame: PointCloudGPU, pose=None):
        return self.calc_overlap(frame, pose) / float(frame.size())

    def get_overlaps(self, frame: PointCloudGPU, pose=None):
        """uint8 device tensor [N]: 1 where the point's cell is occupied"""
        import torch

        pts, n = _points(frame, "OccupancyGridGPU.get_overlaps")
        out = torch.empty(n, dtype=torch.uint8, device=frame.device)
        torch.cuda.current_stream(frame.device).synchronize()
        _capi.check(self._lib.gp_occupancy_grid_get_overlaps(self._h, _ptr(pts), n, None if pose is None else _pose16(pose), _ptr(out)), "gp_occupancy_grid_get_overlaps")
        _capi.check(self._lib.gp_stream_synchronize(self.stream), "gp_stream_synchronize")
        return out

    def calc_overlap_batch(self, frame: PointCloudGPU, poses, sync=True):
        """int32 device tensor [H]: calc_overlap(frame, poses[h]) for every pose, in one launch (RANSAC's scoring kernel).  poses: (H, 4, 4) numpy array, or a float64
        device tensor (H, 16) of column-major poses that is used as it is."""
        import torch

        pts, n = _points(frame, "OccupancyGridGPU.calc_overlap_batch")
        if isinstance(poses, torch.Tensor):
            p = poses.to(device=frame.device, dtype=torch.float64).reshape(-1, 16).contiguous()
        else:
            a = np.asarray(poses, np.float64).reshape(-1, 4, 4)
            p = torch.from_numpy(np.ascontiguousarray(a.transpose(0, 2, 1)).reshape(-1, 16)).to(frame.device)
        h = int(p.shape[0])
        out = torch.empty(h, dtype=torch.int32, device=frame.device)
        torch.cuda.current_stream(frame.device).synchronize()
        _capi.check(self._lib.gp_occupancy_grid_overlap_batch(self._h, _ptr(pts), n, _ptr(p), h, _ptr(out)), "gp_occupancy_grid_overlap_batch")
        if sync:
            _capi.check(self._lib.gp_stream_synchronize(self.stream), "gp_stream_synchronize")
        return out

    def num_occupied_cells(self):
        return int(self._lib.gp_occupancy_grid_num_occupied_cells(self._h))

    def table_info(self):
        """(slots of the hash table, occupied blocks)"""
        s, b = C.c_int(0), C.c_int(0)
        _capi.check(self._lib.gp_occupancy_grid_info(self._h, C.byref(s), C.byref(b)), "gp_occupancy_grid_info")
        return s.value, b.value


def _features(f, device, what):
    """float32 [N][D] row-major on the device"""
    import torch

    t = f if isinstance(f, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(f), dtype=np.float32))
    if t.dim() != 2:
        raise _capi.GPError(f"{what}: features must be [N][D]")
    return t.to(device=device, dtype=torch.float32).contiguous()


def match_features_gpu(target_features, source_features, rows=None, device="cuda:0", stream=None):
    """The exact nearest target row of each query row: (int32 [nq] indices, float64 [nq] squared distances), device tensors.  Brute force over the D-dimensional rows
    (1 <= D <= 128), the distance the direct sum of squared differences in f64.  rows: optional source row indices (the queries); without it every source row is a
    query.  Among target rows at exactly the same distance the lowest index is returned."""
    import torch

    dev = target_features.device if isinstance(target_features, torch.Tensor) and target_features.is_cuda else torch.device(device)
    tf = _features(target_features, dev, "match_features_gpu")
    sf = _features(source_features, dev, "match_features_gpu")
    d = int(tf.shape[1])
    if int(sf.shape[1]) != d:
        raise _capi.GPError(f"match_features_gpu: target features have {d} dimensions, source features {int(sf.shape[1])}")
    if d < 1 or d > _capi.GP_FEATURE_MAX_DIM:
        raise _capi.GPError(f"match_features_gpu: D = {d} is outside 1 .. {_capi.GP_FEATURE_MAX_DIM}")
    if int(tf.shape[0]) < 1:
        raise _capi.GPError("match_features_gpu: no target features")
    ns = int(sf.shape[0])
    r = None
    nq = ns
    if rows is not None:
        r = torch.as_tensor(rows).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
        nq = int(r.shape[0])
        if nq and (ns == 0 or int(r.min()) < 0 or int(r.max()) >= ns):
            raise IndexError("match_features_gpu: row index out of range")
    idx = torch.empty(nq, dtype=torch.int32, device=dev)
    sq = torch.empty(nq, dtype=torch.float64, device=dev)
    lib = _capi.load()
    torch.cuda.current_stream(dev).synchronize()
    _capi.check(lib.gp_feature_nn_search(_ptr(tf), int(tf.shape[0]), _ptr(sf), ns, d, _ptr(r), nq, _ptr(idx), _ptr(sq), stream), "gp_feature_nn_search")
    _capi.check(lib.gp_stream_synchronize(stream), "gp_stream_synchronize")
    return idx, sq


@dataclass
class RANSACParams:
    """RANSACParams (registration/ransac.hpp:17-29) with the reference's defaults; num_threads has no meaning here, chunk_iterations is new: iterations are processed in
    chunks of this many in order, and the early stop takes effect between chunks."""

    max_iterations: int = 5000
    early_stop_inlier_rate: float = 0.8
    poly_error_thresh: float = 0.5
    inlier_voxel_resolution: float = 1.0
    dof: int = 6
    seed: int = 5489
    taboo_thresh_rot: float = 0.5 * math.pi / 180.0
    taboo_thresh_trans: float = 0.25
    taboo_list: list = field(default_factory=list)
    chunk_iterations: int = 1024


@dataclass
class RegistrationResult:
    """RegistrationResult (registration/registration_result.hpp): inlier_rate and T_target_source (4x4); the fields behind them are this library's"""

    inlier_rate: float
    T_target_source: np.ndarray
    best_iteration: int = -1
    best_inliers: int = 0
    num_scored: int = 0
    early_stopped: bool = False
    num_initial: int = 0  # (these five: estimate_pose_gnc_gpu's)
    num_correspondences: int = 0
    num_alignments: int = 0
    final_mu: float = 0.0
    swapped: bool = False


@dataclass
class RANSACHypotheses:
    """per-iteration device arrays: status int32 [H] (STATUS_NAMES), source_indices / target_indices int32 [H][3] (-1 where not drawn / matched), poses float64 [H][16]
    column-major (zeros before the alignment), inliers int32 [H] (-1 where not scored)"""

    status: object
    source_indices: object
    target_indices: object
    poses: object
    inliers: object


def estimate_pose_ransac_gpu(target: PointCloudGPU, source: PointCloudGPU, target_features, source_features, params: RANSACParams = None, sample_indices=None,
                             return_hypotheses=False, stream=None):
    """estimate_pose_ransac: T_target_source from feature matches.  Each iteration samples 3 (dof 6) or 2 (dof 4) source points, matches their feature rows among the
    target's, rejects the sample by the polygon rule, aligns it in closed form, rejects poses on the taboo list and counts the source points that fall into occupied
    cells of the target at inlier_voxel_resolution.  The result is the scored hypothesis with the most inliers (ties: the lowest iteration); the same seed gives the
    same result on every run.  inlier_rate = best_inliers / size(TARGET): the reference's own denominator (ransac_impl.hpp:190), although the early stop compares
    with size(source).  The reference's target_tree argument is unused there (:29) and has no counterpart.
    Features: torch device tensors or numpy arrays [N][D], 1 <= D <= 128.  sample_indices: optional (max_iterations, 3) source indices used instead of the generator.
    return_hypotheses: also return RANSACHypotheses."""
    import torch

    params = params if params is not None else RANSACParams()
    lib = _capi.load()
    what = "estimate_pose_ransac_gpu"
    if params.dof not in (4, 6):
        raise _capi.GPError(f"{what}: dof must be 6 or 4, not {params.dof}")
    samples = 3 if params.dof == 6 else 2
    tp, nt = _points(target, what)
    sp, ns = _points(source, what)
    if nt < 1:
        raise _capi.GPError(f"{what}: the target is empty")
    if ns < samples:
        raise _capi.GPError(f"{what}: {ns} source points, {samples} samples are needed")
    dev = target.device
    tf = _features(target_features, dev, what)
    sf = _features(source_features, dev, what)
    d = int(tf.shape[1])
    if int(sf.shape[1]) != d:
        raise _capi.GPError(f"{what}: target features have {d} dimensions, source features {int(sf.shape[1])}")
    if d < 1 or d > _capi.GP_FEATURE_MAX_DIM:
        raise _capi.GPError(f"{what}: D = {d} is outside 1 .. {_capi.GP_FEATURE_MAX_DIM}")
    if int(tf.shape[0]) != nt or int(sf.shape[0]) != ns:
        raise _capi.GPError(f"{what}: one feature row per point is expected ({int(tf.shape[0])} / {nt} target, {int(sf.shape[0])} / {ns} source)")
    taboo = [np.asarray(T, np.float64).reshape(4, 4) for T in params.taboo_list]
    if len(taboo) > _capi.GP_RANSAC_MAX_TABOO:
        raise _capi.GPError(f"{what}: {len(taboo)} taboo poses, at most {_capi.GP_RANSAC_MAX_TABOO}")
    h = int(params.max_iterations)
    if h < 1 or int(params.chunk_iterations) < 1:
        raise _capi.GPError(f"{what}: max_iterations and chunk_iterations must be positive")
    given = None
    if sample_indices is not None:
        given = torch.as_tensor(sample_indices).to(device=dev, dtype=torch.int32).reshape(h, -1)
        if int(given.shape[1]) < samples:
            raise _capi.GPError(f"{what}: sample_indices must hold {samples} indices per iteration")
        if int(given.shape[1]) < 3:
            given = torch.cat([given, torch.full((h, 3 - int(given.shape[1])), -1, dtype=torch.int32, device=dev)], dim=1)
        given = given[:, :3].contiguous()
        used = given[:, :samples]
        if int(used.min()) < 0 or int(used.max()) >= ns:
            raise IndexError(f"{what}: sample index out of range")
    taboo_flat = np.ascontiguousarray(np.stack([T.T for T in taboo]).reshape(-1)) if taboo else None
    p = _capi.RansacParams(h, int(params.dof), int(params.chunk_iterations), len(taboo), float(params.early_stop_inlier_rate), float(params.poly_error_thresh),
                           float(params.inlier_voxel_resolution), float(params.taboo_thresh_rot), float(params.taboo_thresh_trans), int(params.seed) & 0xFFFFFFFFFFFFFFFF,
                           taboo_flat.ctypes.data if taboo else None)
    hyp = None
    arrays = None
    if return_hypotheses:
        hyp = RANSACHypotheses(torch.empty(h, dtype=torch.int32, device=dev), torch.empty((h, 3), dtype=torch.int32, device=dev),
                               torch.empty((h, 3), dtype=torch.int32, device=dev), torch.empty((h, 16), dtype=torch.float64, device=dev),
                               torch.empty(h, dtype=torch.int32, device=dev))
        arrays = _capi.RansacHypotheses(hyp.status.data_ptr(), hyp.source_indices.data_ptr(), hyp.target_indices.data_ptr(), hyp.poses.data_ptr(), hyp.inliers.data_ptr())
    res = _capi.RansacResult()
    torch.cuda.current_stream(dev).synchronize()
    _capi.check(lib.gp_ransac_estimate_pose(_ptr(tp), nt, _ptr(sp), ns, _ptr(tf), _ptr(sf), d, C.byref(p), _ptr(given), C.byref(arrays) if arrays is not None else None,
                                            C.byref(res), stream), "gp_ransac_estimate_pose")
    T = np.array(list(res.T_target_source), np.float64).reshape(4, 4).T.copy()
    out = RegistrationResult(float(res.inlier_rate), T, int(res.best_iteration), int(res.best_inliers), int(res.num_scored), bool(res.early_stopped))
    return (out, hyp) if return_hypotheses else out


def _align(target_points, source_points, weights, dof, device, stream):
    import torch

    def dev_points(a):
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))
        if t.dim() != 2 or int(t.shape[1]) not in (3, 4):
            raise _capi.GPError("align_points: points must be (N, 3) or (N, 4)")
        return t[:, :3].to(device=device, dtype=torch.float64).contiguous()

    t, s = dev_points(target_points), dev_points(source_points)
    n = int(t.shape[0])
    if n < 1 or int(s.shape[0]) != n:
        raise _capi.GPError(f"align_points: {n} target points, {int(s.shape[0])} source points")
    if weights is None:
        w = torch.ones(n, dtype=torch.float64, device=t.device)
    else:
        w = (weights if isinstance(weights, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(weights, np.float64)))).to(device=t.device, dtype=torch.float64)
        w = w.reshape(-1).contiguous()
        if int(w.shape[0]) != n:
            raise _capi.GPError(f"align_points: {int(w.shape[0])} weights for {n} points")
    out = (C.c_double * 16)()
    torch.cuda.current_stream(t.device).synchronize()
    _capi.check(_capi.load().gp_align_points(_ptr(t), _ptr(s), _ptr(w), n, dof, out, stream), "gp_align_points")
    return np.array(list(out), np.float64).reshape(4, 4).T.copy()


def align_points_se3_gpu(target_points, source_points, weights=None, device="cuda:0", stream=None):
    """align_points_se3(target, source, weights, N) (alignment.cpp:67-102): the 4x4 T minimising sum w |t - T s|^2 over SE(3), from the SVD of the weighted
    cross-covariance with the reference's det(U) det(V) < 0 flip.  Points (N, 3) or (N, 4), numpy or torch; computed in f64 on the device."""
    return _align(target_points, source_points, weights, 6, device, stream)


def align_points_4dof_gpu(target_points, source_points, weights=None, device="cuda:0", stream=None):
    """align_points_4dof (alignment.cpp:104-139): translation and a rotation about z only, from the 2x2 block of the weighted cross-covariance"""
    return _align(target_points, source_points, weights, 4, device, stream)


@dataclass
class GNCParams:
    """GNCParams (registration/graduated_non_convexity.hpp:16-36) with the reference's defaults.  inner_iterations is the reference's `innter_iterations`; its num_threads
    and verbose have no meaning here (return_trace gives what verbose prints)."""

    max_init_samples: int = 5000
    reciprocal_check: bool = True
    tuple_check: bool = False
    tuple_thresh: float = 0.9
    max_num_tuples: int = 1000
    div_factor: float = 1.4
    max_corr_dist: float = 0.25
    inner_iterations: int = 3
    max_iterations: int = 64
    dof: int = 6
    seed: int = 5489


@dataclass
class GNCTrace:
    """one row per alignment, device tensors of num_alignments rows: mu float64, sum_weights float64, sum_errors float64, num_inliers int32 (all at the pose before the
    alignment), poses float64 [.][16] column-major (the pose after it)"""

    mu: object
    sum_weights: object
    sum_errors: object
    num_inliers: object
    poses: object


def _gnc_params(params, what, matching=True, loop=True):
    p = params if params is not None else GNCParams()
    if loop and p.dof not in (4, 6):
        raise _capi.GPError(f"{what}: dof must be 6 or 4, not {p.dof}")
    if matching and int(p.max_init_samples) < 1:
        raise _capi.GPError(f"{what}: max_init_samples must be positive")
    if matching and p.tuple_check and int(p.max_num_tuples) < 1:
        raise _capi.GPError(f"{what}: max_num_tuples must be positive with tuple_check")
    if loop and (not float(p.div_factor) > 1.0 or not float(p.max_corr_dist) > 0.0 or int(p.max_iterations) < 1 or int(p.inner_iterations) < 1):
        raise _capi.GPError(f"{what}: div_factor must be above 1, max_corr_dist, max_iterations and inner_iterations positive")
    c = _capi.GncParams(int(p.max_init_samples), int(bool(p.reciprocal_check)), int(bool(p.tuple_check)), int(p.max_num_tuples), float(p.tuple_thresh), float(p.div_factor),
                        float(p.max_corr_dist), int(p.inner_iterations), int(p.max_iterations), int(p.dof), 0, int(p.seed) & 0xFFFFFFFFFFFFFFFF)
    return p, c


def _gnc_matching_inputs(target, source, target_features, source_features, params, query_indices, what):
    """(tp, nt, sp, ns, tf, sf, d, query tensor or None, number of queries)"""
    import torch

    tp, nt = _points(target, what)
    sp, ns = _points(source, what)
    if nt < 1 or ns < 1:
        raise _capi.GPError(f"{what}: an empty cloud")
    dev = target.device
    tf = _features(target_features, dev, what)
    sf = _features(source_features, dev, what)
    d = int(tf.shape[1])
    if int(sf.shape[1]) != d:
        raise _capi.GPError(f"{what}: target features have {d} dimensions, source features {int(sf.shape[1])}")
    if d < 1 or d > _capi.GP_FEATURE_MAX_DIM:
        raise _capi.GPError(f"{what}: D = {d} is outside 1 .. {_capi.GP_FEATURE_MAX_DIM}")
    if int(tf.shape[0]) != nt or int(sf.shape[0]) != ns:
        raise _capi.GPError(f"{what}: one feature row per point is expected ({int(tf.shape[0])} / {nt} target, {int(sf.shape[0])} / {ns} source)")
    nq = ns if ns < nt else nt  # the smaller cloud queries
    q = None
    k = min(nq, int(params.max_init_samples))
    if query_indices is not None:
        q = torch.as_tensor(query_indices).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
        k = int(q.shape[0])
        if k and (int(q.min()) < 0 or int(q.max()) >= nq):
            raise IndexError(f"{what}: query index out of range")
        if k > 1 and not bool((q[1:] > q[:-1]).all()):
            raise _capi.GPError(f"{what}: query_indices must be ascending and distinct")
    return tp, nt, sp, ns, tf, sf, d, q, k


def _gnc_trace(params, return_trace, dev):
    import torch

    if not return_trace:
        return None, None
    rows = int(params.max_iterations) * int(params.inner_iterations)
    tr = GNCTrace(torch.zeros(rows, dtype=torch.float64, device=dev), torch.zeros(rows, dtype=torch.float64, device=dev), torch.zeros(rows, dtype=torch.float64, device=dev),
                  torch.zeros(rows, dtype=torch.int32, device=dev), torch.zeros((rows, 16), dtype=torch.float64, device=dev))
    return tr, _capi.GncTrace(tr.mu.data_ptr(), tr.sum_weights.data_ptr(), tr.sum_errors.data_ptr(), tr.num_inliers.data_ptr(), tr.poses.data_ptr())


def _gnc_result(res, tr):
    T = np.array(list(res.T_target_source), np.float64).reshape(4, 4).T.copy()
    out = RegistrationResult(float(res.inlier_rate), T, num_initial=int(res.num_initial), num_correspondences=int(res.num_correspondences),
                             num_alignments=int(res.num_alignments), final_mu=float(res.final_mu), swapped=bool(res.swapped))
    if tr is not None:
        n = out.num_alignments
        tr = GNCTrace(tr.mu[:n], tr.sum_weights[:n], tr.sum_errors[:n], tr.num_inliers[:n], tr.poses[:n])
    return out, tr


def find_feature_correspondences_gpu(target: PointCloudGPU, source: PointCloudGPU, target_features, source_features, params: GNCParams = None, query_indices=None, stream=None):
    """The correspondences estimate_pose_gnc starts from (impl :27-131): int32 [M][2] device tensor of (target index, source index).  The smaller cloud queries (the
    source when size(source) < size(target), otherwise the target, the pairs swapped back); more than max_init_samples query rows are subsampled by the library's
    stratified rule (include/gtsam_points_hip.h), or query_indices (ascending, distinct, inside the query cloud) are taken instead; with reciprocal_check a pair is kept
    only when the match's own nearest row is the query; with tuple_check and more than 3 max_num_tuples pairs the tuple test follows.  Deterministic for a seed."""
    import torch

    what = "find_feature_correspondences_gpu"
    params, p = _gnc_params(params, what, loop=False)
    tp, nt, sp, ns, tf, sf, d, q, k = _gnc_matching_inputs(target, source, target_features, source_features, params, query_indices, what)
    pairs = torch.empty((max(k, 1), 2), dtype=torch.int32, device=target.device)
    m, initial, swapped = C.c_int(0), C.c_int(0), C.c_int(0)
    torch.cuda.current_stream(target.device).synchronize()
    _capi.check(_capi.load().gp_feature_correspondences(_ptr(tp), nt, _ptr(sp), ns, _ptr(tf), _ptr(sf), d, C.byref(p), C.c_void_p(q.data_ptr()) if q is not None else None, k,
                                                        C.c_void_p(pairs.data_ptr()), C.byref(m), C.byref(initial), C.byref(swapped), stream), "gp_feature_correspondences")
    return pairs[: m.value]


def gnc_align_correspondences_gpu(target: PointCloudGPU, source: PointCloudGPU, pairs, params: GNCParams = None, return_trace=False, stream=None):
    """The graduated non-convexity loop alone (impl :133-198) on given (target index, source index) pairs, [M][2]: one launch of one workgroup, one wait.  Returns
    RegistrationResult (and GNCTrace with return_trace).  No pairs: the identity, inlier_rate 0, num_alignments 0."""
    import torch

    what = "gnc_align_correspondences_gpu"
    params, p = _gnc_params(params, what, matching=False)
    tp, nt = _points(target, what)
    sp, ns = _points(source, what)
    if nt < 1 or ns < 1:
        raise _capi.GPError(f"{what}: an empty cloud")
    dev = target.device
    pr = torch.as_tensor(pairs).to(device=dev, dtype=torch.int32).reshape(-1, 2).contiguous()
    m = int(pr.shape[0])
    if m and (int(pr.min()) < 0 or int(pr[:, 0].max()) >= nt or int(pr[:, 1].max()) >= ns):
        raise IndexError(f"{what}: pair index out of range")
    tr, ctr = _gnc_trace(params, return_trace, dev)
    res = _capi.GncResult()
    torch.cuda.current_stream(dev).synchronize()
    _capi.check(_capi.load().gp_gnc_align_correspondences(_ptr(tp), nt, _ptr(sp), ns, _ptr(pr), m, C.byref(p), C.byref(ctr) if ctr is not None else None, C.byref(res), stream),
                "gp_gnc_align_correspondences")
    out, tr = _gnc_result(res, tr)
    return (out, tr) if return_trace else out


def estimate_pose_gnc_gpu(target: PointCloudGPU, source: PointCloudGPU, target_features, source_features, params: GNCParams = None, query_indices=None, return_trace=False,
                          return_pairs=False, stream=None):
    """estimate_pose_gnc (Zhou et al., Fast Global Registration): T_target_source from feature matches -- find_feature_correspondences_gpu, then
    gnc_align_correspondences_gpu on its pairs, in one call.  Features: torch device tensors or numpy arrays [N][D], 1 <= D <= 128.  The reference's three tree
    arguments have no counterpart (its target tree is unused there too).  inlier_rate is the share of pairs with |t - T s| < 2 max_corr_dist at the pose BEFORE the last
    alignment, as in the reference (:187).  return_trace / return_pairs: also GNCTrace / the int32 [M][2] pairs, in this order."""
    import torch

    what = "estimate_pose_gnc_gpu"
    params, p = _gnc_params(params, what)
    tp, nt, sp, ns, tf, sf, d, q, k = _gnc_matching_inputs(target, source, target_features, source_features, params, query_indices, what)
    dev = target.device
    pairs = torch.empty((max(k, 1), 2), dtype=torch.int32, device=dev) if return_pairs else None
    tr, ctr = _gnc_trace(params, return_trace, dev)
    res = _capi.GncResult()
    torch.cuda.current_stream(dev).synchronize()
    _capi.check(_capi.load().gp_gnc_estimate_pose(_ptr(tp), nt, _ptr(sp), ns, _ptr(tf), _ptr(sf), d, C.byref(p), C.c_void_p(q.data_ptr()) if q is not None else None, k,
                                                  C.c_void_p(pairs.data_ptr()) if pairs is not None else None, C.byref(ctr) if ctr is not None else None, C.byref(res), stream),
                "gp_gnc_estimate_pose")
    out, tr = _gnc_result(res, tr)
    extra = ([tr] if return_trace else []) + ([pairs[: out.num_correspondences]] if return_pairs else [])
    return (out, *extra) if extra else out

"""GPU counterparts of the CPU-only pieces BASELINE.json configs[4] names, over the C-ABI:

  KdTreeGPU                 <- ann/kdtree.hpp / small_kdtree.hpp (exact k-NN; here a cell-sorted point grid)
  estimate_covariances_gpu  <- features/covariance_estimation.hpp:estimate_covariances(points, k=10)
  estimate_normals_gpu      <- features/normal_estimation.hpp:estimate_normals(points, k=10); estimate_normals_covariances_gpu: both from one search
  IntegratedGICPFactorGPU   <- factors/integrated_gicp_factor.hpp (CPU-only upstream), same calc_delta / HessianFactor protocol
  IntegratedICPFactorGPU    <- factors/integrated_icp_factor.hpp (point-to-point / point-to-plane; CPU-only upstream), on a shared KdTreeGPU
  IntegratedPointToEdgeFactorGPU / IntegratedPointToPlaneFactorGPU / IntegratedLOAMFactorGPU
                            <- factors/integrated_loam_factor.hpp (CPU-only upstream), on the 2 / 3 nearest points of shared KdTreeGPUs
  estimate_intensity_gradients_gpu  <- factors/intensity_gradients.hpp:IntensityGradients::estimate (CPU-only upstream) -> IntensityGradientsGPU
  IntegratedColoredGICPFactorGPU    <- factors/integrated_colored_gicp_factor.hpp (CPU-only upstream), on a shared KdTreeGPU and the target's intensity gradients
  IntegratedCTICPFactorGPU / IntegratedCTGICPFactorGPU
                            <- factors/integrated_ct_icp_factor.hpp, integrated_ct_gicp_factor.hpp (CPU-only upstream): two pose keys, one pose per time stamp
  CorrespondenceFactorBatchGPU  any number of the factor types above linearised / evaluated together, the poses in device memory (gp_corr_batch_*)
  estimate_fpfh_gpu         <- features/fpfh_estimation.hpp:estimate_fpfh (CPU-only upstream): 33-D descriptors over a fixed-radius search, for registration.py
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _capi
from .factors import HessianFactor, LinearizedSystem6, pose_inverse
from .types import GaussianVoxelMapGPU, PointCloudGPU, _pose16


class KdTreeGPU:
    """Exact nearest-neighbour search structure over a PointCloudGPU (KdTree::knn_search semantics)."""

    def __init__(self, frame: PointCloudGPU, cell_size=0.25, stream=None, structure=0, counters=None):
        """structure: GP_TUNE_KNN_STRUCTURE of this search structure (0 default); counters: torch uint64[8] device tensor of work counters (measurement)"""
        self._lib = _capi.load()
        self.frame = frame
        GaussianVoxelMapGPU._sync_torch(frame)
        h = C.c_void_p()
        _capi.check(self._lib.gp_point_grid_create_ex(frame.ptr(frame.points_gpu), frame.size(), float(cell_size), int(structure),
                                                      C.c_void_p(counters.data_ptr()) if counters is not None else None, stream, C.byref(h)), "gp_point_grid_create_ex")
        self._h = h
        self.stream = stream

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.gp_point_grid_destroy(self._h)
            self._h = None

    def knn_search(self, queries, k, max_sq_dist=np.finfo(np.float64).max):
        """queries: (Q,3) numpy/torch -> (indices (Q,k) int32 with -1 padding, sq_dists (Q,k) float64, num_found (Q,))"""
        import torch

        q = PointCloudGPU(queries, device=self.frame.device)
        idx = torch.empty((q.size(), k), dtype=torch.int32, device=self.frame.device)
        d = torch.empty((q.size(), k), dtype=torch.float64, device=self.frame.device)
        nf = torch.empty(q.size(), dtype=torch.int32, device=self.frame.device)
        torch.cuda.current_stream(self.frame.device).synchronize()
        _capi.check(
            self._lib.gp_knn_search(self._h, q.ptr(q.points_gpu), q.size(), int(k), float(max_sq_dist), C.c_void_p(idx.data_ptr()), C.c_void_p(d.data_ptr()), C.c_void_p(nf.data_ptr()), self.stream),
            "gp_knn_search",
        )
        _capi.check(self._lib.gp_stream_synchronize(self.stream), "sync")
        return idx.cpu().numpy(), d.cpu().numpy(), nf.cpu().numpy()


def estimate_covariances_gpu(frame: PointCloudGPU, k_neighbors=10, cell_size=0.0, stream=None, structure=0, counters=None):
    """estimate_covariances(points, n, k): fills frame.covs_gpu (float [N][9]); returns the number of points with < k neighbours.
    structure / counters: per call, see KdTreeGPU (not part of the reference API)."""
    import torch

    lib = _capi.load()
    covs = torch.empty((frame.size(), 9), dtype=torch.float32, device=frame.device)
    GaussianVoxelMapGPU._sync_torch(frame)
    short = C.c_int(0)
    _capi.check(lib.gp_estimate_covariances_ex(frame.ptr(frame.points_gpu), frame.size(), int(k_neighbors), float(cell_size), C.c_void_p(covs.data_ptr()), C.byref(short),
                                               int(structure), C.c_void_p(counters.data_ptr()) if counters is not None else None, stream), "gp_estimate_covariances_ex")
    # the old covariance tensor goes back to torch's caching allocator, which hands same-size blocks out again: a packed source mirror keyed on its address must
    # not survive it, and factors that cached the pointer must re-read it
    frame._forget_mirrors("covs")
    frame.covs_gpu = covs
    frame._host.pop("covs", None)  # the host copy (if any) described the previous covariances
    frame.generation += 1
    return short.value


def _replace_normals(frame, normals):
    # a new tensor where the old one may be handed out again by torch's caching allocator: factors that cached the pointer re-read it on the generation bump
    # (the packed stream mirror holds points and covariances only, so there is no mirror to forget)
    frame.normals_gpu = normals
    frame._host.pop("normals", None)  # the host copy (if any) described the previous normals
    frame.generation += 1


def estimate_normals_gpu(frame: PointCloudGPU, k_neighbors=10, cell_size=0.0, stream=None):
    """estimate_normals(const PointCloud&, k) (features/normal_estimation.cpp:57-62): fills frame.normals_gpu (float [N][3]).  With frame.covs_gpu present the
    normals are read off those covariances (returns 0); otherwise one k-NN search with the covariances left unwritten (returns the
    number of points with < k neighbours)."""
    import torch

    lib = _capi.load()
    normals = torch.empty((frame.size(), 3), dtype=torch.float32, device=frame.device)
    GaussianVoxelMapGPU._sync_torch(frame)
    short = C.c_int(0)
    if frame.covs_gpu is not None:
        _capi.check(lib.gp_estimate_normals_from_covs(frame.ptr(frame.points_gpu), frame.ptr(frame.covs_gpu), frame.size(), C.c_void_p(normals.data_ptr()), stream),
                    "gp_estimate_normals_from_covs")
        _capi.check(lib.gp_stream_synchronize(stream), "sync")  # (the C entry is asynchronous; the tensor is handed to torch and to factors on other streams)
    else:
        _capi.check(lib.gp_estimate_normals_covariances(frame.ptr(frame.points_gpu), frame.size(), int(k_neighbors), float(cell_size), C.c_void_p(normals.data_ptr()), None,
                                                        C.byref(short), stream), "gp_estimate_normals_covariances")
    _replace_normals(frame, normals)
    return short.value


def estimate_normals_covariances_gpu(frame: PointCloudGPU, k_neighbors=10, cell_size=0.0, stream=None):
    """one k-NN search, both attributes: frame.covs_gpu as estimate_covariances_gpu writes it (bit for bit) and frame.normals_gpu as estimate_normals(points, n, k);
    returns the number of points with < k neighbours."""
    import torch

    lib = _capi.load()
    normals = torch.empty((frame.size(), 3), dtype=torch.float32, device=frame.device)
    covs = torch.empty((frame.size(), 9), dtype=torch.float32, device=frame.device)
    GaussianVoxelMapGPU._sync_torch(frame)
    short = C.c_int(0)
    _capi.check(lib.gp_estimate_normals_covariances(frame.ptr(frame.points_gpu), frame.size(), int(k_neighbors), float(cell_size), C.c_void_p(normals.data_ptr()),
                                                    C.c_void_p(covs.data_ptr()), C.byref(short), stream), "gp_estimate_normals_covariances")
    frame._forget_mirrors("covs")  # as estimate_covariances_gpu: the old covariance block may be handed out again under a live packed mirror
    frame.covs_gpu = covs
    frame._host.pop("covs", None)
    _replace_normals(frame, normals)
    return short.value


@dataclass
class FPFHEstimationParams:
    """FPFHEstimationParams (features/fpfh_estimation.hpp:57-66) with the reference's defaults; num_threads has no meaning here."""

    search_radius: float = 5.0
    max_num_neighbors: int = 10000


def estimate_fpfh_gpu(frame: PointCloudGPU, params: FPFHEstimationParams = None, indices=None, dtype=None, return_spfh=False, stream=None):
    """estimate_fpfh (features/fpfh_estimation.cpp:196-307) on frame.points_gpu and frame.normals_gpu: a device tensor [M][33], one FPFH row per entry of `indices`
    (any order, repeats allowed) or per point.  dtype: torch.float32 (the default: what match_features_gpu, estimate_pose_ransac_gpu and estimate_pose_gnc_gpu take,
    no copy through the host) or torch.float64; the f32 row is the f64 row rounded once.  The neighbourhood is every point strictly within search_radius, the point
    itself included, cut at max_num_neighbors by the library's walk order (include/gtsam_points_hip.h: the one deviation from the reference's kd-tree order).
    return_spfh: also (spfh float64 [N][33], num_neighbors int32 [N], num_truncated: the points whose neighbourhood reached max_num_neighbors)."""
    import torch

    what = "estimate_fpfh_gpu"
    if frame.points_gpu is None or frame.normals_gpu is None:
        raise _capi.GPError(f"{what}: the frame has no points or no normals (estimate_normals_gpu)")
    dtype = torch.float32 if dtype is None else dtype
    if dtype not in (torch.float32, torch.float64):
        raise _capi.GPError(f"{what}: dtype must be torch.float32 or torch.float64")
    p = params if params is not None else FPFHEstimationParams()
    n = frame.size()
    if n < 1:
        raise _capi.GPError(f"{what}: an empty cloud")
    if not (float(p.search_radius) > 0.0 and np.isfinite(float(p.search_radius))) or int(p.max_num_neighbors) < 1:
        raise _capi.GPError(f"{what}: search_radius must be finite and positive, max_num_neighbors positive")
    dev = frame.device
    idx, m = None, n
    if indices is not None:
        idx = torch.as_tensor(indices).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
        m = int(idx.shape[0])
        if m and (int(idx.min()) < 0 or int(idx.max()) >= n):
            raise IndexError(f"{what}: index out of range")
    out = torch.empty((m, _capi.GP_FPFH_DIM), dtype=dtype, device=dev)
    spfh = torch.empty((n, _capi.GP_FPFH_DIM), dtype=torch.float64, device=dev) if return_spfh else None
    num = torch.empty(n, dtype=torch.int32, device=dev) if return_spfh else None
    cut = C.c_int(0)
    if m > 0 or return_spfh:
        cp = _capi.FpfhParams(float(p.search_radius), int(p.max_num_neighbors))
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None  # noqa: E731
        GaussianVoxelMapGPU._sync_torch(frame)
        _capi.check(_capi.load().gp_estimate_fpfh(frame.ptr(frame.points_gpu), frame.ptr(frame.normals_gpu), n, C.byref(cp), ptr(idx), m, ptr(out) if dtype == torch.float64 else None,
                                                  ptr(out) if dtype == torch.float32 else None, ptr(spfh), ptr(num), C.byref(cut), stream), "gp_estimate_fpfh")
    return (out, spfh, num, cut.value) if return_spfh else out


class IntegratedGICPFactorGPU:
    """GICP matching-cost factor on the GPU: 1-NN correspondences within max_correspondence_distance (default 1 m,
    integrated_gicp_factor_impl.hpp:30), then the same residual / Jacobian algebra as VGICP."""

    def __init__(self, target_key, source_key, target: PointCloudGPU, source: PointCloudGPU, max_correspondence_distance=1.0, stream=None, _fixed_target_pose=None,
                 structure=0, counters=None):
        self._lib = _capi.load()
        self.is_binary = _fixed_target_pose is None
        self._keys = [target_key, source_key] if self.is_binary else [source_key]
        self.fixed_target_pose = np.eye(4) if self.is_binary else np.asarray(_fixed_target_pose, dtype=np.float64)
        for fr, what in [(target, "target"), (source, "source")]:
            if fr.points_gpu is None or fr.covs_gpu is None:
                raise _capi.GPError(f"error: {what} frame doesn't have required attributes for gicp")
        self.target, self.source = target, source
        GaussianVoxelMapGPU._sync_torch(source)
        h = C.c_void_p()
        _capi.check(
            self._lib.gp_gicp_factor_create_ex(
                target.ptr(target.points_gpu), target.ptr(target.covs_gpu), target.size(), source.ptr(source.points_gpu), source.ptr(source.covs_gpu), source.size(),
                float(max_correspondence_distance) ** 2, int(structure), C.c_void_p(counters.data_ptr()) if counters is not None else None, stream, C.byref(h),
            ),
            "gp_gicp_factor_create_ex",
        )
        self._h = h
        self.stream = stream
        self.linearization_point = np.eye(4)
        self._num_inliers = 0

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.gp_gicp_factor_destroy(self._h)
            self._h = None

    def keys(self):
        return self._keys

    def calc_delta(self, values):
        if not self.is_binary:
            return pose_inverse(self.fixed_target_pose) @ np.asarray(values[self._keys[0]], dtype=np.float64)
        return pose_inverse(values[self._keys[0]]) @ np.asarray(values[self._keys[1]], dtype=np.float64)

    def linearize_delta(self, delta):
        rec = _capi.Linearized6()
        _capi.check(self._lib.gp_gicp_factor_linearize(self._h, _pose16(delta), C.byref(rec)), "gp_gicp_factor_linearize")
        l = LinearizedSystem6(rec)
        self._num_inliers = l.num_inliers
        self.linearization_point = np.asarray(delta, dtype=np.float64)
        self._linearized = True
        return l

    def linearize(self, values):
        l = self.linearize_delta(self.calc_delta(values))
        if self.is_binary:
            return HessianFactor(self._keys, {(0, 0): l.H_target, (0, 1): l.H_target_source, (1, 1): l.H_source}, [-l.b_target, -l.b_source], l.error)
        return HessianFactor(self._keys, {(0, 0): l.H_source}, [-l.b_source], l.error)

    def error(self, values):
        """evaluate(delta) on the correspondences of the last linearise; without one they are computed at `delta` itself first
        (integrated_gicp_factor_impl.hpp:226-228: update_correspondences(delta) when none are stored)"""
        delta = self.calc_delta(values)
        if not getattr(self, "_linearized", False):
            self.linearization_point = np.asarray(delta, dtype=np.float64)
            self._linearized = True
        out = C.c_double()
        _capi.check(self._lib.gp_gicp_factor_compute_error(self._h, _pose16(self.linearization_point), _pose16(delta), C.byref(out)), "gp_gicp_factor_compute_error")
        return out.value

    def num_inliers(self):
        return self._num_inliers


class IntegratedICPFactorGPU:
    """ICP matching-cost factor on the GPU (IntegratedICPFactor_, impl/integrated_icp_factor_impl.hpp): 1-NN correspondences within max_correspondence_distance
    (default 1 m, :30), point-to-point residuals or, with use_point_to_plane, the reference's element-wise r = n_B o (mu_B - T p) on the target's normals.
    target_tree: a KdTreeGPU over `target` that many factors may share (held by reference, never rebuilt); None builds one and holds it (:47-51)."""

    def __init__(self, target_key, source_key, target: PointCloudGPU, source: PointCloudGPU, target_tree=None, use_point_to_plane=False, max_correspondence_distance=1.0,
                 stream=None, _fixed_target_pose=None):
        self._lib = _capi.load()
        self.is_binary = _fixed_target_pose is None
        self._keys = [target_key, source_key] if self.is_binary else [source_key]
        self.fixed_target_pose = np.eye(4) if self.is_binary else np.asarray(_fixed_target_pose, dtype=np.float64)
        if target.points_gpu is None or (use_point_to_plane and target.normals_gpu is None):
            raise _capi.GPError("error: target frame doesn't have required attributes for icp")
        if source.points_gpu is None:
            raise _capi.GPError("error: source frame doesn't have required attributes for icp")
        self.target, self.source = target, source
        self.use_point_to_plane = bool(use_point_to_plane)
        self.target_tree = target_tree if target_tree is not None else KdTreeGPU(target, stream=stream)
        if self.target_tree.frame.points_gpu is None or self.target_tree.frame.points_gpu.data_ptr() != target.points_gpu.data_ptr():
            raise _capi.GPError("error: target_tree was not built over the target frame's points")
        GaussianVoxelMapGPU._sync_torch(target)
        GaussianVoxelMapGPU._sync_torch(source)
        h = C.c_void_p()
        _capi.check(
            self._lib.gp_icp_factor_create(self.target_tree._h, target.ptr(target.points_gpu), target.ptr(target.normals_gpu) if use_point_to_plane else None, target.size(),
                                           source.ptr(source.points_gpu), source.size(), float(max_correspondence_distance) ** 2, int(self.use_point_to_plane), stream, C.byref(h)),
            "gp_icp_factor_create",
        )
        self._h = h
        self.stream = stream
        self.linearization_point = np.eye(4)
        self._num_inliers = 0

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.gp_icp_factor_destroy(self._h)  # (before the tree it borrows: self.target_tree is still referenced here)
            self._h = None

    def keys(self):
        return self._keys

    def set_correspondence_update_tolerance(self, angle, trans):
        """keep the stored correspondences while a linearisation pose stays within (angle [rad], trans [m]) of the pose they were searched at (:128-141)"""
        _capi.check(self._lib.gp_icp_factor_set_correspondence_update_tolerance(self._h, float(angle), float(trans)), "gp_icp_factor_set_correspondence_update_tolerance")

    def calc_delta(self, values):
        if not self.is_binary:
            return pose_inverse(self.fixed_target_pose) @ np.asarray(values[self._keys[0]], dtype=np.float64)
        return pose_inverse(values[self._keys[0]]) @ np.asarray(values[self._keys[1]], dtype=np.float64)

    def linearize_delta(self, delta):
        rec = _capi.Linearized6()
        _capi.check(self._lib.gp_icp_factor_linearize(self._h, _pose16(delta), C.byref(rec)), "gp_icp_factor_linearize")
        l = LinearizedSystem6(rec)
        self._num_inliers = l.num_inliers
        self.linearization_point = np.asarray(delta, dtype=np.float64)
        self._linearized = True
        return l

    def linearize(self, values):
        l = self.linearize_delta(self.calc_delta(values))
        if self.is_binary:
            return HessianFactor(self._keys, {(0, 0): l.H_target, (0, 1): l.H_target_source, (1, 1): l.H_source}, [-l.b_target, -l.b_source], l.error)
        return HessianFactor(self._keys, {(0, 0): l.H_source}, [-l.b_source], l.error)

    def error(self, values):
        """evaluate(delta) on the stored correspondences; without any they are computed at `delta` itself first (:188-190)"""
        delta = self.calc_delta(values)
        if not getattr(self, "_linearized", False):
            self.linearization_point = np.asarray(delta, dtype=np.float64)
            self._linearized = True
        out = C.c_double()
        _capi.check(self._lib.gp_icp_factor_compute_error(self._h, _pose16(self.linearization_point), _pose16(delta), C.byref(out)), "gp_icp_factor_compute_error")
        return out.value

    def num_inliers(self):
        return self._num_inliers


def IntegratedPointToPlaneICPFactorGPU(target_key, source_key, target, source, target_tree=None, max_correspondence_distance=1.0, stream=None, _fixed_target_pose=None):
    """IntegratedPointToPlaneICPFactor_ (factors/integrated_icp_factor.hpp): the ICP factor with use_point_to_plane = true"""
    return IntegratedICPFactorGPU(target_key, source_key, target, source, target_tree=target_tree, use_point_to_plane=True,
                                  max_correspondence_distance=max_correspondence_distance, stream=stream, _fixed_target_pose=_fixed_target_pose)


class IntensityGradientsGPU:
    """IntensityGradients (factors/intensity_gradients.hpp): per-point intensity gradients in the tangent plane, gradients_gpu float [N][3] on the device"""

    def __init__(self, gradients_gpu, num_short=None):
        self.gradients_gpu = gradients_gpu
        self.num_short = num_short  # points with fewer than k neighbours, when the estimate searched for itself

    def size(self):
        return int(self.gradients_gpu.shape[0])

    def download(self):
        return self.gradients_gpu.cpu().numpy()


def estimate_intensity_gradients_gpu(frame: PointCloudGPU, k_neighbors=10, neighbors=None, k_photo_neighbors=None, cell_size=0.0, stream=None):
    """IntensityGradients::estimate (factors/intensity_gradients.cpp:20-133) -> IntensityGradientsGPU.
    neighbors=None: one k-NN search with k_neighbors (:71-133); points with fewer neighbours get (0, 0, 0) and are counted in the result's num_short.
    neighbors: an (N, k) int table (numpy or a device tensor, -1 where a point has fewer), of which the first k_photo_neighbors slots are used (all by default) (:20-69)."""
    import torch

    if frame.points_gpu is None or frame.normals_gpu is None or frame.intensities_gpu is None:
        raise _capi.GPError("error: input frame doesn't have required attributes for intensity gradient estimation!!")  # :21-24
    lib = _capi.load()
    n = frame.size()
    grads = torch.empty((n, 3), dtype=torch.float32, device=frame.device)
    GaussianVoxelMapGPU._sync_torch(frame)
    args = (frame.ptr(frame.points_gpu), frame.ptr(frame.normals_gpu), frame.ptr(frame.intensities_gpu), n)
    out = IntensityGradientsGPU(grads)
    if n == 0:
        return out
    if neighbors is None:
        short = C.c_int(0)
        _capi.check(lib.gp_estimate_intensity_gradients(*args, int(k_neighbors), float(cell_size), C.c_void_p(grads.data_ptr()), C.byref(short), stream),
                    "gp_estimate_intensity_gradients")
        out.num_short = short.value
        return out
    table = neighbors if isinstance(neighbors, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(neighbors, dtype=np.int32))
    table = table.to(device=frame.device, dtype=torch.int32).reshape(n, -1).contiguous()
    k = int(table.shape[1])
    torch.cuda.current_stream(frame.device).synchronize()  # (the table's upload)
    _capi.check(lib.gp_estimate_intensity_gradients_from_neighbors(*args, C.c_void_p(table.data_ptr()), k, int(k if k_photo_neighbors is None else k_photo_neighbors),
                                                                   C.c_void_p(grads.data_ptr()), stream), "gp_estimate_intensity_gradients_from_neighbors")
    _capi.check(lib.gp_stream_synchronize(stream), "sync")  # (the C entry is asynchronous; the table goes back to torch here)
    return out


class IntegratedColoredGICPFactorGPU:
    """Colored GICP matching-cost factor on the GPU (IntegratedColoredGICPFactor_, impl/integrated_colored_gicp_factor_impl.hpp): GICP's geometric term on the 1-NN
    correspondences within max_correspondence_distance (default 1 m, :28) weighted 1 - photometric_term_weight, plus the photometric residual
    I_B - I_A - (P g_B) . (mu_B - T p_A) in the target's tangent plane weighted photometric_term_weight (default 0.25, :29).
    target_tree: a KdTreeGPU over `target` that many factors may share; None builds one.  target_gradients: an IntensityGradientsGPU of `target`; None estimates
    it with k = 10.  The search is the 3-D one (the reference's optional 4-D IntensityKdTree is not provided)."""

    def __init__(self, target_key, source_key, target: PointCloudGPU, source: PointCloudGPU, target_tree=None, target_gradients=None, max_correspondence_distance=1.0,
                 photometric_term_weight=0.25, stream=None, _fixed_target_pose=None):
        self._lib = _capi.load()
        self.is_binary = _fixed_target_pose is None
        self._keys = [target_key, source_key] if self.is_binary else [source_key]
        self.fixed_target_pose = np.eye(4) if self.is_binary else np.asarray(_fixed_target_pose, dtype=np.float64)
        if target.points_gpu is None or target.covs_gpu is None or target.normals_gpu is None or target.intensities_gpu is None:
            raise _capi.GPError("error: target frame doesn't have required attributes for colored_gicp")  # :37-40
        if source.points_gpu is None or source.covs_gpu is None or source.intensities_gpu is None:
            raise _capi.GPError("error: source frame doesn't have required attributes for colored_gicp")  # :42-45
        self.target, self.source = target, source
        self.target_tree = target_tree if target_tree is not None else KdTreeGPU(target, stream=stream)
        if self.target_tree.frame.points_gpu is None or self.target_tree.frame.points_gpu.data_ptr() != target.points_gpu.data_ptr():
            raise _capi.GPError("error: target_tree was not built over the target frame's points")
        self.target_gradients = target_gradients if target_gradients is not None else estimate_intensity_gradients_gpu(target, 10, stream=stream)
        if self.target_gradients.size() != target.size():
            raise _capi.GPError("error: target_gradients does not have one gradient per target point")
        GaussianVoxelMapGPU._sync_torch(target)
        GaussianVoxelMapGPU._sync_torch(source)
        h = C.c_void_p()
        _capi.check(
            self._lib.gp_colored_gicp_factor_create(self.target_tree._h, target.ptr(target.points_gpu), target.ptr(target.covs_gpu), target.ptr(target.normals_gpu),
                                                    target.ptr(target.intensities_gpu), C.c_void_p(self.target_gradients.gradients_gpu.data_ptr()), target.size(),
                                                    source.ptr(source.points_gpu), source.ptr(source.covs_gpu), source.ptr(source.intensities_gpu), source.size(),
                                                    float(max_correspondence_distance) ** 2, float(photometric_term_weight), stream, C.byref(h)),
            "gp_colored_gicp_factor_create",
        )
        self._h = h
        self.stream = stream
        self.linearization_point = np.eye(4)
        self._num_inliers = 0

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.gp_colored_gicp_factor_destroy(self._h)  # (before the tree and the gradients it borrows: both are still referenced here)
            self._h = None

    def keys(self):
        return self._keys

    def set_photometric_term_weight(self, weight):
        _capi.check(self._lib.gp_colored_gicp_factor_set_photometric_term_weight(self._h, float(weight)), "gp_colored_gicp_factor_set_photometric_term_weight")

    def set_max_correspondence_distance(self, dist):
        _capi.check(self._lib.gp_colored_gicp_factor_set_max_correspondence_distance(self._h, float(dist)), "gp_colored_gicp_factor_set_max_correspondence_distance")

    def set_correspondence_update_tolerance(self, angle, trans):
        """keep the stored correspondences while a linearisation pose stays within (angle [rad], trans [m]) of the pose they were searched at (:101-114)"""
        _capi.check(self._lib.gp_colored_gicp_factor_set_correspondence_update_tolerance(self._h, float(angle), float(trans)),
                    "gp_colored_gicp_factor_set_correspondence_update_tolerance")

    def calc_delta(self, values):
        if not self.is_binary:
            return pose_inverse(self.fixed_target_pose) @ np.asarray(values[self._keys[0]], dtype=np.float64)
        return pose_inverse(values[self._keys[0]]) @ np.asarray(values[self._keys[1]], dtype=np.float64)

    def linearize_delta(self, delta):
        rec = _capi.Linearized6()
        _capi.check(self._lib.gp_colored_gicp_factor_linearize(self._h, _pose16(delta), C.byref(rec)), "gp_colored_gicp_factor_linearize")
        l = LinearizedSystem6(rec)
        self._num_inliers = l.num_inliers
        self.linearization_point = np.asarray(delta, dtype=np.float64)
        self._linearized = True
        return l

    def linearize(self, values):
        l = self.linearize_delta(self.calc_delta(values))
        if self.is_binary:
            return HessianFactor(self._keys, {(0, 0): l.H_target, (0, 1): l.H_target_source, (1, 1): l.H_source}, [-l.b_target, -l.b_source], l.error)
        return HessianFactor(self._keys, {(0, 0): l.H_source}, [-l.b_source], l.error)

    def error(self, values):
        """evaluate(delta) on the stored correspondences; without any they are computed at `delta` itself first (:170-172)"""
        delta = self.calc_delta(values)
        if not getattr(self, "_linearized", False):
            self.linearization_point = np.asarray(delta, dtype=np.float64)
            self._linearized = True
        out = C.c_double()
        _capi.check(self._lib.gp_colored_gicp_factor_compute_error(self._h, _pose16(self.linearization_point), _pose16(delta), C.byref(out)),
                    "gp_colored_gicp_factor_compute_error")
        return out.value

    def num_inliers(self):
        return self._num_inliers


class IntegratedCTICPFactorGPU:
    """Continuous-time ICP factor on the GPU (IntegratedCT_ICPFactor_, impl/integrated_ct_icp_factor_impl.hpp): the source was scanned while the sensor moved from
    the pose of source_t0_key to that of source_t1_key; every point is transformed by the pose interpolated at its own time stamp (source.times_gpu, grouped into
    bins 1e-3 apart, :41-55) and matched to its nearest target point within max_correspondence_distance (default 1 m, :27).  The residual is the scalar
    point-to-plane distance on the target's normals.  target_tree: a KdTreeGPU over `target` that many factors may share; None builds one and holds it (:57-61)."""

    _KIND = 0

    def __init__(self, source_t0_key, source_t1_key, target: PointCloudGPU, source: PointCloudGPU, target_tree=None, max_correspondence_distance=1.0, stream=None):
        self._lib = _capi.load()
        self._keys = [source_t0_key, source_t1_key]
        if target.points_gpu is None:
            raise _capi.GPError("error: target frame doesn't have required attributes for ct_icp")  # :31-34
        if source.points_gpu is None or source.times_gpu is None:
            raise _capi.GPError("error: source frame doesn't have required attributes for ct_icp")  # :36-39
        self._check_attributes(target, source)
        self.target, self.source = target, source
        self.target_tree = target_tree if target_tree is not None else KdTreeGPU(target, stream=stream)
        if self.target_tree.frame.points_gpu is None or self.target_tree.frame.points_gpu.data_ptr() != target.points_gpu.data_ptr():
            raise _capi.GPError("error: target_tree was not built over the target frame's points")
        GaussianVoxelMapGPU._sync_torch(target)
        GaussianVoxelMapGPU._sync_torch(source)
        gicp = self._KIND == 1
        h = C.c_void_p()
        _capi.check(
            self._lib.gp_ct_factor_create(self.target_tree._h, target.ptr(target.points_gpu), None if gicp else target.ptr(target.normals_gpu),
                                          target.ptr(target.covs_gpu) if gicp else None, target.size(), source.ptr(source.points_gpu),
                                          source.ptr(source.covs_gpu) if gicp else None, source.ptr(source.times_gpu), source.size(),
                                          float(max_correspondence_distance) ** 2, self._KIND, stream, C.byref(h)),
            "gp_ct_factor_create",
        )
        self._h = h
        self.stream = stream
        self._num_inliers = 0

    @staticmethod
    def _check_attributes(target, source):
        if target.normals_gpu is None:
            raise _capi.GPError("error: target cloud doesn't have normals!!")  # (the reference aborts with this at the first linearise, :133-136)

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.gp_ct_factor_destroy(self._h)  # (before the tree it borrows: self.target_tree is still referenced here)
            self._h = None

    def keys(self):
        return self._keys

    def _poses(self, values):
        return _pose16(values[self._keys[0]]), _pose16(values[self._keys[1]])

    def linearize(self, values):
        """update_poses + update_correspondences + the sums -> HessianFactor(k0, k1, H_00, H_01, -b_0, H_11, -b_1, error) (:132-199)"""
        rec = _capi.Linearized6()
        _capi.check(self._lib.gp_ct_factor_linearize(self._h, *self._poses(values), C.byref(rec)), "gp_ct_factor_linearize")
        l = LinearizedSystem6(rec)
        self._num_inliers = l.num_inliers
        return HessianFactor(self._keys, {(0, 0): l.H_target, (0, 1): l.H_target_source, (1, 1): l.H_source}, [-l.b_target, -l.b_source], l.error)

    def error(self, values):
        """the error at `values` on the stored correspondences; without any they are searched at `values` first (:92-96)"""
        out = C.c_double()
        _capi.check(self._lib.gp_ct_factor_compute_error(self._h, *self._poses(values), C.byref(out)), "gp_ct_factor_compute_error")
        return out.value

    def num_inliers(self):
        return self._num_inliers

    def time_table(self):
        """(normalised time of every bin float64 [bins], bin of every source point int32 [n])"""
        table = np.zeros(self._lib.gp_ct_factor_num_time_bins(self._h), dtype=np.float64)
        indices = np.zeros(self.source.size(), dtype=np.int32)
        _capi.check(self._lib.gp_ct_factor_time_table(self._h, table.ctypes.data, indices.ctypes.data), "gp_ct_factor_time_table")
        return table, indices

    def pose_table(self):
        """(T [bins, 3, 4], D0 [bins, 6, 6], D1 [bins, 6, 6]) of the last linearise (read-only; for tests and diagnosis)"""
        rows = np.zeros((self._lib.gp_ct_factor_num_time_bins(self._h), 84), dtype=np.float64)
        _capi.check(self._lib.gp_ct_factor_pose_table(self._h, rows.ctypes.data), "gp_ct_factor_pose_table")
        return rows[:, :12].reshape(-1, 3, 4), rows[:, 12:48].reshape(-1, 6, 6), rows[:, 48:].reshape(-1, 6, 6)

    def correspondences(self):
        """the stored correspondences int32 [n], -1 where a point has none (read-only; for tests and diagnosis)"""
        out = np.full(self.source.size(), -1, dtype=np.int32)
        _capi.check(self._lib.gp_ct_factor_correspondences(self._h, out.ctypes.data), "gp_ct_factor_correspondences")
        return out

    def deskewed_source_points(self, values, local=False):
        """T(t_i) p_i -- or T0^-1 T(t_i) p_i when `local` -- as float64 [n, 4], last component 1 (:290-308)"""
        import torch

        out = torch.empty((self.source.size(), 4), dtype=torch.float64, device=self.source.device)
        torch.cuda.current_stream(self.source.device).synchronize()
        _capi.check(self._lib.gp_ct_factor_deskew(self._h, *self._poses(values), int(bool(local)), C.c_void_p(out.data_ptr())), "gp_ct_factor_deskew")
        return out.cpu().numpy()


class IntegratedCTGICPFactorGPU(IntegratedCTICPFactorGPU):
    """Continuous-time GICP factor on the GPU (IntegratedCT_GICPFactor_, impl/integrated_ct_gicp_factor_impl.hpp): the CT-ICP factor with the GICP term
    r^T (C_B + R(t_i) C_A R(t_i)^T)^-1 r, the matrix taken at the poses of the last linearise and kept for error() (:171-200)."""

    _KIND = 1

    @staticmethod
    def _check_attributes(target, source):
        if target.covs_gpu is None:
            raise _capi.GPError("error: target frame doesn't have required attributes for ct_gicp")  # :27-30
        if source.covs_gpu is None:
            raise _capi.GPError("error: source frame doesn't have required attributes for ct_gicp")  # :32-35


class IntegratedLOAMFactorGPU:
    """LOAM matching-cost factor on the GPU (IntegratedLOAMFactor_, impl/integrated_loam_factor_impl.hpp): a point-to-edge part on the 2 nearest edge points and a
    point-to-plane part on the 3 nearest plane points within max_correspondence_distance (default 1 m each), their records added edge first.
    target_edges_tree / target_planes_tree: KdTreeGPUs over the target clouds that many factors may share (held by reference); None builds one and holds it."""

    _LOAM = "error: {} frame doesn't have required attributes for loam"
    _EDGE = "error: target or source points has not been allocated!!"

    def __init__(self, target_key, source_key, target_edges, target_planes, source_edges, source_planes, target_edges_tree=None, target_planes_tree=None,
                 max_correspondence_distance=1.0, stream=None, _fixed_target_pose=None):
        self._lib = _capi.load()
        self.is_binary = _fixed_target_pose is None
        self._keys = [target_key, source_key] if self.is_binary else [source_key]
        self.fixed_target_pose = np.eye(4) if self.is_binary else np.asarray(_fixed_target_pose, dtype=np.float64)
        # the reference constructs the edge factor first (:387-390); each aborts with its own text
        if target_edges is not None and (target_edges.points_gpu is None or source_edges.points_gpu is None):
            raise _capi.GPError(self._EDGE)
        if target_planes is not None:
            if target_planes.points_gpu is None:
                raise _capi.GPError(self._LOAM.format("target"))
            if source_planes.points_gpu is None:
                raise _capi.GPError(self._LOAM.format("source"))
        self.target_edges, self.source_edges, self.target_planes, self.source_planes = target_edges, source_edges, target_planes, source_planes
        self.target_edges_tree = self._tree(target_edges, target_edges_tree, stream)
        self.target_planes_tree = self._tree(target_planes, target_planes_tree, stream)
        args = []
        for tree, tgt, src in [(self.target_edges_tree, target_edges, source_edges), (self.target_planes_tree, target_planes, source_planes)]:
            if tgt is None:
                args += [None, None, 0, None, 0]
                continue
            GaussianVoxelMapGPU._sync_torch(tgt)
            GaussianVoxelMapGPU._sync_torch(src)
            args += [tree._h, tgt.ptr(tgt.points_gpu), tgt.size(), src.ptr(src.points_gpu), src.size()]
        h = C.c_void_p()
        _capi.check(self._lib.gp_loam_factor_create(*args, stream, C.byref(h)), "gp_loam_factor_create")
        self._h = h
        self.stream = stream
        self.linearization_point = np.eye(4)
        self._num_inliers = 0
        if max_correspondence_distance != 1.0:
            self.set_max_correspondence_distance(max_correspondence_distance, max_correspondence_distance)

    @staticmethod
    def _tree(target, tree, stream):
        if target is None:
            return None
        tree = tree if tree is not None else KdTreeGPU(target, stream=stream)
        if tree.frame.points_gpu is None or tree.frame.points_gpu.data_ptr() != target.points_gpu.data_ptr():
            raise _capi.GPError("error: target_tree was not built over the target frame's points")
        return tree

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.gp_loam_factor_destroy(self._h)  # (before the trees it borrows, which are still referenced here)
            self._h = None

    def keys(self):
        return self._keys

    def set_max_correspondence_distance(self, dist_edge, dist_plane):
        _capi.check(self._lib.gp_loam_factor_set_max_correspondence_distance(self._h, float(dist_edge), float(dist_plane)), "gp_loam_factor_set_max_correspondence_distance")

    def set_enable_correspondence_validation(self, enable):
        """validate_correspondences (:487-529): drop edge pairs / plane triples that lie in one scan line (off by default)"""
        _capi.check(self._lib.gp_loam_factor_set_enable_correspondence_validation(self._h, int(bool(enable))), "gp_loam_factor_set_enable_correspondence_validation")

    def set_correspondence_update_tolerance(self, angle, trans):
        _capi.check(self._lib.gp_loam_factor_set_correspondence_update_tolerance(self._h, float(angle), float(trans)), "gp_loam_factor_set_correspondence_update_tolerance")

    calc_delta = IntegratedICPFactorGPU.calc_delta

    def linearize_delta(self, delta):
        rec = _capi.Linearized6()
        _capi.check(self._lib.gp_loam_factor_linearize(self._h, _pose16(delta), C.byref(rec)), "gp_loam_factor_linearize")
        l = LinearizedSystem6(rec)
        self._num_inliers = l.num_inliers
        self.linearization_point = np.asarray(delta, dtype=np.float64)
        self._linearized = True
        return l

    linearize = IntegratedICPFactorGPU.linearize

    def error(self, values):
        """evaluate(delta) on the stored correspondences; without any they are computed at `delta` itself first"""
        delta = self.calc_delta(values)
        if not getattr(self, "_linearized", False):
            self.linearization_point = np.asarray(delta, dtype=np.float64)
            self._linearized = True
        out = C.c_double()
        _capi.check(self._lib.gp_loam_factor_compute_error(self._h, _pose16(self.linearization_point), _pose16(delta), C.byref(out)), "gp_loam_factor_compute_error")
        return out.value

    def num_inliers(self):
        return self._num_inliers

    def num_correspondences(self):
        """(edges, planes) of the last linearise"""
        e, p = C.c_int(0), C.c_int(0)
        _capi.check(self._lib.gp_loam_factor_num_correspondences(self._h, C.byref(e), C.byref(p)), "gp_loam_factor_num_correspondences")
        return e.value, p.value

    def correspondences(self):
        """(edges (n, 2) or None, planes (n, 3) or None): the stored correspondences copied to the host, per source point the target indices in ascending order of
        distance, a row of -1 where the point has none (read-only; for tests and diagnosis)"""
        out = []
        for src, K in ((self.source_edges, 2), (self.source_planes, 3)):
            out.append(None if src is None else np.full((K, src.size()), -1, dtype=np.int32))
        _capi.check(self._lib.gp_loam_factor_get_correspondences(self._h, *[None if a is None else a.ctypes.data for a in out]), "gp_loam_factor_get_correspondences")
        return tuple(None if a is None else np.ascontiguousarray(a.T) for a in out)


class IntegratedPointToEdgeFactorGPU(IntegratedLOAMFactorGPU):
    """IntegratedPointToEdgeFactor_ (:197-372): the LOAM factor's edge part alone.  set_max_correspondence_distance takes (dist_edge, dist_plane) like the combined
    factor; the absent part's value is ignored."""

    def __init__(self, target_key, source_key, target, source, target_tree=None, max_correspondence_distance=1.0, stream=None, _fixed_target_pose=None):
        super().__init__(target_key, source_key, target, None, source, None, target_edges_tree=target_tree, max_correspondence_distance=max_correspondence_distance,
                         stream=stream, _fixed_target_pose=_fixed_target_pose)


class IntegratedPointToPlaneFactorGPU(IntegratedLOAMFactorGPU):
    """IntegratedPointToPlaneFactor_ (:16-194): the LOAM factor's plane part alone."""

    def __init__(self, target_key, source_key, target, source, target_tree=None, max_correspondence_distance=1.0, stream=None, _fixed_target_pose=None):
        super().__init__(target_key, source_key, None, target, None, source, target_planes_tree=target_tree, max_correspondence_distance=max_correspondence_distance,
                         stream=stream, _fixed_target_pose=_fixed_target_pose)


def _poses16(deltas, count):
    d = np.asarray(deltas, dtype=np.float64)
    if d.shape != (count, 4, 4):
        raise ValueError(f"poses must be [{count}, 4, 4]")
    return np.ascontiguousarray(d.transpose(0, 2, 1)).reshape(count, 16)


class CorrespondenceFactorBatchGPU:
    """IntegratedGICPFactorGPU / IntegratedICPFactorGPU / LOAM factor / IntegratedColoredGICPFactorGPU objects linearised and evaluated TOGETHER (gp_corr_batch_*,
    csrc/gp_corr_batch.hip): a number of launches that does not depend on their number, with the relative poses read from device memory.  Record order: the GICP
    factors in the order given, then the ICP factors, then the LOAM factors (edge, plane or combined), then the colored GICP factors (`order`: positions in
    `factors`; the results below are returned in the order of `factors`).
    The batch borrows the factors (kept alive here) and keeps correspondences of its own, in two sets: a linearise searches into the set it names (default 0), an
    error evaluation reads the set it names and never searches.  A record / an error has the bits of the factor's own linearize_delta / error at the same pose(s).
    ICP, LOAM and colored GICP factors with non-zero correspondence-update tolerances are refused.  A LOAM factor's cut-offs and validation switch, and a colored GICP
    factor's photometric_term_weight and max_correspondence_distance, are read here, at creation: a later set_* on the factor does not reach an existing batch."""

    def __init__(self, factors, stream=None):
        self._lib = _capi.load()
        self.factors = list(factors)
        gicp = [i for i, f in enumerate(self.factors) if isinstance(f, IntegratedGICPFactorGPU)]
        icp = [i for i, f in enumerate(self.factors) if isinstance(f, IntegratedICPFactorGPU)]
        loam = [i for i, f in enumerate(self.factors) if isinstance(f, IntegratedLOAMFactorGPU)]
        colored = [i for i, f in enumerate(self.factors) if isinstance(f, IntegratedColoredGICPFactorGPU)]
        if len(gicp) + len(icp) + len(loam) + len(colored) != len(self.factors):
            raise TypeError("CorrespondenceFactorBatchGPU takes IntegratedGICPFactorGPU / IntegratedICPFactorGPU / IntegratedLOAMFactorGPU / IntegratedColoredGICPFactorGPU objects")
        self.order = gicp + icp + loam + colored  # record r is factors[order[r]]
        if stream is None and self.factors:
            stream = self.factors[0].stream  # the stream the factors were created on (the library refuses a batch whose factors live on different streams)
        self._slot = np.argsort(np.asarray(self.order, dtype=np.int64)) if self.factors else np.zeros(0, np.int64)  # factors[i] is record _slot[i]
        self.stream = stream
        ga = (C.c_void_p * max(len(gicp), 1))(*[self.factors[i]._h.value for i in gicp])
        ia = (C.c_void_p * max(len(icp), 1))(*[self.factors[i]._h.value for i in icp])
        la = (C.c_void_p * max(len(loam), 1))(*[self.factors[i]._h.value for i in loam])
        ca = (C.c_void_p * max(len(colored), 1))(*[self.factors[i]._h.value for i in colored])
        h = C.c_void_p()
        _capi.check(self._lib.gp_corr_batch_create_ex2(ga, len(gicp), ia, len(icp), la, len(loam), ca, len(colored), stream, C.byref(h)), "gp_corr_batch_create_ex2")
        self._h = h
        self._dev = None

    def close(self):
        if getattr(self, "_h", None):
            self._lib.gp_corr_batch_destroy(self._h)
            self._h = None

    __del__ = close

    def __len__(self):
        return len(self.factors)

    def _records_order(self, poses):
        return np.ascontiguousarray(_poses16(poses, len(self.factors))[self.order])

    def _upload(self, p16):
        import torch

        t = torch.from_numpy(p16).to("cuda")
        torch.cuda.synchronize()
        return t

    def linearize_deltas(self, deltas, rigid=True, corr_set=None):
        """deltas [F, 4, 4] in the order of `factors` -> [LinearizedSystem6] in that order.  rigid: every 3x3 block is orthonormal to 1e-9 (the 29-sum kernels, what
        the factors' own calls choose for such poses); False: the general kernels.  corr_set: None = the synchronous host-pose call (set 0); 0 / 1 = the device-pose
        entry point into that correspondence set."""
        F = len(self.factors)
        p16 = self._records_order(deltas)
        out = np.zeros((F, _capi.LINEARIZED6_DOUBLES))
        if corr_set is None:
            _capi.check(self._lib.gp_corr_batch_linearize(self._h, p16.ctypes.data, int(bool(rigid)), out.ctypes.data), "gp_corr_batch_linearize")
        else:
            import torch

            poses = self._upload(p16)
            rec = torch.zeros((F, _capi.LINEARIZED6_DOUBLES), dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            _capi.check(self._lib.gp_corr_batch_issue_linearize_dev(self._h, C.c_void_p(poses.data_ptr()), int(bool(rigid)), int(corr_set), C.c_void_p(rec.data_ptr())),
                        "gp_corr_batch_issue_linearize_dev")
            _capi.check(self._lib.gp_corr_batch_sync(self._h), "gp_corr_batch_sync")
            out = rec.cpu().numpy()
        return [LinearizedSystem6.from_doubles(out[self._slot[i]]) for i in range(F)]

    def errors(self, deltas_lin, deltas_eval, corr_set=None):
        """the factors' errors at deltas_eval on the stored correspondences of set `corr_set` (None: the synchronous host-pose call on set 0), deltas_lin being the poses that
        set was linearised at -> float64 [F] in the order of `factors`"""
        F = len(self.factors)
        pl, pe = self._records_order(deltas_lin), self._records_order(deltas_eval)
        out = np.zeros(F)
        if corr_set is None:
            _capi.check(self._lib.gp_corr_batch_compute_error(self._h, pl.ctypes.data, pe.ctypes.data, out.ctypes.data), "gp_corr_batch_compute_error")
        else:
            import torch

            dl, de = self._upload(pl), self._upload(pe)
            err = torch.zeros(F, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            _capi.check(self._lib.gp_corr_batch_issue_compute_error_dev(self._h, int(corr_set), C.c_void_p(dl.data_ptr()), C.c_void_p(de.data_ptr()), C.c_void_p(err.data_ptr()),
                                                                        None, 0), "gp_corr_batch_issue_compute_error_dev")
            _capi.check(self._lib.gp_corr_batch_sync(self._h), "gp_corr_batch_sync")
            out = err.cpu().numpy()
        return out[self._slot].copy()

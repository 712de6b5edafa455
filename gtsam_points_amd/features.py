"""GPU counterparts of the CPU-only pieces BASELINE.json configs[4] names, over the C-ABI:

  KdTreeGPU                 <- ann/kdtree.hpp / small_kdtree.hpp (exact k-NN; here a cell-sorted point grid)
  estimate_covariances_gpu  <- features/covariance_estimation.hpp:estimate_covariances(points, k=10)
  estimate_normals_gpu      <- features/normal_estimation.hpp:estimate_normals(points, k=10); estimate_normals_covariances_gpu: both from one search
  estimate_intensity_gradients_gpu  <- factors/intensity_gradients.hpp:IntensityGradients::estimate (CPU-only upstream) -> IntensityGradientsGPU
  estimate_fpfh_gpu         <- features/fpfh_estimation.hpp:estimate_fpfh (CPU-only upstream): 33-D descriptors over a fixed-radius search, for registration.py

The matching-cost factors on nearest-neighbour correspondences that grew up here (GICP, ICP, LOAM, colored GICP, the continuous-time factors, their batch) live in
corr_factors.py; every name is still exported from this module (the import at the end).
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _capi
from .types import GaussianVoxelMapGPU, PointCloudGPU


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


class IntensityKdTreeGPU:
    """IntensityKdTree (ann/intensity_kdtree.hpp) over a PointCloudGPU with intensities: exact 1-NN in (x, y, z, intensity).  The distance of a query (q, I_q) to
    target point j is |q - x_j|^2 + (I_q - intensity_scale * I_j)^2 -- the scale on the STORED side only, as the reference writes it; at 1.0 the plain XYZI metric.
    f64 on the f32 inputs; ties go to the lowest index.  k = 1 only, no search_eps; a point with a non-finite coordinate or intensity is never matched, a query
    with one gets -1.  What the photometric factors take as target_tree to search in 4-D."""

    def __init__(self, frame: PointCloudGPU, intensity_scale=1.0, cell_size=0.25, stream=None):
        self._lib = _capi.load()
        if frame.points_gpu is None or frame.intensities_gpu is None:
            raise _capi.GPError("error: the frame has no points or no intensities for an IntensityKdTreeGPU")
        self.frame = frame
        self.intensity_scale = float(intensity_scale)
        GaussianVoxelMapGPU._sync_torch(frame)
        h = C.c_void_p()
        _capi.check(self._lib.gp_intensity_grid_create(frame.ptr(frame.points_gpu), frame.ptr(frame.intensities_gpu), frame.size(), self.intensity_scale, float(cell_size),
                                                       stream, C.byref(h)), "gp_intensity_grid_create")
        self._xyzi = h
        self._h = C.c_void_p(self._lib.gp_intensity_grid_point_grid(h))  # the 3-D structure inside: what a factor's create takes as its grid
        self._intensities_ptr = frame.intensities_gpu.data_ptr()
        self.stream = stream

    def __del__(self):
        if getattr(self, "_xyzi", None):
            self._lib.gp_intensity_grid_destroy(self._xyzi)
            self._xyzi = self._h = None

    def knn_search(self, queries, k=1, max_sq_dist=np.finfo(np.float64).max):
        """queries: (Q,4) numpy/torch rows (x, y, z, intensity), read as float64 -> (indices (Q,1) int32 with -1 where there is none, sq_dists (Q,1) float64: the
        4-D squared distances, max_sq_dist where there is none; num_found (Q,))"""
        import torch

        if int(k) != 1:
            raise _capi.GPError("IntensityKdTreeGPU.knn_search: k must be 1 (the XYZI search keeps one neighbour)")
        dev = self.frame.device
        q = torch.as_tensor(np.asarray(queries, dtype=np.float64) if not isinstance(queries, torch.Tensor) else queries).to(device=dev, dtype=torch.float64).reshape(-1, 4).contiguous()
        m = int(q.shape[0])
        idx = torch.empty((m, 1), dtype=torch.int32, device=dev)
        d = torch.empty((m, 1), dtype=torch.float64, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        _capi.check(self._lib.gp_intensity_grid_search(self._xyzi, C.c_void_p(q.data_ptr()), m, float(max_sq_dist), C.c_void_p(idx.data_ptr()), C.c_void_p(d.data_ptr()),
                                                       self.stream), "gp_intensity_grid_search")
        _capi.check(self._lib.gp_stream_synchronize(self.stream), "sync")
        idx = idx.cpu().numpy()
        return idx, d.cpu().numpy(), (idx[:, 0] >= 0).astype(np.int32)


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


# the factors that lived here, under their old address.  At the END: corr_factors takes KdTreeGPU and estimate_intensity_gradients_gpu from this module, which must be
# defined when it is imported from here -- so this module is imported before it (the package does)
from .corr_factors import (  # noqa: E402,F401
    CorrespondenceFactorBatchGPU,
    IntegratedColorConsistencyFactorGPU,
    IntegratedColoredGICPFactorGPU,
    IntegratedCTGICPFactorGPU,
    IntegratedCTICPFactorGPU,
    IntegratedGICPFactorGPU,
    IntegratedICPFactorGPU,
    IntegratedLOAMFactorGPU,
    IntegratedPointToEdgeFactorGPU,
    IntegratedPointToPlaneFactorGPU,
    IntegratedPointToPlaneICPFactorGPU,
)

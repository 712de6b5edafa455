"""Down-sampling of a PointCloudGPU on the device, over the C-ABI (csrc/gp_sampling.hip):

  sample_gpu               <- types/point_cloud_cpu.hpp:110 sample(frame, indices)
  voxelgrid_sampling_gpu   <- :124 voxelgrid_sampling(frame, voxel_resolution)            (point_cloud_cpu_funcs.cpp:119-295)
  randomgrid_sampling_gpu  <- :138 randomgrid_sampling(frame, voxel_resolution, rate, mt)  (point_cloud_cpu_funcs.cpp:298-456)
  find_inlier_points_gpu   <- :248 find_inlier_points(frame, neighbors, k, std_thresh)      (point_cloud_cpu_funcs.cpp:576-612)
  remove_outliers_gpu      <- :258,267 remove_outliers(frame, [neighbors,] k, std_thresh)   (point_cloud_cpu_funcs.cpp:614-650)
  filter_gpu               <- :164 filter / :181 filter_by_index, the predicate evaluated by the caller into a mask
  sort_by_time_gpu         <- :209 sort_by_time(frame)                                      (point_cloud_cpu_funcs.cpp:459-465)

CPU-only upstream; these are device counterparts, not ports (include/gtsam_points_hip.h states what is and is not reproduced).  Every result is a NEW PointCloudGPU
on the frame's device that holds each attribute the input holds on the device (points, covs, normals, intensities, times), device to device; the input frame is not
modified and its generation does not change.
"""
import ctypes as C
import math

from . import _capi
from .types import GaussianVoxelMapGPU, PointCloudGPU

_WIDTH = {"points": 3, "covs": 9, "normals": 3, "intensities": 1, "times": 1}


def _device_attrs(frame):
    return [(a, getattr(frame, a + "_gpu")) for a in PointCloudGPU._ATTRS if getattr(frame, a + "_gpu") is not None]


def _new_cloud(frame, attrs, n):
    """a fresh cloud of device-only attributes (no host copies: offload_gpu() downloads them first, as for from_device)"""
    out = PointCloudGPU(device=str(frame.device))
    for a, t in attrs.items():
        setattr(out, a + "_gpu", t)
    out.num_points = int(n)
    out.generation += 1
    return out


class VoxelGridPlan:
    """gp_voxelgrid_plan: the points of `frame` sorted by voxel at `voxel_resolution`, built once; average() / random_indices() run on it any number of times.
    num_voxels: occupied voxels; num_dropped: points without a voxel (non-finite, or beyond +-2^20 voxels on an axis) -- they appear in no output."""

    def __init__(self, frame: PointCloudGPU, voxel_resolution, stream=None):
        self._lib = _capi.load()
        self._h = None
        self.frame = frame
        self.stream = stream
        self.num_points = frame.size() if frame.points_gpu is not None else 0
        if self.num_points:
            GaussianVoxelMapGPU._sync_torch(frame)
        h = C.c_void_p()
        _capi.check(self._lib.gp_voxelgrid_plan_create(frame.ptr(frame.points_gpu) if self.num_points else None, self.num_points, float(voxel_resolution), stream, C.byref(h)),
                    "gp_voxelgrid_plan_create")
        self._h = h
        nv, nd = C.c_int(0), C.c_int(0)
        _capi.check(self._lib.gp_voxelgrid_plan_info(self._h, C.byref(nv), C.byref(nd)), "gp_voxelgrid_plan_info")
        self.num_voxels, self.num_dropped = nv.value, nd.value

    def close(self):
        if getattr(self, "_h", None):
            self._lib.gp_voxelgrid_plan_destroy(self._h)
            self._h = None

    __del__ = close

    def average(self, attr, sync=True):
        """float32 device tensor (num_points, w) or (num_points,) -> the per-voxel means (num_voxels, w), in voxel order"""
        import torch

        t = attr.reshape(self.num_points, int(attr.shape[1]) if attr.dim() > 1 else 1)
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.frame.device:
            raise ValueError("average: a contiguous float32 tensor on the plan's device is expected")
        out = torch.empty((self.num_voxels, t.shape[1]), dtype=torch.float32, device=t.device)
        torch.cuda.current_stream(t.device).synchronize()
        _capi.check(self._lib.gp_voxelgrid_plan_average(self._h, C.c_void_p(t.data_ptr()) if self.num_points else None, int(t.shape[1]),
                                                        C.c_void_p(out.data_ptr()) if self.num_voxels else None), "gp_voxelgrid_plan_average")
        if sync:
            _capi.check(self._lib.gp_stream_synchronize(self.stream), "gp_stream_synchronize")
        return out

    def random_indices(self, sampling_rate, seed=0):
        """the selection of randomgrid_sampling as an int32 device tensor of ascending point indices"""
        import torch

        idx = torch.empty(max(self.num_points, 1), dtype=torch.int32, device=self.frame.device)
        torch.cuda.current_stream(self.frame.device).synchronize()
        k = C.c_int(0)
        _capi.check(self._lib.gp_voxelgrid_plan_random_indices(self._h, float(sampling_rate), int(seed) & 0xFFFFFFFFFFFFFFFF, C.c_void_p(idx.data_ptr()), C.byref(k)),
                    "gp_voxelgrid_plan_random_indices")
        return idx[: k.value]


def sample_gpu(frame: PointCloudGPU, indices, stream=None):
    """sample(frame, indices): row i of every device attribute of the result is row indices[i] of the frame's (repeated and unsorted indices allowed).
    indices: an int sequence, numpy array or torch tensor; out-of-range indices raise IndexError."""
    import torch

    idx = torch.as_tensor(indices).to(device=frame.device, dtype=torch.int32).reshape(-1).contiguous()
    m = int(idx.shape[0])
    n = frame.size()
    if m and (n == 0 or int(idx.min()) < 0 or int(idx.max()) >= n):
        raise IndexError("sample_gpu: index out of range")
    return _gather_rows(frame, idx, stream)


def _gather_rows(frame, idx, stream=None):
    """sample() for an int32 device tensor of indices that are known to lie inside the frame (the library's own selections)"""
    import torch

    lib = _capi.load()
    m = int(idx.shape[0])
    out = {}
    torch.cuda.current_stream(frame.device).synchronize()
    for a, t in _device_attrs(frame):
        w = _WIDTH[a]
        o = torch.empty((m, w), dtype=torch.float32, device=frame.device)
        _capi.check(lib.gp_cloud_gather(C.c_void_p(t.data_ptr()) if m else None, w, C.c_void_p(idx.data_ptr()) if m else None, m, C.c_void_p(o.data_ptr()) if m else None, stream),
                    "gp_cloud_gather")
        out[a] = o
    _capi.check(lib.gp_stream_synchronize(stream), "gp_stream_synchronize")
    return _new_cloud(frame, out, m)


def voxelgrid_sampling_gpu(frame: PointCloudGPU, voxel_resolution, stream=None):
    """voxelgrid_sampling: one point per occupied voxel, every device attribute the mean of the voxel's rows (f64 accumulation, one rounding to f32; normals are not
    re-normalised, as upstream), voxels in ascending (z, y, x) order.  The result carries `num_dropped`: the input points that have no voxel (non-finite, or beyond
    +-2^20 voxels) and therefore contribute to no row.  An empty input gives an empty cloud."""
    plan = VoxelGridPlan(frame, voxel_resolution, stream)
    try:
        out = {a: plan.average(t, sync=False) for a, t in _device_attrs(frame)}
        _capi.check(plan._lib.gp_stream_synchronize(stream), "gp_stream_synchronize")
        cloud = _new_cloud(frame, out, plan.num_voxels)
        cloud.num_dropped = plan.num_dropped
        return cloud
    finally:
        plan.close()


def randomgrid_sampling_gpu(frame: PointCloudGPU, voxel_resolution, sampling_rate, seed=0, stream=None):
    """randomgrid_sampling: about sampling_rate x N points spread evenly over the voxels -- ceil(sampling_rate x N / num_voxels) per voxel (all of a smaller voxel),
    chosen by a counter-based hash of (seed, point index): the same seed gives the same cloud.  sampling_rate >= 0.99 keeps every valid point.  The rows are the
    input's own, in ascending point index; the result carries `sample_indices_gpu` (int32 device tensor) and `num_dropped`."""
    plan = VoxelGridPlan(frame, voxel_resolution, stream)
    try:
        idx = plan.random_indices(sampling_rate, seed)
        cloud = sample_gpu(frame, idx, stream)
        cloud.sample_indices_gpu = idx
        cloud.num_dropped = plan.num_dropped
        return cloud
    finally:
        plan.close()


# ---- remove_outliers / filter / sort_by_time: an index selection on the device, then sample() -------------------------------------------------------------------------
_OUTLIER_CELL_SIZE = 0.25


def _inlier_selection(frame, k, std_thresh, neighbors, tree, stream):
    """(inlier indices, mean distances, [mean, var, thresh, m], num_short) of find_inlier_points, all selections on the device"""
    import torch

    from .features import KdTreeGPU

    lib = _capi.load()
    k, std_thresh = int(k), float(std_thresh)
    # refused before any device work (the C entry points refuse the same, but the search structure would have been built by then)
    if k < 1 or (neighbors is None and k > 32):
        raise _capi.GPError(f"find_inlier_points_gpu: k = {k} is outside 1 .. 32 (the fused search; caller-supplied neighbours take any k >= 1)")
    if not math.isfinite(std_thresh):
        raise _capi.GPError("find_inlier_points_gpu: std_thresh must be finite")
    if frame.points_gpu is None:
        raise _capi.GPError("find_inlier_points_gpu: the frame has no points on the device")
    n = frame.size()
    dev = frame.device
    dists = torch.empty(n, dtype=torch.float64, device=dev)
    idx = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    short, kept = C.c_int(0), C.c_int(0)
    stats = (C.c_double * 4)()
    pts = frame.ptr(frame.points_gpu) if n else None
    if neighbors is not None:
        nb = torch.as_tensor(neighbors).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
        if int(nb.shape[0]) != n * k:
            raise ValueError(f"find_inlier_points_gpu: neighbors holds {int(nb.shape[0])} indices, {n} x {k} are expected")
        torch.cuda.current_stream(dev).synchronize()
        _capi.check(lib.gp_cloud_mean_neighbor_distances_from(pts, n, C.c_void_p(nb.data_ptr()) if n else None, k, C.c_void_p(dists.data_ptr()) if n else None, C.byref(short),
                                                              stream), "gp_cloud_mean_neighbor_distances_from")
    elif n:
        if tree is None:
            tree = KdTreeGPU(frame, cell_size=_OUTLIER_CELL_SIZE, stream=stream)
        elif tree.frame.points_gpu is None or tree.frame.points_gpu.data_ptr() != frame.points_gpu.data_ptr():
            raise _capi.GPError("error: tree was not built over the frame's points")
        torch.cuda.current_stream(dev).synchronize()
        _capi.check(lib.gp_cloud_mean_neighbor_distances(tree._h, pts, n, k, C.c_void_p(dists.data_ptr()), C.byref(short), stream), "gp_cloud_mean_neighbor_distances")
    d_ptr = C.c_void_p(dists.data_ptr()) if n else None
    _capi.check(lib.gp_cloud_inlier_threshold(d_ptr, n, std_thresh, stats, stream), "gp_cloud_inlier_threshold")
    _capi.check(lib.gp_cloud_select_below(d_ptr, n, stats[2], C.c_void_p(idx.data_ptr()) if n else None, C.byref(kept), stream), "gp_cloud_select_below")
    return idx[: kept.value], dists, list(stats), short.value


def find_inlier_points_gpu(frame: PointCloudGPU, k=10, std_thresh=1.0, neighbors=None, tree=None, stream=None):
    """find_inlier_points: the ascending indices (int32 device tensor) of the points whose mean distance d_i to their k nearest neighbours in the cloud -- the point
    itself among them, at distance 0 -- is below mean(d) + std_thresh x sqrt(var(d)) (strict; var = E[d^2] - E[d]^2 in one pass, as upstream).
    neighbors: the caller's lists, (n, k) or flat, any k >= 1 (the first upstream overload).  Otherwise an exact search with 1 <= k <= 32 on `tree`, a KdTreeGPU over
    this frame's points that many calls may share, or, with tree = None, on a grid built for the call with 0.25 m cells: the cell size KdTreeGPU and
    estimate_covariances_gpu default to, chosen there for a k = 10 search on LiDAR scans.  The search is exact, so the cell size changes the time, never the result.
    Short points -- a non-finite coordinate, fewer than k neighbours (n < k), a listed index outside [0, n) -- are left out of the statistics and are never inliers
    (upstream reads points[-1] there)."""
    return _inlier_selection(frame, k, std_thresh, neighbors, tree, stream)[0]


def remove_outliers_gpu(frame: PointCloudGPU, k=10, std_thresh=1.0, neighbors=None, tree=None, stream=None):
    """remove_outliers: sample(frame, find_inlier_points(...)) -- a new cloud of the inliers' rows of every device attribute, in ascending point index; the input is not
    modified.  The result carries `inlier_indices_gpu` (int32), `mean_dists_gpu` (float64 [n] of the INPUT's points, +inf for short points), `dist_mean`, `dist_var`,
    `dist_thresh` and `num_short`.  Arguments as find_inlier_points_gpu."""
    idx, dists, stats, short = _inlier_selection(frame, k, std_thresh, neighbors, tree, stream)
    cloud = _gather_rows(frame, idx, stream)
    cloud.inlier_indices_gpu = idx
    cloud.mean_dists_gpu = dists
    cloud.dist_mean, cloud.dist_var, cloud.dist_thresh = stats[0], stats[1], stats[2]
    cloud.num_short = short
    return cloud


def filter_gpu(frame: PointCloudGPU, mask, stream=None):
    """filter / filter_by_index with the predicate already evaluated: keeps the rows whose mask entry is true, in order.  mask: a bool or uint8 numpy array or torch
    tensor of length n (e.g. a torch expression on frame.points_gpu); any other length raises ValueError.  The result carries `sample_indices_gpu`."""
    import torch

    lib = _capi.load()
    n = frame.size()
    m = torch.as_tensor(mask)
    if m.dtype not in (torch.bool, torch.uint8):
        raise ValueError("filter_gpu: a bool or uint8 mask is expected")
    m = m.reshape(-1)
    if int(m.shape[0]) != n:
        raise ValueError(f"filter_gpu: the mask has {int(m.shape[0])} entries, the frame {n} points")
    m = m.to(device=frame.device, dtype=torch.uint8).contiguous()
    idx = torch.empty(max(n, 1), dtype=torch.int32, device=frame.device)
    kept = C.c_int(0)
    torch.cuda.current_stream(frame.device).synchronize()
    _capi.check(lib.gp_cloud_select_mask(C.c_void_p(m.data_ptr()) if n else None, n, C.c_void_p(idx.data_ptr()) if n else None, C.byref(kept), stream), "gp_cloud_select_mask")
    cloud = _gather_rows(frame, idx[: kept.value], stream)
    cloud.sample_indices_gpu = idx[: kept.value]
    return cloud


def sort_by_time_gpu(frame: PointCloudGPU, stream=None):
    """sort_by_time: the rows of every device attribute in ascending order of frame.times_gpu.  Stable: equal times stay in ascending point index (one of std::sort's
    legal outcomes); -0.0 and +0.0 are equal; NaN times go last, in ascending index.  A frame without times raises GPError.  The result carries `sample_indices_gpu`."""
    import torch

    if frame.times_gpu is None:
        raise _capi.GPError("error: frame does not have times on GPU!!")
    lib = _capi.load()
    n = frame.size()
    idx = torch.empty(max(n, 1), dtype=torch.int32, device=frame.device)
    torch.cuda.current_stream(frame.device).synchronize()
    _capi.check(lib.gp_cloud_sort_by_time_indices(frame.ptr(frame.times_gpu) if n else None, n, C.c_void_p(idx.data_ptr()) if n else None, stream), "gp_cloud_sort_by_time_indices")
    cloud = _gather_rows(frame, idx[:n], stream)
    cloud.sample_indices_gpu = idx[:n]
    return cloud

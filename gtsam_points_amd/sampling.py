"""Down-sampling of a PointCloudGPU on the device, over the C-ABI (csrc/gp_sampling.hip):

  sample_gpu               <- types/point_cloud_cpu.hpp:110 sample(frame, indices)
  voxelgrid_sampling_gpu   <- :124 voxelgrid_sampling(frame, voxel_resolution)            (point_cloud_cpu_funcs.cpp:119-295)
  randomgrid_sampling_gpu  <- :138 randomgrid_sampling(frame, voxel_resolution, rate, mt)  (point_cloud_cpu_funcs.cpp:298-456)

CPU-only upstream; these are device counterparts, not ports (include/gtsam_points_hip.h states what is and is not reproduced).  Every result is a NEW PointCloudGPU
on the frame's device that holds each attribute the input holds on the device (points, covs, normals, intensities, times), device to device; the input frame is not
modified and its generation does not change.
"""
import ctypes as C

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

    lib = _capi.load()
    idx = torch.as_tensor(indices).to(device=frame.device, dtype=torch.int32).reshape(-1).contiguous()
    m = int(idx.shape[0])
    n = frame.size()
    if m and (n == 0 or int(idx.min()) < 0 or int(idx.max()) >= n):
        raise IndexError("sample_gpu: index out of range")
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

"""gtsam_points_amd -- MI355X (gfx950) native VGICP path behind koide3/gtsam_points' GPU API.

The compute lives in libgtsam_points_hip.so (hand-written HIP, C-ABI in include/gtsam_points_hip.h).
This package is the thin host-side mirror of the reference's classes used by the tests and bench;
gtsam_points_amd/host/ holds the C++ mirror a GTSAM application links.  There is NO CPU fallback:
every class raises if the HIP library cannot be loaded.
"""
from ._capi import GPError, LIB_PATH, load  # noqa: F401
from .factors import (  # noqa: F401
    HessianFactor,
    IntegratedVGICPFactorGPU,
    LinearizationHook,
    LinearizedSystem6,
    NonlinearFactorGPU,
    NonlinearFactorSetGPU,
    StreamTempBufferRoundRobin,
    TempBufferManager,
    create_nonlinear_factor_set_gpu,
    pose_inverse,
)
from .features import (  # noqa: F401
    CorrespondenceFactorBatchGPU,
    IntegratedGICPFactorGPU,
    IntegratedICPFactorGPU,
    IntegratedLOAMFactorGPU,
    IntegratedPointToEdgeFactorGPU,
    IntegratedPointToPlaneFactorGPU,
    IntegratedPointToPlaneICPFactorGPU,
    KdTreeGPU,
    estimate_covariances_gpu,
    estimate_normals_covariances_gpu,
    estimate_normals_gpu,
)
from .sampling import (  # noqa: F401
    VoxelGridPlan,
    filter_gpu,
    find_inlier_points_gpu,
    randomgrid_sampling_gpu,
    remove_outliers_gpu,
    sample_gpu,
    sort_by_time_gpu,
    voxelgrid_sampling_gpu,
)
from .solver import (  # noqa: F401
    BetweenFactorPose3,
    DenseLinearSystemGPU,
    LevenbergMarquardtGraphGPU,
    PoseFactorsGPU,
    PriorFactorPose3,
    SparseLinearSystemGPU,
    linearize_on_device,
    sparse_symbolic,
)
from .types import GaussianVoxelMapGPU, PointCloudGPU, merge_frames_gpu, overlap_gpu  # noqa: F401

__all__ = [
    "GPError",
    "GaussianVoxelMapGPU",
    "HessianFactor",
    "IntegratedGICPFactorGPU",
    "CorrespondenceFactorBatchGPU",
    "IntegratedICPFactorGPU",
    "IntegratedPointToPlaneICPFactorGPU",
    "IntegratedLOAMFactorGPU",
    "IntegratedPointToEdgeFactorGPU",
    "IntegratedPointToPlaneFactorGPU",
    "IntegratedVGICPFactorGPU",
    "KdTreeGPU",
    "estimate_covariances_gpu",
    "estimate_normals_gpu",
    "estimate_normals_covariances_gpu",
    "LinearizationHook",
    "LinearizedSystem6",
    "NonlinearFactorGPU",
    "NonlinearFactorSetGPU",
    "PointCloudGPU",
    "StreamTempBufferRoundRobin",
    "TempBufferManager",
    "create_nonlinear_factor_set_gpu",
    "overlap_gpu",
    "merge_frames_gpu",
    "VoxelGridPlan",
    "sample_gpu",
    "find_inlier_points_gpu",
    "remove_outliers_gpu",
    "filter_gpu",
    "sort_by_time_gpu",
    "voxelgrid_sampling_gpu",
    "randomgrid_sampling_gpu",
    "BetweenFactorPose3",
    "DenseLinearSystemGPU",
    "LevenbergMarquardtGraphGPU",
    "PoseFactorsGPU",
    "PriorFactorPose3",
    "SparseLinearSystemGPU",
    "sparse_symbolic",
    "linearize_on_device",
    "load",
]

"""The Python surface of the matching-cost factors after their move from features.py to corr_factors.py onto one base class: every name the package and
gtsam_points_amd.features exported stays importable from both, every factor class and the batch keeps its public attribute set (the lists below were taken with
dir() from the classes as they stood in features.py), and the isinstance relations hold.  No device: nothing is constructed."""
import importlib

import gtsam_points_amd as gpa
from gtsam_points_amd import corr_factors, features

# what features.py defined (its classes and functions; the modules it imported for its own use are not part of this)
FEATURES_NAMES = [
    "CorrespondenceFactorBatchGPU", "FPFHEstimationParams", "IntegratedCTGICPFactorGPU", "IntegratedCTICPFactorGPU", "IntegratedColoredGICPFactorGPU",
    "IntegratedGICPFactorGPU", "IntegratedICPFactorGPU", "IntegratedLOAMFactorGPU", "IntegratedPointToEdgeFactorGPU", "IntegratedPointToPlaneFactorGPU",
    "IntegratedPointToPlaneICPFactorGPU", "IntensityGradientsGPU", "KdTreeGPU", "estimate_covariances_gpu", "estimate_fpfh_gpu", "estimate_intensity_gradients_gpu",
    "estimate_normals_covariances_gpu", "estimate_normals_gpu",
]
MOVED = [
    "CorrespondenceFactorBatchGPU", "IntegratedCTGICPFactorGPU", "IntegratedCTICPFactorGPU", "IntegratedColoredGICPFactorGPU", "IntegratedGICPFactorGPU",
    "IntegratedICPFactorGPU", "IntegratedLOAMFactorGPU", "IntegratedPointToEdgeFactorGPU", "IntegratedPointToPlaneFactorGPU", "IntegratedPointToPlaneICPFactorGPU",
]
PACKAGE_NAMES = [
    "BetweenFactorPose3", "BundleAdjustmentFactorsGPU", "CorrespondenceFactorBatchGPU", "DenseLinearSystemGPU", "EdgeEVMFactorGPU", "FPFHEstimationParams", "GNCParams",
    "GNCTrace", "GPError", "GaussianVoxelMapGPU", "HessianFactor", "IntegratedCTGICPFactorGPU", "IntegratedCTICPFactorGPU", "IntegratedColoredGICPFactorGPU",
    "IntegratedGICPFactorGPU", "IntegratedICPFactorGPU", "IntegratedLOAMFactorGPU", "IntegratedPointToEdgeFactorGPU", "IntegratedPointToPlaneFactorGPU",
    "IntegratedPointToPlaneICPFactorGPU", "IntegratedVGICPFactorGPU", "IntensityGradientsGPU", "KdTreeGPU", "LIB_PATH", "LevenbergMarquardtGraphGPU", "LinearizationHook",
    "LinearizedSystem6", "NonlinearFactorGPU", "NonlinearFactorSetGPU", "OccupancyGridGPU", "PlaneEVMFactorGPU", "PointCloudGPU", "PoseFactorsGPU", "PriorFactorPose3",
    "RANSACHypotheses", "RANSACParams", "RegistrationResult", "SparseLinearSystemGPU", "StreamTempBufferRoundRobin", "TempBufferManager", "VoxelGridPlan",
    "align_points_4dof_gpu", "align_points_se3_gpu", "bundle_adjustment", "create_nonlinear_factor_set_gpu", "estimate_covariances_gpu", "estimate_fpfh_gpu",
    "estimate_intensity_gradients_gpu", "estimate_normals_covariances_gpu", "estimate_normals_gpu", "estimate_pose_gnc_gpu", "estimate_pose_ransac_gpu", "factors", "features",
    "filter_gpu", "find_feature_correspondences_gpu", "find_inlier_points_gpu", "gnc_align_correspondences_gpu", "linearize_on_device", "load", "match_features_gpu",
    "merge_frames_gpu", "overlap_gpu", "pose_inverse", "randomgrid_sampling_gpu", "registration", "remove_outliers_gpu", "sample_gpu", "sampling", "solver",
    "sort_by_time_gpu", "sparse_symbolic", "types", "voxelgrid_sampling_gpu",
]

RELATIVE = ["calc_delta", "error", "keys", "linearize", "linearize_delta", "num_inliers"]
LOAM = RELATIVE + ["correspondences", "num_correspondences", "set_correspondence_update_tolerance", "set_enable_correspondence_validation", "set_max_correspondence_distance"]
CT = ["correspondences", "deskewed_source_points", "error", "keys", "linearize", "num_inliers", "pose_table", "time_table"]
PUBLIC = {
    "IntegratedGICPFactorGPU": RELATIVE,
    "IntegratedICPFactorGPU": RELATIVE + ["set_correspondence_update_tolerance"],
    "IntegratedColoredGICPFactorGPU": RELATIVE + ["set_correspondence_update_tolerance", "set_max_correspondence_distance", "set_photometric_term_weight"],
    "IntegratedLOAMFactorGPU": LOAM,
    "IntegratedPointToEdgeFactorGPU": LOAM,
    "IntegratedPointToPlaneFactorGPU": LOAM,
    "IntegratedCTICPFactorGPU": CT,
    "IntegratedCTGICPFactorGPU": CT,
    "CorrespondenceFactorBatchGPU": ["close", "errors", "linearize_deltas"],
}


def test_every_exported_name_is_still_there():
    assert not set(PACKAGE_NAMES) - set(dir(gpa))  # (a superset: corr_factors is new, and dir() also lists whatever submodule another test imported)
    assert len(gpa.__all__) == len(set(gpa.__all__)) == 65 and all(hasattr(gpa, n) for n in gpa.__all__)
    for n in FEATURES_NAMES:
        assert getattr(features, n) is getattr(gpa, n), n
    for n in MOVED:
        assert getattr(corr_factors, n) is getattr(features, n), n
        assert getattr(corr_factors, n).__module__ == "gtsam_points_amd.corr_factors", n
    ns = {}
    exec("from gtsam_points_amd.features import " + ", ".join(FEATURES_NAMES), ns)  # the form the tests and scripts use
    assert all(ns[n] is getattr(features, n) for n in FEATURES_NAMES)
    assert importlib.import_module("gtsam_points_amd.corr_factors") is corr_factors


def test_public_attributes_of_the_factor_classes():
    for name, want in PUBLIC.items():
        cls = getattr(gpa, name)
        assert sorted(n for n in dir(cls) if not n.startswith("_")) == sorted(want), name


def test_isinstance_relations():
    assert issubclass(gpa.IntegratedPointToEdgeFactorGPU, gpa.IntegratedLOAMFactorGPU) and issubclass(gpa.IntegratedPointToPlaneFactorGPU, gpa.IntegratedLOAMFactorGPU)
    assert issubclass(gpa.IntegratedCTGICPFactorGPU, gpa.IntegratedCTICPFactorGPU)
    # the batch sorts its members by these four types: none may be a subclass of another
    four = [gpa.IntegratedGICPFactorGPU, gpa.IntegratedICPFactorGPU, gpa.IntegratedLOAMFactorGPU, gpa.IntegratedColoredGICPFactorGPU]
    assert all(not issubclass(a, b) for a in four for b in four if a is not b)
    assert not any(issubclass(gpa.IntegratedCTICPFactorGPU, c) or issubclass(c, gpa.IntegratedCTICPFactorGPU) for c in four)
    assert callable(gpa.IntegratedPointToPlaneICPFactorGPU) and not isinstance(gpa.IntegratedPointToPlaneICPFactorGPU, type)  # (a constructor function, as before)
    # one C prefix per class
    want = {"IntegratedGICPFactorGPU": "gp_gicp_factor", "IntegratedICPFactorGPU": "gp_icp_factor", "IntegratedColoredGICPFactorGPU": "gp_colored_gicp_factor",
            "IntegratedLOAMFactorGPU": "gp_loam_factor", "IntegratedPointToEdgeFactorGPU": "gp_loam_factor", "IntegratedCTICPFactorGPU": "gp_ct_factor",
            "IntegratedCTGICPFactorGPU": "gp_ct_factor"}
    from gtsam_points_amd import _capi

    for name, prefix in want.items():
        assert getattr(gpa, name)._PREFIX == prefix
        for entry in ("destroy", "linearize", "compute_error"):
            assert f"{prefix}_{entry}" in _capi.EXPORTED_SYMBOLS

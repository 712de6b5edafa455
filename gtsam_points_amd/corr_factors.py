"""The matching-cost factors on nearest-neighbour correspondences, over the C-ABI (CPU-only upstream; csrc/gp_corr_factors.hip, gp_colored_factors.hip,
gp_ct_factors.hip, gp_corr_batch.hip):

  IntegratedGICPFactorGPU   <- factors/integrated_gicp_factor.hpp, same calc_delta / HessianFactor protocol as the VGICP factor
  IntegratedICPFactorGPU    <- factors/integrated_icp_factor.hpp (point-to-point / point-to-plane), on a shared KdTreeGPU
  IntegratedPointToEdgeFactorGPU / IntegratedPointToPlaneFactorGPU / IntegratedLOAMFactorGPU
                            <- factors/integrated_loam_factor.hpp, on the 2 / 3 nearest points of shared KdTreeGPUs
  IntegratedColoredGICPFactorGPU    <- factors/integrated_colored_gicp_factor.hpp, on a shared KdTreeGPU and the target's intensity gradients
  IntegratedCTICPFactorGPU / IntegratedCTGICPFactorGPU
                            <- factors/integrated_ct_icp_factor.hpp, integrated_ct_gicp_factor.hpp: two pose keys, one pose per time stamp
  CorrespondenceFactorBatchGPU  any number of the relative-pose factors above linearised / evaluated together, the poses in device memory (gp_corr_batch_*)

features.py re-exports every name (they lived there); it is imported first -- by the package -- and imports this module at its end, when what this module takes
from it is defined.
"""
import ctypes as C

import numpy as np

from . import _capi
from .factors import HessianFactor, LinearizedSystem6, pose_inverse
from .features import IntensityKdTreeGPU, KdTreeGPU, estimate_intensity_gradients_gpu
from .types import GaussianVoxelMapGPU, PointCloudGPU, _pose16


class _CorrFactorGPU:
    """What every factor here keeps: the handle `_h` of the C factor `_PREFIX`_*, the keys, the inliers of the last linearise, and the trees it borrows."""

    _PREFIX = None  # "gp_icp_factor": the C entry points are _PREFIX + "_create", "_linearize", ...

    def _call(self, name, *args):
        _capi.check(getattr(self._lib, f"{self._PREFIX}_{name}")(self._h, *args), f"{self._PREFIX}_{name}")

    def _adopt(self, h, stream):
        """the created handle; the two hot entry points are looked up once, with the names _capi.check reports them under (_call's lookup by name is for the setters
        and getters: it costs a 20 us error evaluation a percent)"""
        self._h = h
        self.stream = stream
        self._num_inliers = 0
        self._c_linearize = getattr(self._lib, f"{self._PREFIX}_linearize"), f"{self._PREFIX}_linearize"
        self._c_error = getattr(self._lib, f"{self._PREFIX}_compute_error"), f"{self._PREFIX}_compute_error"

    @staticmethod
    def _shared_tree(target, tree, stream):
        """the KdTreeGPU over `target` that many factors may share (held by reference, never rebuilt); None builds one; no target, no tree"""
        if target is None:
            return None
        tree = tree if tree is not None else KdTreeGPU(target, stream=stream)
        if tree.frame.points_gpu is None or tree.frame.points_gpu.data_ptr() != target.points_gpu.data_ptr():
            raise _capi.GPError("error: target_tree was not built over the target frame's points")
        if isinstance(tree, IntensityKdTreeGPU) and (target.intensities_gpu is None or tree._intensities_ptr != target.intensities_gpu.data_ptr()):
            raise _capi.GPError("error: target_tree was not built over the target frame's points and intensities")
        return tree

    def _photometric_tree(self, target, tree, stream):
        """_shared_tree for the factors that may search in XYZI: a KdTreeGPU (the 3-D search -- what the reference does when handed a plain KdTree, which ignores
        pt[3]) or an IntensityKdTreeGPU"""
        if tree is not None and not isinstance(tree, (KdTreeGPU, IntensityKdTreeGPU)):
            raise TypeError("target_tree must be a KdTreeGPU or an IntensityKdTreeGPU")
        return self._shared_tree(target, tree, stream)

    def _searches_xyzi(self):
        return isinstance(getattr(self, "target_tree", None), IntensityKdTreeGPU)

    def __del__(self):
        if getattr(self, "_h", None):
            # before the trees (and gradients) the handle borrows: the factor's attributes are still referenced here
            getattr(self._lib, f"{self._PREFIX}_destroy")(self._h)
            self._h = None

    def keys(self):
        return self._keys

    def num_inliers(self):
        return self._num_inliers


class _RelativePoseFactorGPU(_CorrFactorGPU):
    """A factor on delta = T_target^-1 T_source between two pose keys, or on one key against a fixed target pose (the reference's binary / unary constructors).
    A subclass checks its frames' attributes with the reference's texts, creates its C factor and hands the handle to _adopt."""


    def _init_keys(self, target_key, source_key, fixed_target_pose):
        self._lib = _capi.load()
        self.is_binary = fixed_target_pose is None
        self._keys = [target_key, source_key] if self.is_binary else [source_key]
        self.fixed_target_pose = np.eye(4) if self.is_binary else np.asarray(fixed_target_pose, dtype=np.float64)

    def _adopt(self, h, stream):
        super()._adopt(h, stream)
        self.linearization_point = np.eye(4)

    def calc_delta(self, values):
        if not self.is_binary:
            return pose_inverse(self.fixed_target_pose) @ np.asarray(values[self._keys[0]], dtype=np.float64)
        return pose_inverse(values[self._keys[0]]) @ np.asarray(values[self._keys[1]], dtype=np.float64)

    def linearize_delta(self, delta):
        rec = _capi.Linearized6()
        fn, name = self._c_linearize
        _capi.check(fn(self._h, _pose16(delta), C.byref(rec)), name)
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
        """evaluate(delta) on the correspondences of the last linearise; without one they are computed at `delta` itself first (integrated_gicp_factor_impl.hpp
        :226-228, integrated_icp_factor_impl.hpp:188-190, integrated_colored_gicp_factor_impl.hpp:170-172: update_correspondences(delta) when none are stored)"""
        delta = self.calc_delta(values)
        if not getattr(self, "_linearized", False):
            self.linearization_point = np.asarray(delta, dtype=np.float64)
            self._linearized = True
        out = C.c_double()
        fn, name = self._c_error
        _capi.check(fn(self._h, _pose16(self.linearization_point), _pose16(delta), C.byref(out)), name)
        return out.value


class IntegratedGICPFactorGPU(_RelativePoseFactorGPU):
    """GICP matching-cost factor on the GPU: 1-NN correspondences within max_correspondence_distance (default 1 m,
    integrated_gicp_factor_impl.hpp:30), then the same residual / Jacobian algebra as VGICP."""

    _PREFIX = "gp_gicp_factor"

    def __init__(self, target_key, source_key, target: PointCloudGPU, source: PointCloudGPU, max_correspondence_distance=1.0, stream=None, _fixed_target_pose=None,
                 structure=0, counters=None):
        self._init_keys(target_key, source_key, _fixed_target_pose)
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
        self._adopt(h, stream)


class IntegratedICPFactorGPU(_RelativePoseFactorGPU):
    """ICP matching-cost factor on the GPU (IntegratedICPFactor_, impl/integrated_icp_factor_impl.hpp): 1-NN correspondences within max_correspondence_distance
    (default 1 m, :30), point-to-point residuals or, with use_point_to_plane, the reference's element-wise r = n_B o (mu_B - T p) on the target's normals.
    target_tree: a KdTreeGPU over `target` that many factors may share (held by reference, never rebuilt); None builds one and holds it (:47-51)."""

    _PREFIX = "gp_icp_factor"

    def __init__(self, target_key, source_key, target: PointCloudGPU, source: PointCloudGPU, target_tree=None, use_point_to_plane=False, max_correspondence_distance=1.0,
                 stream=None, _fixed_target_pose=None):
        self._init_keys(target_key, source_key, _fixed_target_pose)
        if target.points_gpu is None or (use_point_to_plane and target.normals_gpu is None):
            raise _capi.GPError("error: target frame doesn't have required attributes for icp")
        if source.points_gpu is None:
            raise _capi.GPError("error: source frame doesn't have required attributes for icp")
        self.target, self.source = target, source
        self.use_point_to_plane = bool(use_point_to_plane)
        self.target_tree = self._shared_tree(target, target_tree, stream)
        GaussianVoxelMapGPU._sync_torch(target)
        GaussianVoxelMapGPU._sync_torch(source)
        h = C.c_void_p()
        _capi.check(
            self._lib.gp_icp_factor_create(self.target_tree._h, target.ptr(target.points_gpu), target.ptr(target.normals_gpu) if use_point_to_plane else None, target.size(),
                                           source.ptr(source.points_gpu), source.size(), float(max_correspondence_distance) ** 2, int(self.use_point_to_plane), stream, C.byref(h)),
            "gp_icp_factor_create",
        )
        self._adopt(h, stream)

    def set_correspondence_update_tolerance(self, angle, trans):
        """keep the stored correspondences while a linearisation pose stays within (angle [rad], trans [m]) of the pose they were searched at (:128-141)"""
        self._call("set_correspondence_update_tolerance", float(angle), float(trans))


def IntegratedPointToPlaneICPFactorGPU(target_key, source_key, target, source, target_tree=None, max_correspondence_distance=1.0, stream=None, _fixed_target_pose=None):
    """IntegratedPointToPlaneICPFactor_ (factors/integrated_icp_factor.hpp): the ICP factor with use_point_to_plane = true"""
    return IntegratedICPFactorGPU(target_key, source_key, target, source, target_tree=target_tree, use_point_to_plane=True,
                                  max_correspondence_distance=max_correspondence_distance, stream=stream, _fixed_target_pose=_fixed_target_pose)


class IntegratedColoredGICPFactorGPU(_RelativePoseFactorGPU):
    """Colored GICP matching-cost factor on the GPU (IntegratedColoredGICPFactor_, impl/integrated_colored_gicp_factor_impl.hpp): GICP's geometric term on the 1-NN
    correspondences within max_correspondence_distance (default 1 m, :28) weighted 1 - photometric_term_weight, plus the photometric residual
    I_B - I_A - (P g_B) . (mu_B - T p_A) in the target's tangent plane weighted photometric_term_weight (default 0.25, :29).
    target_tree: a KdTreeGPU over `target` that many factors may share (None builds one): the 3-D search; or an IntensityKdTreeGPU over it: the correspondences are
    the nearest in (x, y, z, intensity) and max_correspondence_distance bounds the 4-D distance (:121-127).  target_gradients: an IntensityGradientsGPU of `target`;
    None estimates it with k = 10."""

    _PREFIX = "gp_colored_gicp_factor"

    def __init__(self, target_key, source_key, target: PointCloudGPU, source: PointCloudGPU, target_tree=None, target_gradients=None, max_correspondence_distance=1.0,
                 photometric_term_weight=0.25, stream=None, _fixed_target_pose=None):
        self._init_keys(target_key, source_key, _fixed_target_pose)
        if target.points_gpu is None or target.covs_gpu is None or target.normals_gpu is None or target.intensities_gpu is None:
            raise _capi.GPError("error: target frame doesn't have required attributes for colored_gicp")  # :37-40
        if source.points_gpu is None or source.covs_gpu is None or source.intensities_gpu is None:
            raise _capi.GPError("error: source frame doesn't have required attributes for colored_gicp")  # :42-45
        self.target, self.source = target, source
        self.target_tree = self._photometric_tree(target, target_tree, stream)
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
        self._adopt(h, stream)
        if self._searches_xyzi():
            self._call("set_intensity_grid", self.target_tree._xyzi)

    def set_photometric_term_weight(self, weight):
        self._call("set_photometric_term_weight", float(weight))

    def set_max_correspondence_distance(self, dist):
        self._call("set_max_correspondence_distance", float(dist))

    def set_correspondence_update_tolerance(self, angle, trans):
        """keep the stored correspondences while a linearisation pose stays within (angle [rad], trans [m]) of the pose they were searched at (:101-114)"""
        self._call("set_correspondence_update_tolerance", float(angle), float(trans))


class IntegratedColorConsistencyFactorGPU(_RelativePoseFactorGPU):
    """Color consistency matching-cost factor on the GPU (IntegratedColorConsistencyFactor_, impl/integrated_color_consistency_factor_impl.hpp): the photometric
    residual I_B - I_A - (P g_B) . (mu_B - T p_A) alone, weighted photometric_term_weight (default 1.0, :31), on the 1-NN correspondences within
    max_correspondence_distance (default 1 m, :30).  No covariances are needed.  target_tree: a KdTreeGPU over `target` (None builds one) -- the 3-D search, what the
    reference does when handed a plain KdTree -- or an IntensityKdTreeGPU: the nearest in (x, y, z, intensity), the cut-off on the 4-D distance.  target_gradients:
    an IntensityGradientsGPU of `target`; None estimates it with k = 10.  Not a member of CorrespondenceFactorBatchGPU or the LM graph yet."""

    _PREFIX = "gp_color_consistency_factor"

    def __init__(self, target_key, source_key, target: PointCloudGPU, source: PointCloudGPU, target_tree=None, target_gradients=None, max_correspondence_distance=1.0,
                 photometric_term_weight=1.0, stream=None, _fixed_target_pose=None):
        self._init_keys(target_key, source_key, _fixed_target_pose)
        # (the reference's texts say colored_gicp in this factor too, :37-45)
        if target.points_gpu is None or target.normals_gpu is None or target.intensities_gpu is None:
            raise _capi.GPError("error: target frame doesn't have required attributes for colored_gicp")
        if source.points_gpu is None or source.intensities_gpu is None:
            raise _capi.GPError("error: source frame doesn't have required attributes for colored_gicp")
        self.target, self.source = target, source
        self.target_tree = self._photometric_tree(target, target_tree, stream)
        self.target_gradients = target_gradients if target_gradients is not None else estimate_intensity_gradients_gpu(target, 10, stream=stream)
        if self.target_gradients.size() != target.size():
            raise _capi.GPError("error: target_gradients does not have one gradient per target point")
        GaussianVoxelMapGPU._sync_torch(target)
        GaussianVoxelMapGPU._sync_torch(source)
        h = C.c_void_p()
        _capi.check(
            self._lib.gp_color_consistency_factor_create(self.target_tree._h, target.ptr(target.points_gpu), target.ptr(target.normals_gpu), target.ptr(target.intensities_gpu),
                                                         C.c_void_p(self.target_gradients.gradients_gpu.data_ptr()), target.size(), source.ptr(source.points_gpu),
                                                         source.ptr(source.intensities_gpu), source.size(), float(max_correspondence_distance) ** 2,
                                                         float(photometric_term_weight), stream, C.byref(h)),
            "gp_color_consistency_factor_create",
        )
        self._adopt(h, stream)
        if self._searches_xyzi():
            self._call("set_intensity_grid", self.target_tree._xyzi)

    def set_photometric_term_weight(self, weight):
        self._call("set_photometric_term_weight", float(weight))

    def set_max_correspondence_distance(self, dist):
        self._call("set_max_correspondence_distance", float(dist))

    def set_correspondence_update_tolerance(self, angle, trans):
        """keep the stored correspondences while a linearisation pose stays within (angle [rad], trans [m]) of the pose they were searched at (:101-114)"""
        self._call("set_correspondence_update_tolerance", float(angle), float(trans))


class IntegratedLOAMFactorGPU(_RelativePoseFactorGPU):
    """LOAM matching-cost factor on the GPU (IntegratedLOAMFactor_, impl/integrated_loam_factor_impl.hpp): a point-to-edge part on the 2 nearest edge points and a
    point-to-plane part on the 3 nearest plane points within max_correspondence_distance (default 1 m each), their records added edge first.
    target_edges_tree / target_planes_tree: KdTreeGPUs over the target clouds that many factors may share (held by reference); None builds one and holds it."""

    _PREFIX = "gp_loam_factor"
    _LOAM = "error: {} frame doesn't have required attributes for loam"
    _EDGE = "error: target or source points has not been allocated!!"

    def __init__(self, target_key, source_key, target_edges, target_planes, source_edges, source_planes, target_edges_tree=None, target_planes_tree=None,
                 max_correspondence_distance=1.0, stream=None, _fixed_target_pose=None):
        self._init_keys(target_key, source_key, _fixed_target_pose)
        # the reference constructs the edge factor first (:387-390); each aborts with its own text
        if target_edges is not None and (target_edges.points_gpu is None or source_edges.points_gpu is None):
            raise _capi.GPError(self._EDGE)
        if target_planes is not None:
            if target_planes.points_gpu is None:
                raise _capi.GPError(self._LOAM.format("target"))
            if source_planes.points_gpu is None:
                raise _capi.GPError(self._LOAM.format("source"))
        self.target_edges, self.source_edges, self.target_planes, self.source_planes = target_edges, source_edges, target_planes, source_planes
        self.target_edges_tree = self._shared_tree(target_edges, target_edges_tree, stream)
        self.target_planes_tree = self._shared_tree(target_planes, target_planes_tree, stream)
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
        self._adopt(h, stream)
        if max_correspondence_distance != 1.0:
            self.set_max_correspondence_distance(max_correspondence_distance, max_correspondence_distance)

    def set_max_correspondence_distance(self, dist_edge, dist_plane):
        self._call("set_max_correspondence_distance", float(dist_edge), float(dist_plane))

    def set_enable_correspondence_validation(self, enable):
        """validate_correspondences (:487-529): drop edge pairs / plane triples that lie in one scan line (off by default)"""
        self._call("set_enable_correspondence_validation", int(bool(enable)))

    def set_correspondence_update_tolerance(self, angle, trans):
        self._call("set_correspondence_update_tolerance", float(angle), float(trans))

    def num_correspondences(self):
        """(edges, planes) of the last linearise"""
        e, p = C.c_int(0), C.c_int(0)
        self._call("num_correspondences", C.byref(e), C.byref(p))
        return e.value, p.value

    def correspondences(self):
        """(edges (n, 2) or None, planes (n, 3) or None): the stored correspondences copied to the host, per source point the target indices in ascending order of
        distance, a row of -1 where the point has none (read-only; for tests and diagnosis)"""
        out = []
        for src, K in ((self.source_edges, 2), (self.source_planes, 3)):
            out.append(None if src is None else np.full((K, src.size()), -1, dtype=np.int32))
        self._call("get_correspondences", *[None if a is None else a.ctypes.data for a in out])
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


class IntegratedCTICPFactorGPU(_CorrFactorGPU):
    """Continuous-time ICP factor on the GPU (IntegratedCT_ICPFactor_, impl/integrated_ct_icp_factor_impl.hpp): the source was scanned while the sensor moved from
    the pose of source_t0_key to that of source_t1_key; every point is transformed by the pose interpolated at its own time stamp (source.times_gpu, grouped into
    bins 1e-3 apart, :41-55) and matched to its nearest target point within max_correspondence_distance (default 1 m, :27).  The residual is the scalar
    point-to-plane distance on the target's normals.  target_tree: a KdTreeGPU over `target` that many factors may share; None builds one and holds it (:57-61)."""

    _PREFIX = "gp_ct_factor"
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
        self.target_tree = self._shared_tree(target, target_tree, stream)
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
        self._adopt(h, stream)

    @staticmethod
    def _check_attributes(target, source):
        if target.normals_gpu is None:
            raise _capi.GPError("error: target cloud doesn't have normals!!")  # (the reference aborts with this at the first linearise, :133-136)

    def _poses(self, values):
        return _pose16(values[self._keys[0]]), _pose16(values[self._keys[1]])

    def linearize(self, values):
        """update_poses + update_correspondences + the sums -> HessianFactor(k0, k1, H_00, H_01, -b_0, H_11, -b_1, error) (:132-199)"""
        rec = _capi.Linearized6()
        fn, name = self._c_linearize
        _capi.check(fn(self._h, *self._poses(values), C.byref(rec)), name)
        l = LinearizedSystem6(rec)
        self._num_inliers = l.num_inliers
        return HessianFactor(self._keys, {(0, 0): l.H_target, (0, 1): l.H_target_source, (1, 1): l.H_source}, [-l.b_target, -l.b_source], l.error)

    def error(self, values):
        """the error at `values` on the stored correspondences; without any they are searched at `values` first (:92-96)"""
        out = C.c_double()
        fn, name = self._c_error
        _capi.check(fn(self._h, *self._poses(values), C.byref(out)), name)
        return out.value

    def time_table(self):
        """(normalised time of every bin float64 [bins], bin of every source point int32 [n])"""
        table = np.zeros(self._lib.gp_ct_factor_num_time_bins(self._h), dtype=np.float64)
        indices = np.zeros(self.source.size(), dtype=np.int32)
        self._call("time_table", table.ctypes.data, indices.ctypes.data)
        return table, indices

    def pose_table(self):
        """(T [bins, 3, 4], D0 [bins, 6, 6], D1 [bins, 6, 6]) of the last linearise (read-only; for tests and diagnosis)"""
        rows = np.zeros((self._lib.gp_ct_factor_num_time_bins(self._h), 84), dtype=np.float64)
        self._call("pose_table", rows.ctypes.data)
        return rows[:, :12].reshape(-1, 3, 4), rows[:, 12:48].reshape(-1, 6, 6), rows[:, 48:].reshape(-1, 6, 6)

    def correspondences(self):
        """the stored correspondences int32 [n], -1 where a point has none (read-only; for tests and diagnosis)"""
        out = np.full(self.source.size(), -1, dtype=np.int32)
        self._call("correspondences", out.ctypes.data)
        return out

    def deskewed_source_points(self, values, local=False):
        """T(t_i) p_i -- or T0^-1 T(t_i) p_i when `local` -- as float64 [n, 4], last component 1 (:290-308)"""
        import torch

        out = torch.empty((self.source.size(), 4), dtype=torch.float64, device=self.source.device)
        torch.cuda.current_stream(self.source.device).synchronize()
        self._call("deskew", *self._poses(values), int(bool(local)), C.c_void_p(out.data_ptr()))
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
        # what the batch's one 3-D search launch and its term tables do not serve yet is refused, never searched in 3-D instead
        for f in self.factors:
            if isinstance(f, IntegratedColorConsistencyFactorGPU):
                raise _capi.GPError("CorrespondenceFactorBatchGPU: an IntegratedColorConsistencyFactorGPU cannot join a batch or an LM graph yet")
            if isinstance(f, IntegratedColoredGICPFactorGPU) and f._searches_xyzi():
                raise _capi.GPError("CorrespondenceFactorBatchGPU: an IntegratedColoredGICPFactorGPU on an IntensityKdTreeGPU (XYZI search) cannot join a batch or an LM "
                                    "graph yet: the batch searches in 3-D")
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

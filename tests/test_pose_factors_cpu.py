"""CPU checks of the pose factors (gp_pose_factors_*, gp_lm_graph_create_with_pose_factors): the struct layout, every argument refusal -- made on the host before any
device work --, the numpy statement of Pose3 against its own identities, and the kernel's resources (no scratch, no spills)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pose3_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = os.path.join(ROOT, "gtsam_points_amd", "csrc", "gp_pose_factors.resources.txt")
INVALID = 1  # GP_ERROR_INVALID_ARGUMENT


def _lib():
    from gtsam_points_amd import _capi

    return _capi, _capi.load()


def _factors(*specs):
    _capi, _ = _lib()
    arr = (_capi.PoseFactor * max(len(specs), 1))()
    for i, (kind, a, b) in enumerate(specs):
        arr[i].kind, arr[i].pose_a, arr[i].pose_b = kind, a, b
        arr[i].measured[:] = np.eye(4).reshape(16)
        arr[i].information[:] = np.eye(6).reshape(36)
    return arr


def test_struct_matches_the_header():
    _capi, _ = _lib()
    assert C.sizeof(_capi.PoseFactor) == 432
    assert _capi.PoseFactor.measured.offset == 16 and _capi.PoseFactor.information.offset == 144
    hdr = open(os.path.join(ROOT, "include", "gtsam_points_hip.h")).read()
    assert "#define GP_POSE_FACTOR_BETWEEN 0" in hdr and "#define GP_POSE_FACTOR_PRIOR 1" in hdr


def _refusals():
    """(name, factors, num_poses) that create must refuse"""
    out = []
    out.append(("pose_a out of range", _factors((0, 5, 1)), 4))
    out.append(("pose_b out of range", _factors((0, 0, 4)), 4))
    out.append(("negative pose", _factors((1, -1, -1)), 4))
    out.append(("between a = b", _factors((0, 2, 2)), 4))
    out.append(("unknown kind", _factors((2, 0, 1)), 4))
    out.append(("prior with pose_b", _factors((1, 0, 1)), 4))
    f = _factors((0, 0, 1))
    f[0].measured[0] = 1.001  # not orthonormal
    out.append(("non-rigid measured", f, 4))
    f = _factors((1, 0, -1))
    f[0].measured[:] = np.diag([1.0, 1.0, -1.0, 1.0]).reshape(16)  # a reflection
    out.append(("reflection", f, 4))
    f = _factors((0, 0, 1))
    f[0].information[7] = float("nan")
    out.append(("non-finite information", f, 4))
    f = _factors((0, 0, 1))
    f[0].information[1] = 1e-6  # (0, 1) but not (1, 0)
    out.append(("asymmetric information", f, 4))
    return out


@pytest.mark.parametrize("case", range(10))
def test_create_refuses_without_a_device(case):
    """every refusal of gp_pose_factors_create and gp_lm_graph_create_with_pose_factors is GP_ERROR_INVALID_ARGUMENT, returned before any device work (no GPU here)"""
    _capi, lib = _lib()
    name, arr, n = _refusals()[case]
    h = C.c_void_p()
    assert lib.gp_pose_factors_create(arr, 1, n, None, C.byref(h)) == INVALID and not h.value, name
    assert lib.gp_lm_graph_create_with_pose_factors(None, None, arr, 1, n, None, 4, None, C.byref(h)) == INVALID and not h.value, name


def test_symmetry_is_relative_and_graph_needs_factors():
    _capi, lib = _lib()
    h = C.c_void_p()
    # a graph with neither VGICP nor pose factors
    assert lib.gp_lm_graph_create_with_pose_factors(None, None, None, 0, 4, None, 4, None, C.byref(h)) == INVALID and not h.value
    assert lib.gp_lm_graph_create_with_pose_factors(None, None, _factors((1, 0, -1)), 1, 1, None, 4, None, None) == INVALID  # null out
    assert lib.gp_pose_factors_create(_factors((1, 0, -1)), 1, 0, None, C.byref(h)) == INVALID  # no poses
    assert lib.gp_pose_factors_create(_factors((1, 0, -1)), -1, 1, None, C.byref(h)) == INVALID
    assert lib.gp_pose_factors_size(None) == 0 and lib.gp_pose_factors_destroy(None) == 0
    for fn in (lib.gp_pose_factors_linearize, lib.gp_pose_factors_compute_error, lib.gp_pose_factors_issue_linearize_dev, lib.gp_pose_factors_issue_compute_error_dev):
        assert fn(None, None, None) == INVALID


def test_python_factor_classes_without_a_device():
    import gtsam_points_amd as gpa

    f = gpa.BetweenFactorPose3(2, 3, np.eye(4), sigmas=[0.1, 0.1, 0.1, 0.5, 0.5, 0.5])
    assert np.allclose(f.information, np.diag([100.0] * 3 + [4.0] * 3))
    s = f._struct()
    assert (s.kind, s.pose_a, s.pose_b) == (0, 2, 3)
    p = gpa.PriorFactorPose3(1, np.eye(4), information=1e6 * np.eye(6))
    s = p._struct()
    assert (s.kind, s.pose_a, s.pose_b) == (1, 1, -1) and s.information[0] == 1e6
    assert np.array_equal(gpa.BetweenFactorPose3(0, 1, np.eye(4)).information, np.eye(6))  # neither: the unit model
    with pytest.raises(ValueError):
        gpa.BetweenFactorPose3(0, 1, np.eye(4), information=np.eye(6), sigmas=np.ones(6))


def test_reference_statement_identities():
    """the numpy statement itself: Logmap inverts Expmap on every SO3::Logmap branch; AdjointMap moves a twist through T (T Exp(xi) T^-1 = Exp(Ad_T xi))"""
    rng = np.random.default_rng(3)
    for th in (0.0, 1e-12, 1e-7, 0.3, 2.0, np.pi - 1e-4, np.pi - 1e-7):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        xi = np.concatenate([th * axis, rng.normal(size=3)])
        back = pose3_ref.pose3_logmap(pose3_ref.expmap(xi))
        assert np.allclose(back, xi, atol=1e-6 if th > 3 else 1e-12), (th, back, xi)
    T = pose3_ref.expmap(rng.normal(size=6))
    xi = 1e-3 * rng.normal(size=6)
    lhs = T @ pose3_ref.expmap(xi) @ pose3_ref.inverse(T)
    assert np.allclose(lhs, pose3_ref.expmap(pose3_ref.adjoint(T) @ xi), atol=1e-12)


def test_kernel_has_no_scratch_and_no_spills():
    assert os.path.exists(RES), "build the HIP library first (python -c 'import __graft_entry__ as g; g.build()')"
    txt = open(RES).read()
    blocks = {b.split()[0]: b for b in txt.split("remark: Function Name: ")[1:]}
    ks = {k: v for k, v in blocks.items() if "pose_factors_kernel" in k}
    assert len(ks) == 1
    for name, b in ks.items():
        get = lambda key: int(re.search(re.escape(key) + r":\s+(\d+)", b).group(1))  # noqa: E731
        assert get("ScratchSize [bytes/lane]") == 0 and get("VGPRs Spill") == 0 and get("SGPRs Spill") == 0, name
        assert get("Occupancy [waves/SIMD]") >= 4, name

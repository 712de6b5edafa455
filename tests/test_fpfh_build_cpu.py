"""CPU checks of the FPFH unit's build products: every kernel of csrc/gp_fpfh.hip as the compiler's resource remarks list them, none with scratch or spills; the
defaults of gp_fpfh_params; and the argument refusals that are made on the host before any device work."""
import ctypes as C
import os

from test_icp_build_cpu import ROOT, _assert_no_scratch

RES = os.path.join(ROOT, "gtsam_points_amd", "csrc", "gp_fpfh.resources.txt")


def test_every_kernel_of_the_unit_uses_no_scratch():
    assert os.path.exists(RES), "build the HIP library first (python -c 'import __graft_entry__ as g; g.build()')"
    ks = {b.split()[0]: b for b in open(RES).read().split("remark: Function Name: ")[1:]}
    for name in ("fpfh_insert_kernel", "fpfh_gather_kernel", "fpfh_spfh_kernel", "fpfh_fpfh_kernel"):
        assert sum(name in k for k in ks) == 1, name
    assert not any("radix_" in k for k in ks)  # the sort's kernels live in gp_cloud_filter.hip (gp::sort_indices_by_key)
    _assert_no_scratch(ks)  # every kernel the unit emits, the helpers its headers instantiate included


def test_defaults_are_the_reference_values():
    from gtsam_points_amd import FPFHEstimationParams, _capi

    p = _capi.FpfhParams()
    _capi.load().gp_fpfh_params_default(C.byref(p))
    assert (p.search_radius, p.max_num_neighbors) == (5.0, 10000)  # features/fpfh_estimation.hpp:60-64
    q = FPFHEstimationParams()
    assert (q.search_radius, q.max_num_neighbors) == (5.0, 10000)
    assert _capi.GP_FPFH_DIM == 33


def test_the_entry_point_refuses_bad_arguments_without_a_device():
    from gtsam_points_amd import _capi

    lib = _capi.load()
    fake = C.c_void_p(64)  # never dereferenced
    cut = C.c_int(0)

    def call(points=fake, normals=fake, n=10, params="default", num_indices=0, out=fake, out32=None, spfh=None, **kw):
        p = _capi.FpfhParams()
        lib.gp_fpfh_params_default(C.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.gp_estimate_fpfh(points, normals, n, C.byref(p) if params == "default" else None, None, num_indices, out, out32, spfh, None, C.byref(cut), None)

    assert call(params=None) == 1 and b"params is NULL" in lib.gp_last_error()
    assert call(points=None) == 1 and b"points or normals is NULL" in lib.gp_last_error()
    assert call(normals=None) == 1 and b"points or normals is NULL" in lib.gp_last_error()
    assert call(n=0) == 1 and b"n must be positive" in lib.gp_last_error()
    assert call(n=-3) == 1 and b"n must be positive" in lib.gp_last_error()
    for radius in (0.0, -1.0, float("inf"), float("nan")):
        assert call(search_radius=radius) == 1 and b"search_radius" in lib.gp_last_error()
    assert call(max_num_neighbors=0) == 1 and b"max_num_neighbors" in lib.gp_last_error()
    assert call(num_indices=-1) == 1 and b"num_indices" in lib.gp_last_error()
    assert call(out=None) == 1 and b"no output" in lib.gp_last_error()
    assert b"gp_estimate_fpfh" in lib.gp_last_error()

"""CPU checks of the ICP and GICP factors' build products: the tile kernels' resources as the compiler reports them (no scratch, no spills) and the argument refusals
that are made on the host before any device work."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = os.path.join(ROOT, "gtsam_points_amd", "csrc", "gp_corr_factors.resources.txt")


def _tile_kernels(term):
    """the compiler's remarks on the instantiations of corr_tile_kernel<MODE, TERM> whose (mangled) TERM contains `term`"""
    assert os.path.exists(RES), "build the HIP library first (python -c 'import __graft_entry__ as g; g.build()')"
    blocks = {b.split()[0]: b for b in open(RES).read().split("remark: Function Name: ")[1:]}
    return {k: v for k, v in blocks.items() if "corr_tile_kernel" in k and term in k}


def _assert_no_scratch(ks):
    for name, b in ks.items():
        get = lambda key: int(re.search(re.escape(key) + r":\s+(\d+)", b).group(1))  # noqa: E731
        assert get("ScratchSize [bytes/lane]") == 0 and get("VGPRs Spill") == 0 and get("SGPRs Spill") == 0, name


def test_icp_tile_kernels_use_no_scratch():
    ks = _tile_kernels("IcpTerm")
    assert len(ks) == 6  # {linearise, error, general linearise} x {point-to-point, point-to-plane}
    _assert_no_scratch(ks)


def test_gicp_tile_kernels_use_no_scratch():
    ks = _tile_kernels("GicpTerm")
    assert len(ks) == 3  # linearise, error, general linearise
    _assert_no_scratch(ks)


def test_icp_entry_points_refuse_bad_arguments_without_a_device():
    from gtsam_points_amd import _capi

    lib = _capi.load()
    h = C.c_void_p()
    fake = C.c_void_p(64)  # never dereferenced: the NULL grid is refused first
    assert lib.gp_icp_factor_create(None, fake, None, 1, fake, 1, 1.0, 0, None, C.byref(h)) == 1 and not h.value  # GP_ERROR_INVALID_ARGUMENT
    assert b"gp_icp_factor_create" in lib.gp_last_error()
    assert lib.gp_icp_factor_destroy(None) == 0 and lib.gp_icp_factor_num_correspondences(None) == 0
    assert lib.gp_icp_factor_linearize(None, None, None) == 1 and lib.gp_icp_factor_compute_error(None, None, None, None) == 1
    assert lib.gp_icp_factor_set_correspondence_update_tolerance(None, 0.1, 0.1) == 1

"""CPU checks of the correspondence batch's build products for the colored GICP kind: the batch tile kernel is instantiated with ColoredGicpTerm exactly three times
(linearise, error, general linearise) and the compiler reports no scratch and no spills for any of them -- the single-factor colored tile kernels meet that
(test_colored_build_cpu.py), and the batched form only adds the look-up of the tile, the descriptor and the poses in front of the point loop."""
import ctypes as C
import os

from test_icp_build_cpu import ROOT, _assert_no_scratch

RES = os.path.join(ROOT, "gtsam_points_amd", "csrc", "gp_corr_batch.resources.txt")


def _kernels():
    assert os.path.exists(RES), "build the HIP library first (python -c 'import __graft_entry__ as g; g.build()')"
    return {b.split()[0]: b for b in open(RES).read().split("remark: Function Name: ")[1:]}


def test_colored_batch_tile_kernels_use_no_scratch():
    ks = {k: v for k, v in _kernels().items() if "batch_tiles_kernel" in k and "ColoredGicpTerm" in k}
    assert len(ks) == 3, sorted(ks)  # linearise, error, general linearise
    _assert_no_scratch(ks)


def test_other_batch_tile_kernels_are_still_instantiated():
    """the GICP and the two ICP terms keep their three batch tile kernels each, the two LOAM terms theirs"""
    tiles = [k for k in _kernels() if "batch_tiles_kernel" in k]
    assert len([k for k in tiles if "ColoredGicpTerm" not in k and "GicpTerm" in k]) == 3
    assert len([k for k in tiles if "IcpTerm" in k]) == 6
    assert len([k for k in tiles if "Loam" in k]) == 6
    assert len(tiles) == 18


def test_create_with_colored_members_refuses_bad_arguments_without_a_device():
    from gtsam_points_amd import _capi

    lib = _capi.load()
    assert "gp_corr_batch_create_ex2" in _capi.EXPORTED_SYMBOLS
    h = C.c_void_p()
    null = (C.c_void_p * 1)(None)
    assert lib.gp_corr_batch_create_ex2(None, 0, None, 0, None, 0, None, 0, None, C.byref(h)) == 1 and not h.value  # GP_ERROR_INVALID_ARGUMENT: an empty batch
    assert lib.gp_corr_batch_create_ex2(None, 0, None, 0, None, 0, None, 1, None, C.byref(h)) == 1 and not h.value  # a count without the array
    assert lib.gp_corr_batch_create_ex2(None, 0, None, 0, None, 0, null, -1, None, C.byref(h)) == 1 and not h.value  # a negative count
    assert lib.gp_corr_batch_create_ex2(None, 0, None, 0, None, 0, null, 1, None, C.byref(h)) == 1 and not h.value  # a NULL member
    assert b"null colored GICP factor" in lib.gp_last_error()
    assert lib.gp_corr_batch_create_ex2(None, 0, None, 0, None, 0, null, 1, None, None) == 1  # no place for the handle

"""CPU checks of the correspondence batch's build products for the colored GICP kind: the batch tile kernel is instantiated with ColoredGicpTerm exactly three times
(linearise, error, general linearise) and the compiler reports no scratch and no spills for any of them -- the single-factor colored tile kernels meet that
(test_colored_build_cpu.py), and the batched form only adds the look-up of the tile, the descriptor and the poses in front of the point loop."""
import ctypes as C
import os
import re

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


# The six LOAM instantiations of corr_batch_tiles_kernel<MODE, TERM, LoamBatchDesc> against the figures of loam_batch_tiles_kernel<MODE, TERM>, the kernel they were
# before they joined the template (HIP 7.2 / AMD clang 22, gfx950), as upper bounds: (MODE, term) -> SGPRs (the remarks' TotalSGPRs), VGPRs, AGPRs, LDS bytes per workgroup; scratch and spills none.
# The build this came with sits on every figure: the merged kernels are the separate ones instruction for instruction.
LOAM_BOUNDS = {
    (0, "LoamEdgeTerm"): (50, 118, 0, 13312),
    (0, "LoamPlaneTerm"): (52, 124, 0, 13312),
    (1, "LoamEdgeTerm"): (50, 46, 0, 13312),
    (1, "LoamPlaneTerm"): (52, 60, 0, 13312),
    (2, "LoamEdgeTerm"): (50, 256, 24, 15360),
    (2, "LoamPlaneTerm"): (50, 256, 40, 15360),
}


def test_loam_batch_tile_kernels_keep_the_figures_of_their_own_kernel():
    ks = _kernels()
    assert not any("loam_batch_tiles_kernel" in k for k in ks)  # one template
    for (mode, term), (sgprs, vgprs, agprs, lds) in LOAM_BOUNDS.items():
        (name,) = [k for k in ks if f"corr_batch_tiles_kernelILi{mode}ENS_{len(term)}{term}ENS_13LoamBatchDescE" in k]
        get = lambda key: int(re.search(re.escape(key) + r":\s+(\d+)", ks[name]).group(1))  # noqa: E731
        got = (get("TotalSGPRs"), get("    VGPRs"), get("    AGPRs"), get("LDS Size [bytes/block]"))
        print(name, got)
        assert got[0] <= sgprs and got[1] <= vgprs and got[2] <= agprs and got[3] <= lds, (name, got)
        _assert_no_scratch({name: ks[name]})


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

"""CPU checks of the continuous-time factors' build products: the unit's kernels as the compiler's resource remarks list them, none with scratch or spills."""
import os

from test_icp_build_cpu import ROOT, _assert_no_scratch

RES = os.path.join(ROOT, "gtsam_points_amd", "csrc", "gp_ct_factors.resources.txt")


def _kernels():
    assert os.path.exists(RES), "build the HIP library first (python -c 'import __graft_entry__ as g; g.build()')"
    return {b.split()[0]: b for b in open(RES).read().split("remark: Function Name: ")[1:]}


def test_unit_holds_exactly_its_seven_kernels():
    """the pose table, the search, the deskew and the tile kernel as {linearise, error} x {CT-ICP, CT-GICP}: seven -- beside host_flag_kernel, which gp_host.hpp's
    HostWords brings into every unit that includes it"""
    ks = _kernels()
    own = {k for k in ks if "ct_" in k}
    assert len(own) == 7 and set(ks) - own == {k for k in ks if "host_flag_kernel" in k} and len(ks) <= 8, sorted(ks)
    for name in ("ct_pose_table_kernel", "ct_nearest_kernel", "ct_deskew_kernel"):
        assert sum(name in k for k in own) == 1, name
    tiles = {k for k in own if "ct_tile_kernel" in k}
    assert len(tiles) == 4 and sum("CtIcpTerm" in k for k in tiles) == 2 and sum("CtGicpTerm" in k for k in tiles) == 2
    assert sum("ILi1E" in k for k in tiles) == 2 and sum("ILi2E" in k for k in tiles) == 2  # MODE_ERR = 1, MODE_LIN_GENERAL = 2


def test_every_kernel_uses_no_scratch():
    _assert_no_scratch(_kernels())

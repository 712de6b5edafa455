"""CPU checks of the colored GICP unit's build products: the resources of its tile kernels and of the intensity-gradient kernel as the compiler reports them
(no scratch, no spills)."""
import os
import re

from test_icp_build_cpu import ROOT, _assert_no_scratch

RES = os.path.join(ROOT, "gtsam_points_amd", "csrc", "gp_colored_factors.resources.txt")


def _kernels():
    assert os.path.exists(RES), "build the HIP library first (python -c 'import __graft_entry__ as g; g.build()')"
    return {b.split()[0]: b for b in open(RES).read().split("remark: Function Name: ")[1:]}


def test_colored_tile_kernels_use_no_scratch():
    tiles = {k: v for k, v in _kernels().items() if "corr_tile_kernel" in k}
    ks = {k: v for k, v in tiles.items() if "ColoredGicpTerm" in k}
    assert len(ks) == 3 and len(tiles) == 3  # linearise, error, general linearise -- and the unit instantiates the tile kernel with no other term
    _assert_no_scratch(ks)


def test_gradient_kernel_uses_no_scratch():
    ks = {k: v for k, v in _kernels().items() if "intensity_gradient_kernel" in k}
    assert len(ks) == 1
    assert int(re.search(r"ScratchSize \[bytes/lane\]:\s+(\d+)", next(iter(ks.values()))).group(1)) == 0
    _assert_no_scratch(ks)

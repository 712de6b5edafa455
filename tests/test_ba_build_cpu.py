"""CPU checks of the bundle-adjustment unit's build products: its kernels as the compiler's resource remarks list them, none with scratch or spills."""
import os

from test_icp_build_cpu import ROOT, _assert_no_scratch

RES = os.path.join(ROOT, "gtsam_points_amd", "csrc", "gp_ba_factors.resources.txt")


def _kernels():
    assert os.path.exists(RES), "build the HIP library first (python -c 'import __graft_entry__ as g; g.build()')"
    return {b.split()[0]: b for b in open(RES).read().split("remark: Function Name: ")[1:]}


def test_unit_holds_exactly_its_three_kernels():
    """the feature kernel as {linearise, error only} and the record gather: three -- beside host_flag_kernel, which gp_host.hpp's HostWords brings into every unit
    that includes it"""
    ks = _kernels()
    own = {k for k in ks if "ba_" in k}
    assert len(own) == 3 and set(ks) - own == {k for k in ks if "host_flag_kernel" in k} and len(ks) <= 4, sorted(ks)
    assert sum("ba_feature_kernelILb1E" in k for k in own) == 1 and sum("ba_feature_kernelILb0E" in k for k in own) == 1
    assert sum("ba_records_kernel" in k for k in own) == 1


def test_every_kernel_uses_no_scratch():
    _assert_no_scratch(_kernels())

"""CPU checks of the block-sparse solver's build products: the kernels' resources as the compiler reports them, and the symbolic unit free of device code."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gtsam_points_amd", "csrc")


def _kernel(unit, name):
    """the compiler's remarks on the one kernel of `unit` whose (mangled) name contains `name`, as {key: int}"""
    res = os.path.join(CSRC, unit + ".resources.txt")
    assert os.path.exists(res), "build the HIP library first (python -c 'import __graft_entry__ as g; g.build()')"
    blocks = [b for b in open(res).read().split("remark: Function Name: ")[1:] if name in b.split()[0]]
    assert len(blocks) == 1, (name, [b.split()[0] for b in blocks])
    return {k: int(re.search(re.escape(k) + r":\s+(\d+)", blocks[0]).group(1)) for k in ("VGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill")}


def test_one_launch_step_keeps_its_rows_in_registers():
    """eight waves of up to 256 registers: a lone wave's panel rows live in registers, without scratch (gp_sparse_small_lds.hpp: kSmallThreads)"""
    k = _kernel("gp_sparse_small", "sparse_small_step_kernel")
    assert k["ScratchSize [bytes/lane]"] == 0 and k["VGPRs Spill"] == 0 and k["VGPRs"] <= 256, k


def test_multi_launch_kernels_use_no_scratch():
    # (sparse_factor_staged_kernel<1024> is exempt: 36 B/lane under its 128-register cap)
    for name in ("sparse_factor_kernelILi256E", "sparse_backsolve_kernel"):
        assert _kernel("gp_sparse", name)["ScratchSize [bytes/lane]"] == 0, name


def test_symbolic_unit_holds_no_device_code():
    src = open(os.path.join(CSRC, "gp_sparse_symbolic.hip")).read() + open(os.path.join(CSRC, "gp_sparse_symbolic.hpp")).read()
    assert not re.search(r"__global__|__device__|\bhip[A-Z]\w*\(|GP_HIP\(", src)

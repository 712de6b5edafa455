"""CPU checks of the build products of the incremental voxel-map insert: its kernels as the compiler reports them for gfx950 -- present, no scratch, no spills."""
import os
import re

from test_icp_build_cpu import ROOT, _assert_no_scratch

CSRC = os.path.join(ROOT, "gtsam_points_amd", "csrc")
NEW_KERNELS = ("segmented_sums_kernel", "survivors_bbox_kernel", "grid_mark_survivors_kernel", "merge_source_kernel", "merge_finalize_kernel")
SHARED_KERNELS = ("grid_count_kernel", "insert_voxels_kernel", "line_claim_kernel")  # launched by this unit too


def _kernels(unit):
    path = os.path.join(CSRC, unit + ".resources.txt")
    assert os.path.exists(path), "build the HIP library first (python -c 'import __graft_entry__ as g; g.build()')"
    return {b.split()[0]: b for b in open(path).read().split("remark: Function Name: ")[1:]}


def _get(block, key):
    return int(re.search(re.escape(key) + r":\s+(\d+)", block).group(1))


def test_incremental_insert_kernels_use_no_scratch():
    ks = _kernels("gp_voxelmap_incremental")
    for name in NEW_KERNELS + SHARED_KERNELS:
        found = {k: v for k, v in ks.items() if name in k}
        assert len(found) == 1, name
        _assert_no_scratch(found)
    _assert_no_scratch(ks)  # nor does any other kernel the unit holds
    # the frame's sums are the one-shot build's segmented sum without its finalize: no more registers than that kernel
    stats = [v for k, v in ks.items() if "segmented_stats_kernel" in k]
    sums = [v for k, v in ks.items() if "segmented_sums_kernel" in k]
    assert len(stats) == 1 and _get(sums[0], "VGPRs") <= _get(stats[0], "VGPRs")
    for name in ("segmented_sums_kernel", "merge_finalize_kernel"):
        b = [v for k, v in ks.items() if name in k][0]
        print(f"[incremental map] {name}: {_get(b, 'VGPRs')} VGPRs, {_get(b, 'Occupancy [waves/SIMD]')} waves/SIMD")

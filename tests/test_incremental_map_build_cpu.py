"""CPU checks of the build products of the voxel-map build and the incremental insert: their kernels as the compiler reports them for gfx950 -- each present in exactly
one unit, no scratch, no spills."""
import os
import re

from test_icp_build_cpu import ROOT, _assert_no_scratch

CSRC = os.path.join(ROOT, "gtsam_points_amd", "csrc")
# the kernels only the incremental insert launches: gp_voxelmap_incremental.hip
OWN_KERNELS = ("segmented_sums_kernel", "merge_source_kernel", "merge_finalize_kernel")
# the kernels it reaches through the helpers of gp_voxelmap.hpp (bounding box, block grid, bucket placement, line table): gp_voxelmap.hip
SHARED_KERNELS = ("voxels_bbox_kernel", "grid_mark_kernel", "grid_count_kernel", "insert_voxels_kernel", "line_claim_kernel")
# the rest of what came out of gp_voxelmap_kernels.hpp into gp_voxelmap.hip: the one-shot builds
BUILD_KERNELS = ("claim_buckets_kernel", "assign_voxels_kernel", "accumulate_kernel", "finalize_kernel", "grid_renumber_kernel", "buckets_renumber_kernel",
                 "segmented_stats_kernel")


def _kernels(unit):
    path = os.path.join(CSRC, unit + ".resources.txt")
    assert os.path.exists(path), "build the HIP library first (python -c 'import __graft_entry__ as g; g.build()')"
    return {b.split()[0]: b for b in open(path).read().split("remark: Function Name: ")[1:]}


def _get(block, key):
    return int(re.search(re.escape(key) + r":\s+(\d+)", block).group(1))


def _named(ks, name):
    """the kernels of the unit called gp::<name>, by the mangled name's length-prefixed component (finalize_kernel is not merge_finalize_kernel)"""
    return {k: v for k, v in ks.items() if f"{len(name)}{name}E" in k}


def _one(ks, name):
    found = _named(ks, name)
    assert len(found) == 1, name
    return found


def test_incremental_insert_kernels_use_no_scratch():
    own, shared = _kernels("gp_voxelmap_incremental"), _kernels("gp_voxelmap")
    for name in OWN_KERNELS:
        _assert_no_scratch(_one(own, name))
        assert not _named(shared, name), f"{name} is compiled into gp_voxelmap.hip too"
    for name in SHARED_KERNELS + BUILD_KERNELS:
        _assert_no_scratch(_one(shared, name))
        assert not _named(own, name), f"{name} is compiled into gp_voxelmap_incremental.hip too"
    _assert_no_scratch(own)  # nor does any other kernel the incremental unit holds
    # the frame's sums are the one-shot build's segmented sum without its finalize: no more registers than that kernel
    stats = list(_one(shared, "segmented_stats_kernel").values())[0]
    sums = list(_one(own, "segmented_sums_kernel").values())[0]
    assert _get(sums, "VGPRs") <= _get(stats, "VGPRs")
    for ks, names in ((own, ("segmented_sums_kernel", "merge_finalize_kernel")), (shared, ("segmented_stats_kernel", "lookup_kernel"))):
        for name in names:
            b = list(_one(ks, name).values())[0]
            print(f"[voxel map] {name}: {_get(b, 'VGPRs')} VGPRs, {_get(b, 'ScratchSize [bytes/lane]')} B scratch, {_get(b, 'Occupancy [waves/SIMD]')} waves/SIMD")

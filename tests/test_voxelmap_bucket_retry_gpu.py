"""The retry path of the bucket placement (csrc/gp_voxelmap.hip, place_voxels), shared by the binned one-shot build and the incremental insert: a table that cannot
hold every voxel within max_bucket_scan_count probes is doubled until it can.  216 voxels -- a 6 x 6 x 6 block of coordinates, one point each -- with
init_num_buckets = 64 and max_bucket_scan_count = 1: every voxel then has ONE bucket, and at the entry size (1024) two of them share it, by the hash itself."""
import numpy as np
import pytest

import voxelmap_ref as vr
from helpers import reference_bucket_lookup

pytestmark = pytest.mark.gpu

RES = 0.5
COORDS = [(x, y, z) for z in range(-2, 4) for y in range(-2, 4) for x in range(-2, 4)]
INIT_BUCKETS, MAX_SCAN = 64, 1


def _cloud(gpu):
    points = ((np.array(COORDS, dtype=np.float64) + 0.5) * RES).astype(np.float32)  # the voxel centres: exact in f32
    covs = np.tile((np.diag([1.0, 2.0, 3.0]) * 1e-2).reshape(1, 9), (len(COORDS), 1)).astype(np.float32)
    return gpu.PointCloudGPU(points, covs, intensities=np.arange(1, len(COORDS) + 1, dtype=np.float32))


def _per_voxel(vm, incremental):
    dl = vm.download()
    return list(vm.download_f64()) + [dl[k] for k in ("num_points", "means", "covs", "intensities")] + ([vm.download_stamps()] if incremental else [])


@pytest.mark.parametrize("incremental", [False, True], ids=["binned", "incremental"])
def test_too_small_table_is_doubled_until_every_voxel_is_placed(gpu, incremental):
    entry = vr.entry_bucket_count(INIT_BUCKETS, len(COORDS))
    assert not vr.buckets_can_place(COORDS, entry, MAX_SCAN)  # the condition of the test: the entry-size table cannot hold these voxels

    def build(**kw):
        vm = gpu.IncrementalGaussianVoxelMapGPU(RES, **kw) if incremental else gpu.GaussianVoxelMapGPU(RES, target_points_drop_rate=0.0, **kw)
        vm.insert(_cloud(gpu))
        return vm

    vm = build(init_num_buckets=INIT_BUCKETS, max_bucket_scan_count=MAX_SCAN)
    info = vm.voxelmap_info
    assert info.num_voxels == len(COORDS)
    assert info.num_buckets > entry  # a retry really happened
    assert vr.buckets_can_place(COORDS, info.num_buckets, MAX_SCAN) and not vr.buckets_can_place(COORDS, info.num_buckets // 2, MAX_SCAN)  # and stopped where it could
    b = vm.download()["buckets"]
    assert len(b) == info.num_buckets
    used = b[b[:, 3] >= 0]
    assert sorted(used[:, 3].tolist()) == list(range(info.num_voxels))
    coords = vm.download_f64()[0]
    assert sorted(map(tuple, coords.tolist())) == sorted(COORDS)
    for v, c in enumerate(coords.tolist()):
        assert reference_bucket_lookup(b, info, c) == v
    # the retries touch the bucket table alone: everything kept per voxel is the default build's, to the byte
    for i, (x, y) in enumerate(zip(_per_voxel(vm, incremental), _per_voxel(build(), incremental))):
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), f"per-voxel array {i} differs from the build with default bucket settings"

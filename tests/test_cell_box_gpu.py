"""The four bounding-box kernels (csrc/gp_cells.hpp, CellBox: bins_bbox_kernel, grid_insert_kernel + bbox_reduce_kernel, sampling_bbox_kernel, voxels_bbox_kernel)
and the key table's claim (csrc/gp_key_table.hpp) at the wave, workgroup and tile edges: clouds of 1, 63, 64, 65, 255, 256, 257, 4095, 4096 and 4097 points in
which point 0 ALONE sets the box's minimum, point n - 1 ALONE its maximum, and one point in between (n >= 3) is NaN -- a reduce that loses its first or last
lane, wave or tile, or lets a neutral / skipped lane into the box, loses a point, a voxel or a cell here.

Per size: a k = 1 search on the binned and on the hashed structure against tests/knn_ref.py (test_knn_edges_gpu.check_knn), voxelgrid_sampling against
tests/sampling_ref.py (assert_voxelgrid), a voxel-map build against tests/voxelmap_ref.py (test_voxelmap_edges_gpu._check) and OccupancyGridGPU.insert with its
cell and block counts against tests/ransac_ref.py's set (test_occupancy_edges_gpu.check_set): the comparison rules of those suites, no tolerance of this file's.
Covered there already and not repeated: the covariance launch shapes around 128 / 4096 points on structures 0 and 1 (test_knn_edges_gpu
test_covariances_around_the_launch_shapes), empty and all-invalid clouds (test_sampling_gpu, test_voxelmap_edges_gpu case_all_invalid), probe chains across the end
of the occupancy table (test_occupancy_edges_gpu)."""
import numpy as np
import pytest

import ransac_ref as rr
import sampling_ref as sr
import voxelmap_ref as vr
from test_knn_edges_gpu import HASHED, check_knn
from test_occupancy_edges_gpu import check_set, frame
from test_sampling_gpu import make_frame, rows
from test_voxelmap_edges_gpu import _build, _check

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097)
RES = 0.5


def cloud(n):
    """n points in [-4, 4)^3; point 0 at (-9.3, -8.3, -7.3) and point n - 1 at (9.3, 8.3, 7.3) set the box alone, point n // 2 is NaN (n >= 3)"""
    rng = np.random.default_rng(1000 + n)
    p = rng.uniform(-4.0, 4.0, (n, 3)).astype(np.float32)
    p[0] = (-9.3, -8.3, -7.3)
    if n > 1:
        p[n - 1] = (9.3, 8.3, 7.3)
    if n >= 3:
        p[n // 2] = (np.nan, 1.0, 1.0)
    return p


@pytest.fixture(scope="module")
def clouds():
    return {n: cloud(n) for n in SIZES}


@pytest.mark.parametrize("structure", [0, HASHED])
@pytest.mark.parametrize("n", SIZES)
def test_nearest_neighbour_sees_the_first_and_the_last_point(gpu, clouds, n, structure):
    p = clouds[n]
    tree = gpu.KdTreeGPU(gpu.PointCloudGPU(p), cell_size=RES, structure=structure)
    # the cloud's own points (each finds itself, the NaN point nothing) and one query beyond each corner, whose neighbours are the two extreme points
    q = np.concatenate([p, np.array([[-30.0, -30.0, -30.0], [30.0, 30.0, 30.0]], np.float32)])
    res = tree.knn_search(q, 1)
    check_knn(res, p, q, 1, what=f"n={n} structure {structure}")
    idx = res[0].reshape(-1)
    assert idx[len(p)] == 0 and idx[len(p) + 1] == n - 1


@pytest.mark.parametrize("n", SIZES)
def test_voxelgrid_sampling_keeps_the_corner_voxels(gpu, clouds, n):
    p = clouds[n]
    out = gpu.voxelgrid_sampling_gpu(make_frame(gpu, {"points": p}, names=("points",)), RES)
    ref = sr.voxelgrid_reference(p, {"points": p}, RES)
    assert out.size() == len(ref["keys"]) and out.num_dropped == (1 if n >= 3 else 0)
    got = rows(out, ("points",))
    sr.assert_voxelgrid(got, ref, what=f"n={n}", quiet=True)
    assert got["points"][:, 0].min() == p[0, 0] and got["points"][:, 0].max() == p[n - 1, 0]  # (each alone in its voxel: the mean is the point)


@pytest.mark.parametrize("n", SIZES)
def test_voxel_map_holds_the_corner_voxels(gpu, clouds, n):
    p = clouds[n]
    rng = np.random.default_rng(n)
    case = dict(points=p, covs=vr.general_covs(rng, n), intensities=rng.uniform(0.0, 1.0, n).astype(np.float32), res=RES)
    ref = vr.Map(case["points"], case["covs"], case["intensities"], case["res"])
    vm, c = _build(gpu, case, "binned")
    _check(gpu, vm, ref, f"n={n}", lookup_cloud=c)
    assert gpu.load().gp_voxelmap_has_block_grid(vm._h)  # the block grid is where voxels_bbox_kernel's box goes
    assert tuple(vr.voxel_coords(p[:1], RES)[0]) in ref.index and tuple(vr.voxel_coords(p[n - 1 :], RES)[0]) in ref.index


@pytest.mark.parametrize("n", SIZES)
def test_occupancy_insert_counts_cells_and_blocks(gpu, clouds, n):
    p = clouds[n]
    grid, ref = gpu.OccupancyGridGPU(RES).insert(frame(gpu, p)), rr.OccupancySet(RES).insert(p)
    check_set(gpu, grid, ref, [p, p[::-1].copy()])

"""OccupancyGridGPU at the edges of its table and of its coordinates, against the occupancy set of tests/ransac_ref.py.  Inputs: tests/registration_edges.py, held to
their conditions (empty band, planted home slots, aliasing keys) by tests/test_ransac_edges_ref_cpu.py.  Every comparison is exact, as in tests/test_occupancy_gpu.py.

  wrap-around     24 (48) blocks whose probe chains start in the last two slots of the 64 (128)-slot table and of the table twice as large: the chain runs over the
                  table's end in occ_find_or_claim, in occ_lookup and, after the growth, in the rehash.  Lookups of other cells of the same blocks and of other blocks
                  with the same home slots (the whole chain, then a free slot) must answer 0.
  growth          nine inserts of 20 .. 5120 one-point-per-block clouds into one grid: eight doublings, the set checked after each
  one block       4096 points (64 waves) claiming one block and setting all 512 of its cells at once
  aliasing        block coordinates beyond 21 bits (cells >= 2^24) and cells below -2^20, |floor| < 2^31 - 2^20.  Beyond the int range the float -> int conversion
                  decides; that contract is undefined and is not tested.
  scoring tiles   calc_overlap_batch at n = 1, 1023, 1024, 1025, 2049 (the kernel's tile is 1024 points) for 1, 2 and 65 poses"""
import numpy as np
import pytest

import ransac_ref as rr
import registration_edges as re_

pytestmark = pytest.mark.gpu


def frame(gpu, pts):
    return gpu.PointCloudGPU(np.ascontiguousarray(pts, np.float32))


def check_set(gpu, grid, ref, probes):
    assert grid.num_occupied_cells() == ref.num_occupied_cells()
    slots, blocks = grid.table_info()
    assert blocks == ref.num_blocks() and slots >= 2 * blocks and slots & (slots - 1) == 0
    for pts in probes:
        want = ref.get_overlaps(pts)
        got = grid.get_overlaps(frame(gpu, pts)).cpu().numpy()
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
        assert grid.calc_overlap(frame(gpu, pts)) == int(want.sum())
    return slots


@pytest.mark.parametrize("slots", [64, 128])
def test_probe_chains_wrap_over_the_end_of_the_table(gpu, slots):
    c = re_.wrap_case(slots)
    n = len(c["inserted"])
    grid = gpu.OccupancyGridGPU(re_.RES).insert(frame(gpu, c["inserted"]))
    assert grid.table_info()[0] == slots  # the premise: the planted keys were searched for this table
    ref = rr.OccupancySet(re_.RES).insert(c["inserted"])
    probes = [c["inserted"], c["same_blocks"], c["same_homes"], c["second"]]
    check_set(gpu, grid, ref, probes)
    assert ref.num_blocks() == n and ref.calc_overlap(c["inserted"]) == n and ref.calc_overlap(c["same_blocks"]) == 0 and ref.calc_overlap(c["same_homes"]) == 0
    grid.insert(frame(gpu, c["second"]))  # grows: the rehash walks the same wrapped chains in the larger table
    ref.insert(c["second"])
    assert check_set(gpu, grid, ref, probes) == 2 * slots
    assert ref.calc_overlap(c["second"]) == len(c["second"]) and ref.calc_overlap(c["same_homes"]) == 0
    grid.insert(frame(gpu, c["same_blocks"]))  # a second cell in every wrapped block, found through the chain by the insert
    ref.insert(c["same_blocks"])
    check_set(gpu, grid, ref, probes)
    assert ref.num_occupied_cells() == 3 * n + 8 and ref.num_blocks() == 2 * n + 8


def test_growth_through_eight_doublings(gpu):
    clouds, misses = re_.growth_clouds()
    grid, ref = gpu.OccupancyGridGPU(re_.RES), rr.OccupancySet(re_.RES)
    sizes = []
    for k, c in enumerate(clouds):
        grid.insert(frame(gpu, c))
        ref.insert(c)
        sizes.append(check_set(gpu, grid, ref, [np.concatenate(clouds[: k + 1]), clouds[min(k + 1, len(clouds) - 1)], misses]))
    assert sizes[0] == 64 and all(b >= 2 * a for a, b in zip(sizes, sizes[1:])) and sizes[-1] >= 2 * sum(re_.GROWTH_SIZES)


def test_one_block_claimed_by_4096_points(gpu):
    pts, neighbour = re_.full_block()
    grid = gpu.OccupancyGridGPU(re_.RES).insert(frame(gpu, pts))
    ref = rr.OccupancySet(re_.RES).insert(pts)
    check_set(gpu, grid, ref, [pts, neighbour])
    assert grid.num_occupied_cells() == 512 and grid.table_info()[1] == 1
    assert grid.calc_overlap(frame(gpu, pts)) == 4096 and grid.calc_overlap(frame(gpu, neighbour)) == 0


def test_aliasing_blocks_and_cells_far_below_the_origin(gpu):
    c = re_.alias_case()
    grid = gpu.OccupancyGridGPU(re_.FAR_RES).insert(frame(gpu, c["far"]))
    ref = rr.OccupancySet(re_.FAR_RES).insert(c["far"])
    probes = [c["far"], c["near"], c["unrelated"], np.concatenate([c["near"], c["unrelated"], c["far"]])]
    check_set(gpu, grid, ref, probes)
    assert ref.calc_overlap(c["near"]) == len(c["near"]) and ref.calc_overlap(c["unrelated"]) == 0  # the near cells alias with the far ones, as in the reference
    # the other way round: near-origin cells inserted, the far points fall into them; then both: the same set
    grid2 = gpu.OccupancyGridGPU(re_.FAR_RES).insert(frame(gpu, c["near"]))
    ref2 = rr.OccupancySet(re_.FAR_RES).insert(c["near"])
    check_set(gpu, grid2, ref2, probes)
    assert ref2.cells == ref.cells
    grid2.insert(frame(gpu, c["far"]))
    check_set(gpu, grid2, ref2, probes)


@pytest.mark.parametrize("n", re_.SCORE_SIZES)
def test_scoring_tile_edges(gpu, n):
    cloud = re_.score_cloud()
    grid = gpu.OccupancyGridGPU(re_.RES).insert(frame(gpu, cloud))
    ref = rr.OccupancySet(re_.RES).insert(cloud)
    pts = cloud[len(cloud) - n :]  # the last n points: the tail of the cloud is what a tile's edge would drop or read twice
    f = frame(gpu, pts)
    poses = [re_.score_pose(k) for k in range(re_.SCORE_POSES)]
    want = [ref.calc_overlap(pts, T) for T in poses]
    assert [grid.calc_overlap(f, T) for T in poses] == want
    for h in (1, 2, 65):
        got = grid.calc_overlap_batch(f, np.stack([poses[k % len(poses)] for k in range(h)])).cpu().numpy()
        assert got.dtype == np.int32 and got.tolist() == [want[k % len(poses)] for k in range(h)], (n, h)

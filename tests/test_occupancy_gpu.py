"""OccupancyGridGPU against the occupancy set of tests/ransac_ref.py (the restatement of FastOccupancyGrid; see its docstring).

Every comparison is exact: the device forms pose * p and the cell in the same f64 operations as the restatement (no fused multiply-add), and the pose reaches both as
the same 16 doubles.  The only points two roundings could place differently are those with a transformed coordinate / resolution within 1e-10 of an integer; the
inputs are asserted to have none."""
import functools

import numpy as np
import pytest

import ransac_ref as rr

pytestmark = pytest.mark.gpu

RES = 0.5


def pose(k):
    T = np.eye(4)
    T[:3, :3] = rr.rot([0.3 + k, -1.0, 0.5 * k + 0.2], 0.05 + 0.37 * k)
    T[:3, 3] = [0.31 * k - 1.0, 0.17 * k, -0.05 * k]
    return T


@functools.lru_cache(maxsize=None)
def clouds():
    rng = np.random.default_rng(17)
    c = {n: (rng.normal(size=(n, 3)) * 3).astype(np.float32) for n in (1, 63, 64, 65, 257)}
    c["wide"] = (rng.random((5000, 3)) * [120, 120, 20] - [60, 60, 10]).astype(np.float32)  # ~30 x 30 x 5 blocks of 4 m: more than 600 distinct blocks
    c["other"] = (rng.random((700, 3)) * 30 - [25, 5, 15]).astype(np.float32)
    c["negative"] = (-rng.random((300, 3)) * 50 - 0.001).astype(np.float32)
    c["one_cell"] = (np.array([3.1, -2.4, 0.6]) + rng.random((200, 3)) * 0.3).astype(np.float32)
    c["probe"] = np.concatenate([c["wide"][::7], c["other"][::3], c["negative"][::2], c["one_cell"][:20], c[257]]).astype(np.float32)
    return c


def frame(gpu, pts):
    return gpu.PointCloudGPU(np.ascontiguousarray(pts, np.float32))


def check(gpu, grid, ref, probe, poses):
    f = frame(gpu, probe)
    assert grid.num_occupied_cells() == ref.num_occupied_cells()
    assert grid.table_info()[1] == ref.num_blocks() and grid.table_info()[0] >= 2 * ref.num_blocks()
    singles = []
    for T in poses:
        assert rr.band_count(probe, T, ref.resolution) == 0
        want = ref.get_overlaps(probe, T)
        got = grid.get_overlaps(f, T).cpu().numpy()
        assert got.dtype == np.uint8 and np.array_equal(got, want)
        singles.append(grid.calc_overlap(f, T))
        assert singles[-1] == int(want.sum())
        assert grid.calc_overlap_rate(f, T) == singles[-1] / float(len(probe))
    for h in (1, 2, 65):
        batch = [poses[k % len(poses)] for k in range(h)]
        got = grid.calc_overlap_batch(f, np.stack(batch)).cpu().numpy()
        assert got.dtype == np.int32 and got.tolist() == [singles[k % len(poses)] for k in range(h)], h


@pytest.mark.parametrize("name", [1, 63, 64, 65, 257, "negative", "one_cell"])
def test_small_clouds(gpu, name):
    c = clouds()
    pts = c[name]
    grid = gpu.OccupancyGridGPU(RES).insert(frame(gpu, pts))
    ref = rr.OccupancySet(RES).insert(pts)
    if name == "one_cell":
        assert ref.num_occupied_cells() == 1
    probe = np.concatenate([pts, c["probe"][:200]])
    check(gpu, grid, ref, probe, [np.eye(4), pose(0), pose(1)])
    assert grid.calc_overlap(frame(gpu, pts)) == len(pts)


def test_many_blocks_inserted_twice_and_a_union(gpu):
    c = clouds()
    ref = rr.OccupancySet(RES).insert(c["wide"])
    assert ref.num_blocks() > 600
    grid = gpu.OccupancyGridGPU(RES).insert(frame(gpu, c["wide"]))
    poses = [np.eye(4), pose(0), pose(2), pose(3)]
    check(gpu, grid, ref, c["probe"], poses)
    grid.insert(frame(gpu, c["wide"]))  # the same cloud again: the same set
    check(gpu, grid, ref, c["probe"], poses)
    # a second cloud, inserted at a pose: the union (the table grows from the first cloud's size)
    grid.insert(frame(gpu, c["other"]), pose(1))
    ref.insert(c["other"], pose(1))
    assert rr.band_count(c["other"], pose(1), RES) == 0
    check(gpu, grid, ref, c["probe"], poses)
    # small first, large second: the rehash carries the first cloud's cells over
    grid2 = gpu.OccupancyGridGPU(RES).insert(frame(gpu, c[65])).insert(frame(gpu, c["wide"]))
    ref2 = rr.OccupancySet(RES).insert(c[65]).insert(c["wide"])
    check(gpu, grid2, ref2, c["probe"], poses[:2])


def test_points_without_a_cell(gpu):
    pts = np.array([[0.1, 0.2, 0.3], [np.nan, 0, 0], [np.inf, 1, 1], [4.0, 4.0, 4.0]], np.float32)
    grid = gpu.OccupancyGridGPU(1.0).insert(frame(gpu, pts))
    assert grid.num_occupied_cells() == 2
    assert grid.get_overlaps(frame(gpu, pts)).cpu().numpy().tolist() == [1, 0, 0, 1] and grid.calc_overlap(frame(gpu, pts)) == 2
    with pytest.raises(gpu.GPError):
        gpu.OccupancyGridGPU(-1.0)

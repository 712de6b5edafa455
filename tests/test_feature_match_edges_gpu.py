"""match_features_gpu / gp_feature_nn_search at their edges, against the brute-force search of tests/ransac_ref.py.  Inputs: tests/registration_edges.py, held to their
conditions (the planted ties are the only ties, no tie at all in the shape cases) by tests/test_ransac_edges_ref_cpu.py.

The tie contract: among targets at exactly the same f64 distance the LOWEST index is returned -- what the kernel does (each lane keeps its first by strict <, the
shuffle reduction prefers the lower index at equal distances), what rr.match_features restates (np.argmin), and what "the same seed gives the same arrays" in RANSAC
rests on.  Identical rows give identical sums on the device (the same operations in the same order on the same values), so a planted copy IS an exact tie there.

Bounds (tests/test_feature_match_gpu.py): index exact; |d_gpu - d_ref| <= (D + 4) 2^-52 d_ref.  A distance of exactly 0 (a query copied from a target row) has the
bound 0: every term is (x - x)^2 = 0 on both sides.  Entries of 1e18 and 1e-30 keep every f64 term between 1e-60 and 1e37: the same bound."""
import ctypes as C

import numpy as np
import pytest

import ransac_ref as rr
import registration_edges as re_

pytestmark = pytest.mark.gpu


def device_match(gpu, tf, sf, rows=None):
    gi, gd = gpu.match_features_gpu(tf, sf, rows)
    return gi.cpu().numpy(), gd.cpu().numpy()


def within_bound(what, d, gd, sq):
    finite = np.isfinite(sq)
    assert np.array_equal(np.isposinf(gd), ~finite) and not np.isnan(gd).any()
    err, bound = np.abs(gd[finite] - sq[finite]), (d + 4) * 2.0 ** -52 * sq[finite]
    if finite.any():
        print(f"{what}: worst |d_gpu - d_ref| = {float((err / np.maximum(bound, 1e-300)).max()):.3f} of the bound (D + 4) 2^-52 d")
    assert (err <= bound).all()


@pytest.mark.parametrize("a", re_.TIE_PLACES)
@pytest.mark.parametrize("pattern", [p for p, _ in re_.TIE_PATTERNS])
@pytest.mark.parametrize("d", re_.TIE_DIMS)
def test_planted_ties_go_to_the_lowest_index(gpu, d, pattern, a):
    tf, sf, group = re_.tie_case(d, pattern, a)
    idx, sq, ties = rr.match_features(tf, sf)
    gi, gd = device_match(gpu, tf, sf)
    assert (gi[[0, 5, 16]] == a).all() and a == min(group), (gi[[0, 5, 16]], group)
    assert np.array_equal(gi, idx)
    within_bound(f"D {d} {pattern} a {a}", d, gd, sq)


@pytest.mark.parametrize("d", re_.TIE_DIMS)
def test_every_target_row_identical_gives_index_0(gpu, d):
    same = np.tile(np.float32(0.25), (130, d))
    gi, gd = device_match(gpu, same, np.zeros((17, d), np.float32))
    assert (gi == 0).all() and (gd == d * 0.0625).all()  # (exact: D x 2^-4)


@pytest.mark.parametrize("with_rows", [False, True])
@pytest.mark.parametrize("nq", re_.SHAPE_NQ)
@pytest.mark.parametrize("nt", re_.SHAPE_NT)
@pytest.mark.parametrize("d", re_.SHAPE_DIMS)
def test_shapes_around_the_tile_and_the_workgroup(gpu, d, nt, nq, with_rows):
    tf, sf, rows, idx, sq, ties = re_.shape_case(d, nt, nq, with_rows)
    gi, gd = device_match(gpu, tf, sf, rows)
    assert gi.shape == (nq,) and gd.shape == (nq,) and np.array_equal(gi, idx)
    within_bound(f"D {d} nt {nt} nq {nq}", d, gd, sq)


@pytest.mark.parametrize("kind", ["zero", "huge", "nan_target", "all_nan", "nan_query"])
def test_values(gpu, kind):
    tf, sf = re_.value_case(kind)
    idx, sq, ties = rr.match_features(tf, sf)
    gi, gd = device_match(gpu, tf, sf)
    assert np.array_equal(gi, idx), (gi, idx)
    within_bound(kind, 8, gd, sq)
    if kind == "zero":
        assert gd[3] == 0.0 and gd[16] == 0.0 and gi[3] == 77 and gi[16] == 5
    if kind == "huge":
        assert gd[1] == float(np.float32(1e-30)) ** 2 and gi[1] == 4  # one exact product, not flushed to 0
    if kind == "nan_target":
        assert not np.isin(gi, (9, 70)).any()
    if kind == "all_nan":
        assert (gi == -1).all() and np.isposinf(gd).all()
    if kind == "nan_query":
        assert gi[5] == -1 and gi[16] == -1 and np.isposinf(gd[[5, 16]]).all() and (gi[np.r_[0:5, 6:16]] >= 0).all()


def test_rows_outside_the_source_through_the_c_abi(gpu):
    """the Python wrapper refuses these; the C entry point documents (-1, +inf) for them, and RANSAC relies on it (a dead iteration's rows are -1)"""
    import torch

    tf, sf = re_.value_case("zero")
    ns = len(sf)
    rows = np.array([0, -1, 3, ns, 16, ns + 1000, -(2 ** 31), 2 ** 31 - 1, 5, -1, 1, 2, 4, 6, 7, 8, 9], np.int32)  # 17 queries: both workgroups hold some
    inside = (rows >= 0) & (rows < ns)
    idx, sq, _ = rr.match_features(tf, sf, rows)
    assert (idx[~inside] == -1).all() and (idx[inside] >= 0).all()
    t, s, r = torch.from_numpy(tf).cuda(), torch.from_numpy(sf).cuda(), torch.from_numpy(rows).cuda()
    gi = torch.full((len(rows),), -7, dtype=torch.int32, device="cuda")
    gd = torch.full((len(rows),), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    lib = gpu._capi.load()
    ptr = lambda x: C.c_void_p(x.data_ptr())
    gpu._capi.check(lib.gp_feature_nn_search(ptr(t), len(tf), ptr(s), ns, 8, ptr(r), len(rows), ptr(gi), ptr(gd), None), "gp_feature_nn_search")
    gpu._capi.check(lib.gp_stream_synchronize(None), "gp_stream_synchronize")
    gi, gd = gi.cpu().numpy(), gd.cpu().numpy()
    assert np.array_equal(gi, idx) and np.isposinf(gd[~inside]).all()
    within_bound("rows", 8, gd, sq)
    assert gd[2] == 0.0 and gd[4] == 0.0

"""tests/stream_plan_ref.py against the library's own plan (gp_debug_stream_plan_ex: make_stream_plan + plan_tile + split_tile on the host, no device), and what the
case table of tests/test_stream_edges_gpu.py covers: the GPU file runs exactly these geometries, so a stream length or plan shape missing here is one no test runs."""
import ctypes as C

import numpy as np
import pytest

import stream_plan_ref as spr


def _library_waves(n, cap, skew, weights, tile_points=0):
    from gtsam_points_amd import _capi

    lib = _capi.load()
    w = (C.c_int * 8)(*weights) if weights is not None else None
    G = C.c_int()
    assert lib.gp_debug_stream_plan_ex(n, tile_points, cap, skew, w, 0, None, None, None, C.byref(G)) == 0, lib.gp_last_error()
    b, c, wv = np.zeros(G.value, np.int32), np.zeros(G.value, np.int32), np.zeros((G.value * 4, 3), np.int64)
    assert lib.gp_debug_stream_plan_ex(n, tile_points, cap, skew, w, G.value, b.ctypes.data, c.ctypes.data, wv.ctypes.data, C.byref(G)) == 0, lib.gp_last_error()
    return np.stack([b, c], 1).astype(np.int64), wv


def _assert_partition(wv, n, what):
    """the waves' streams, in order, are [0, n) without a gap or an overlap; only a wave that ends the cloud has a tail"""
    at = 0
    for first, chunks, tail in wv.tolist():
        if chunks or tail:
            assert first == at and first % 64 == 0, (what, first, at)
            at += 64 * chunks + tail
        assert chunks >= 0 and 0 <= tail < 64 and (tail == 0 or at == n), (what, first, chunks, tail)
    assert at == n, (what, at)


# beyond the table: sizes around every boundary of the plan (the threshold, one chunk per wave, gx = 32 | 33, 64 | 65, 96 | 97, 128), large clouds, odd caps
EXTRA = [(n, cap, skew, w) for n in (65_536, 66_000, 69_632, 131_008, 131_136, 196_544, 196_672, 262_144, 262_145, 400_000, 1_000_077, 8_000_000)
         for cap, skew, w in ((1024, -1, None), (1000, 250, None), (520, 1000, spr._w(x0=1500, x1=500)), (40, 0, (1000,) * 8), (8, 600, None))]


@pytest.mark.parametrize("table", ["cases", "extra"])
def test_restatement_equals_the_library_plan(table):
    for n, cap, skew, weights in spr.CASES if table == "cases" else EXTRA:
        p, tiles = spr.planned_tiles(n, cap, skew, weights)
        lt, lw = _library_waves(n, cap, skew, weights)
        what = (n, cap, skew, weights)
        assert len(lt) == p["workgroups"] and len(lt) % 8 == 0 and 8 <= len(lt) <= 1024, what
        assert np.array_equal(tiles, lt), what
        assert np.array_equal(spr.waves(tiles), lw), what
        _assert_partition(lw, n, what)


def test_old_entry_point_is_the_new_one_at_the_default_cap():
    from gtsam_points_amd import _capi

    lib = _capi.load()
    for n, skew in [(65_599, -1), (1_000_077, 200), (198_719, 400)]:
        G = C.c_int()
        assert lib.gp_debug_stream_plan(n, skew, None, 0, None, None, C.byref(G)) == 0
        b, c = np.zeros(G.value, np.int32), np.zeros(G.value, np.int32)
        assert lib.gp_debug_stream_plan(n, skew, None, G.value, b.ctypes.data, c.ctypes.data, C.byref(G)) == 0
        lt, _ = _library_waves(n, 1024, skew, None)
        assert np.array_equal(np.stack([b, c], 1), lt)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 255, 256, 257, 4_096, 4_097, 5_000, spr.N_CONTROL])
@pytest.mark.parametrize("tile_chunks", spr.TILE_CHUNKS)
def test_fixed_tiles(n, tile_chunks):
    tiles = spr.fixed_tiles(n, 256 * tile_chunks)
    lt, lw = _library_waves(n, 1024, -1, None, 256 * tile_chunks)
    assert np.array_equal(tiles, lt) and np.array_equal(spr.waves(tiles), lw)
    _assert_partition(lw, n, (n, tile_chunks))
    assert lw[:, 1].max(initial=0) <= tile_chunks


def test_bad_arguments_are_refused():
    from gtsam_points_amd import _capi

    lib = _capi.load()
    G = C.c_int()
    for n, tp, cap in [(-1, 0, 1024), (100, 0, 7), (100, 0, 1025), (100, 100, 1024), (100, -256, 1024)]:
        assert lib.gp_debug_stream_plan_ex(n, tp, cap, -1, None, 0, None, None, None, C.byref(G)) != 0
    b = np.zeros(4, np.int32)
    assert lib.gp_debug_stream_plan_ex(100_000, 0, 1024, -1, None, 4, b.ctypes.data, b.ctypes.data, None, C.byref(G)) != 0 and G.value > 4  # capacity


def test_the_case_table_covers_the_kernels_paths():
    """what tests/test_stream_edges_gpu.py runs, read off the restatement (held to the library above): every stream length at which vgicp_stream_kernel's loop takes
    another way -- no chunk, 1 (the prologue alone), 2 (has1 without more2), 3, both parities beyond, the lengths of an 8 M-point source (>= 32) and twice that --
    beside each other in planned launches, and every shape of plan"""
    lengths, tails, facts, skewed_default, distinct = set(), set(), set(), set(), set()
    for n, cap, skew, weights in spr.CASES:
        assert n >= spr.PLAN_MIN_POINTS
        p, wv = spr.launch_waves(n, cap, skew, weights)
        _assert_partition(wv, n, (n, cap, skew, weights))
        per_launch = set(wv[:, 1].tolist())
        distinct.add((n, wv.tobytes()))
        lengths |= per_launch
        tails.add(n % 64)
        per_wg = wv[:, 1].reshape(-1, 4).sum(1)
        if ((wv[:, 1] == 0) & (wv[:, 2] > 0)).any():
            facts.add("tail-only wave")
        rounds = -(-p["gx"] // 32)
        if p["skewed"]:
            assert p["last_begin"] == 32 * (rounds - 1) > 0
            facts.add(f"skewed, {rounds} rounds")
            facts.add("skewed, partial last round" if p["gx"] % 32 else "skewed, full last round")
            if skew == 1000:
                facts.add("skewed at 1000")
            if cap == 1024:
                facts.add(f"skewed at the default cap, {rounds} rounds")
                skewed_default.add((n, skew))
            if p["gx"] == 33:
                assert p["last_begin"] == 32 and all(len(c) == 33 for c in p["chunks"])
                facts.add("skewed at gx = 33")
        elif skew != 0 and rounds > 1:
            facts.add("skew refused")
            if p["gx"] == 33:
                facts.add("skew refused at gx = 33")
            if rounds == 4:
                facts.add("skew refused, four rounds")
        if (per_wg < 4).any():
            facts.add("workgroup with fewer than 4 chunks")
        if ((per_wg >= 1) & (per_wg <= 2)).any() and weights is not None:
            facts.add("extreme weights leave 1-2 chunks")
        if {0, 2}.issubset(per_launch) and max(per_launch) >= 3:
            facts.add("0 and 2 beside more")
        if 3 in per_launch and max(per_launch) > 3:
            facts.add("3 beside more")
    for want in (0, 1, 2, 3):
        assert want in lengths, want
    assert any(v >= 5 and v % 2 == 1 for v in lengths) and any(v >= 5 and v % 2 == 0 for v in lengths)
    assert any(v >= 32 for v in lengths) and any(v >= 64 for v in lengths)
    assert {0, 1, 63}.issubset(tails)
    assert facts == {"tail-only wave", "skewed, 2 rounds", "skewed, 3 rounds", "skewed, partial last round", "skewed, full last round", "skewed at 1000", "skewed at gx = 33",
                     "skewed at the default cap, 2 rounds", "skewed at the default cap, 3 rounds", "skew refused", "skew refused at gx = 33", "skew refused, four rounds",
                     "workgroup with fewer than 4 chunks", "extreme weights leave 1-2 chunks", "0 and 2 beside more", "3 beside more"}, facts
    # the balance sweep at the default cap is not empty: one size takes three of the issue's values, and what stream_plan_ref.py says about the others holds
    assert skewed_default == {(spr.N_SKEW_DEF, 50), (spr.N_SKEW_DEF, 150), (spr.N_SKEW_DEF, 400), (spr.N_MID[2], 50), (spr.N_MID[2], 150)}, skewed_default
    # repeated plans (a refused skew is the flat plan; 256 workgroups are all 65,536 points need) are run but not counted
    assert len(spr.CASES) == 52 and len(distinct) == 39, (len(spr.CASES), len(distinct))
    # the control runs on fixed tiles, and so does the batch of small factors at every tile size
    assert spr.N_CONTROL < spr.PLAN_MIN_POINTS
    for tc in spr.TILE_CHUNKS:
        for n in spr.FIXED_BATCH:
            _assert_partition(spr.launch_waves(n, tile_points=256 * tc)[1], n, (n, tc))

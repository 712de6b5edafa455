"""The inputs of the edge tests of global registration (tests/test_occupancy_edges_gpu.py, tests/test_feature_match_edges_gpu.py, tests/test_ransac_edges_gpu.py), built
on the restatement alone.  tests/test_ransac_edges_ref_cpu.py holds every one of them to the conditions the exact device comparisons rest on; the GPU tests only use them.

Occupancy points are cell centres: (cell + 0.5) * resolution with resolution 0.5, exactly representable in f32 and half a cell from every face, so the band of
rr.band_count is empty by construction (and asserted).  The far points are integer-valued in f32 (spacing 2 at 1.7e7, 64 at 1e9): at a power-of-two resolution they would
sit exactly on faces, so their resolution is sqrt(1.03) (1.01 would
not do: every multiple of 101 is on a face), at which x * (1 / resolution) is nowhere within 1e-10 of an integer (asserted)."""
import functools

import numpy as np

import ransac_ref as rr

RES = 0.5
FAR_RES = 1.03 ** 0.5  # 1.0148891565092219
ORIGIN_BLOCK = rr.OFFSET >> 3  # the block coordinate of cell 0


def cell_centre(cells, resolution=RES):
    """f32 points at the centres of the cells (integer cell coordinates counted from the origin, any sign)"""
    return ((np.asarray(cells, np.float64) + 0.5) * resolution).astype(np.float32)


def blocks_at_home(slots, homes, count, skip=0, span=24):
    """the first `count` (after `skip`) blocks of a span^3 cube of block coordinates around the origin whose key's home slot in a table of `slots` is in `homes`: (block
    coordinates relative to the origin's block [count][3], keys)"""
    found, keys = [], []
    for bz in range(-span // 2, span // 2):
        for by in range(-span // 2, span // 2):
            for bx in range(-span // 2, span // 2):
                k = rr.block_key(bx + ORIGIN_BLOCK, by + ORIGIN_BLOCK, bz + ORIGIN_BLOCK)
                if rr.home_slot(k, slots) in homes:
                    found.append((bx, by, bz))
                    keys.append(k)
    assert len(found) >= skip + count
    return np.array(found[skip : skip + count], np.int64), keys[skip : skip + count]


@functools.lru_cache(maxsize=None)
def wrap_case(slots):
    """keys whose probe chains start in the last two slots of a `slots`-slot table and of the table twice as large: `inserted` (one point per block, cell (1, 2, 3) of
    it), `same_blocks` (cell (6, 5, 4) of the same blocks: not in the set), `same_homes` (points in other blocks with the same home slots: not in the set, found only
    behind the whole chain), `second` (a cloud in generic blocks that forces the table to grow)"""
    n = 24 * slots // 64
    homes2 = (2 * slots - 2, 2 * slots - 1)  # home 2 s - 2 or 2 s - 1 of 2 s slots is home s - 2 or s - 1 of s slots
    blocks, keys = blocks_at_home(2 * slots, homes2, n)
    other, other_keys = blocks_at_home(2 * slots, homes2, 8, skip=n)
    rng = np.random.default_rng(slots)
    second_blocks = rng.permutation(40 ** 3)[: n + 8]
    second_blocks = np.stack([second_blocks % 40, second_blocks // 40 % 40, second_blocks // 1600], axis=1) + 100  # away from the cube searched above
    return {"slots": slots, "keys": keys, "other_keys": other_keys, "inserted": cell_centre(blocks * 8 + [1, 2, 3]), "same_blocks": cell_centre(blocks * 8 + [6, 5, 4]),
            "same_homes": cell_centre(other * 8 + [1, 2, 3]), "second": cell_centre(second_blocks * 8 + [7, 0, 5]),
            "second_keys": [rr.block_key(*(np.array(b) + ORIGIN_BLOCK)) for b in second_blocks.tolist()]}


GROWTH_SIZES = (20, 40, 80, 160, 320, 640, 1280, 2560, 5120)


@functools.lru_cache(maxsize=None)
def growth_clouds():
    """one point per block, every block distinct over all clouds (10220 of the 32^3 blocks of a cube), cells varied"""
    rng = np.random.default_rng(23)
    b = rng.permutation(32 ** 3)[: sum(GROWTH_SIZES)]
    blocks = np.stack([b % 32, b // 32 % 32, b // 1024], axis=1) - 16
    pts = cell_centre(blocks * 8 + rng.integers(0, 8, size=blocks.shape))
    out, at = [], 0
    for n in GROWTH_SIZES:
        out.append(pts[at : at + n])
        at += n
    misses = cell_centre((np.stack([b % 32, b // 32 % 32, b // 1024], axis=1)[:500] + 40) * 8)  # blocks no cloud touches
    return out, misses


@functools.lru_cache(maxsize=None)
def full_block():
    """4096 points over all 512 cells of the block (-3, 2, 5), eight per cell at different places inside it, shuffled; and the same cells of the neighbouring block"""
    rng = np.random.default_rng(29)
    cells = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), axis=-1).reshape(-1, 3) + np.array([-3, 2, 5]) * 8
    cells = np.repeat(cells, 8, axis=0)
    pts = ((cells + rng.integers(1, 8, size=cells.shape) / 8.0) * RES).astype(np.float32)  # eighths of a cell: exact in f32, at least 1/8 cell from a face
    return pts[rng.permutation(len(pts))], cell_centre(cells[::8] + [8, 0, 0])


@functools.lru_cache(maxsize=None)
def alias_case():
    """far: f32 points whose coordinates lie k x 2^24 cells from the origin, k in (1, -1, 59, -59) (about +-1.7e7 and +-1e9 at the resolution 1.0149), so that their blocks
    alias by the 21-bit mask with blocks near the origin and the negative ones lie below cell -2^20; near: for every far point the centre of the near-origin cell with
    the same (key, bit); unrelated: near-origin cells that alias with none of them.  |floor| stays below 2^31 - 2^20: beyond the int range the contract is undefined."""
    rng = np.random.default_rng(31)
    ks = np.array([1, -1, 59, -59])
    k = ks[rng.integers(0, 4, size=(96, 3))]
    k[:4] = ks[:, None]  # every k on all three axes at once
    far = (k * float(1 << 24) * FAR_RES + rng.uniform(-3000, 3000, size=k.shape)).astype(np.float32)
    cells = np.floor(far.astype(np.float64) * (1.0 / FAR_RES)).astype(np.int64)
    assert (np.abs(cells) < 2 ** 31 - 2 ** 20).all()
    near = cell_centre(cells - k * (1 << 24), FAR_RES)
    unrelated = cell_centre(cells - k * (1 << 24) + [16, -24, 8], FAR_RES)
    return {"far": far, "near": near, "unrelated": unrelated, "k": k}


SCORE_SIZES = (1, 1023, 1024, 1025, 2049)


def score_pose(k):
    T = np.eye(4)
    T[:3, :3] = rr.rot([0.3 + k, -1.0, 0.5 * k + 0.2], 0.05 + 0.37 * k)
    T[:3, 3] = [0.31 * k - 1.0, 0.17 * k + 0.013, -0.05 * k + 0.007]
    return T


SCORE_POSES = 5


@functools.lru_cache(maxsize=None)
def score_cloud():
    rng = np.random.default_rng(37)
    return (rng.random((2049, 3)) * [40, 40, 10] - [20, 20, 5]).astype(np.float32)


# ---- feature matching -----------------------------------------------------------------------------------------------------------------------------------------------
TIE_DIMS = (1, 64, 128)
TIE_NT, TIE_NQ = 257, 17
# (name, offsets of the twins from a): inside one tile of 64 rows, the same lane one tile on, another lane two tiles on, three ways over a tile's edge
TIE_PATTERNS = (("next", (1,)), ("lane", (64,)), ("far", (130,)), ("three", (63, 64)))


TIE_PLACES = (0, 40, 63)  # a: with a = 63 the twin a + 1 (a + 130) lies in a LOWER lane of a later tile, with a = 0 and 40 in a higher one or the same


@functools.lru_cache(maxsize=None)
def tie_case(d, pattern, a):
    """random rows with one row copied to the places a, a + off ...; queries 0, 5 and 16 (the first and a middle query of a wave, and the second workgroup) sit next to
    that row, far nearer than to any other.  A rule that keeps the first or the last candidate met, or the lower LANE, differs from "the lowest index" at one of
    TIE_PLACES.  Returns (tf, sf, group)"""
    offs = dict(TIE_PATTERNS)[pattern]
    rng = np.random.default_rng(100 * d + len(pattern) + 7 * a)
    tf = rng.normal(size=(TIE_NT, d)).astype(np.float32)
    if d == 1:  # random scalars crowd: a grid of 0.05 in random order keeps every other row 0.05 away from the planted one
        tf = (rng.permutation(TIE_NT)[:, None] * 0.05 - 6.0).astype(np.float32)
    sf = rng.normal(size=(TIE_NQ, d)).astype(np.float32)
    group = [a] + [a + o for o in offs]
    for g in group:
        tf[g] = tf[a]
    for q, eps in ((0, 0.001), (5, -0.002), (16, 0.003)):
        sf[q] = tf[a] + np.float32(eps)
    return tf, sf, group


SHAPE_DIMS = (2, 63, 64, 65, 127)
SHAPE_NT = (63, 64, 65, 129)
SHAPE_NQ = (15, 16, 17)


@functools.lru_cache(maxsize=None)
def shape_case(d, nt, nq, with_rows):
    rng = np.random.default_rng(5000 * d + 10 * nt + nq + int(with_rows))
    tf = rng.normal(size=(nt, d)).astype(np.float32)
    ns = nq if not with_rows else 2 * nq + 3
    sf = rng.normal(size=(ns, d)).astype(np.float32)
    rows = rng.integers(0, ns, size=nq).astype(np.int32) if with_rows else None
    return (tf, sf, rows) + rr.match_features(tf, sf, rows)


@functools.lru_cache(maxsize=None)
def value_case(kind):
    """D = 8, 130 targets, 17 queries (two workgroups of 16).  kind: zero (queries 3 and 16 are copies of targets 77 and 5), huge (entries of 1e18 and 1e-30 mixed in: distances of 1e36 and of 1e-60),
    nan_target (target 9 NaN, target 70 +inf, and query 2 sits next to where target 9 was), all_nan (every target NaN), nan_query (queries 5 and 16 NaN)"""
    rng = np.random.default_rng(41)
    tf = rng.normal(size=(130, 8)).astype(np.float32)
    sf = rng.normal(size=(17, 8)).astype(np.float32)
    if kind == "zero":
        sf[3], sf[16] = tf[77], tf[5]
    elif kind == "huge":
        tf[::3, 2] = (1e18 * (1.0 + np.arange(44) / 64.0)).astype(np.float32)  # told apart far above the rounding of their squares
        tf[1::3, 5] = np.float32(1e-30)
        sf[::2, 2] = np.float32(3e18)  # nearest: the largest of the 1e18 rows, at a distance of about 1.8e36
        sf[1::2, 7] = np.float32(1e-30)
        sf[1] = tf[4]
        sf[1, 5] = 0.0  # target 4 differs from query 1 by 1e-30 in one entry: the distance is 1e-60, not 0
    elif kind == "nan_target":
        sf[2] = tf[9] + np.float32(0.001)
        sf[4] = tf[70] + np.float32(0.001)
        tf[9, 3] = np.nan
        tf[70, 6] = np.inf
    elif kind == "all_nan":
        tf[np.arange(130), rng.integers(0, 8, size=130)] = np.nan  # one NaN entry per row
    elif kind == "nan_query":
        sf[5, 0] = np.nan
        sf[16] = np.nan
    return tf, sf


# ---- RANSAC -----------------------------------------------------------------------------------------------------------------------------------------------------------
EDGE_ITERATIONS = 50
CHUNKS = (1, 7, 50, 64)
NEVER_STOP = 1.0  # inliers > N_s x 1.0 cannot happen


def small_ref(dof, far=0.0, iterations=EDGE_ITERATIONS, **kw):
    c = rr.make_small_case(dof, far)
    return rr.estimate_pose_ransac(c["target"], c["source"], c["target_features"], c["source_features"], iterations, dof=dof, **kw)


@functools.lru_cache(maxsize=None)
def boundary_samples(dof):
    """explicit samples, 20 iterations: the generator's own draws of seed 7 with one index replaced by the float32(1e-3) row (0 .. 3: still valid), the 2^-10 row (4 .. 7:
    invalid), the NaN row (8 .. 11: valid, no match, target 0) and an all-zero row (12 .. 15: invalid), the special row at every position of the sample"""
    samples = 3 if dof == 6 else 2
    given = np.full((20, 3), -1, np.int32)
    for it in range(16):
        idx = rr.draw_samples(7, it, 256, samples)
        special = (rr.SMALL_ROW_1E3, rr.SMALL_ROW_2M10, rr.SMALL_ROW_NAN, rr.SMALL_ZERO_ROWS[0])[it // 4]
        assert special not in idx
        idx[it % samples] = special
        given[it, :samples] = idx
    base = small_ref(dof, chunk_iterations=EDGE_ITERATIONS, early_stop_inlier_rate=NEVER_STOP)
    scored = np.flatnonzero(base[2] == rr.SCORED)[:4]
    given[16:] = base[4]["source_indices"][scored]  # 16 .. 19: four samples of the generator's that are scored, as they are
    return given


def decoy_poses(n):
    """poses far from anything RANSAC can produce from the small case: translations of hundreds of metres"""
    out = []
    for k in range(n):
        T = np.eye(4)
        T[:3, :3] = rr.rot([1.0, 0.3 * k, -0.5], 0.1 * k)
        T[:3, 3] = [500.0 + 7 * k, -300.0, 40.0 * k]
        out.append(T)
    return out


@functools.lru_cache(maxsize=None)
def degenerate_cloud():
    """a hand-made cloud whose samples reach the alignment's degenerate branches.  Source: points 0, 1, 2 identical (A), 3 = A + (3, 0, 0) (the difference along x alone:
    H has one non-zero column exactly), 4 and 7 generic, 5 = A + (0, 0, 2) (differs from A in z only), 6 generic.  Target i = T source i (T a rotation about z and a
    translation, so that 5's image differs from A's in z only), then 30 random points; feature row i of the source sits next to row i of the target."""
    rng = np.random.default_rng(43)
    A = np.array([1.25, -2.5, 0.75])
    source = np.array([A, A, A, A + [3, 0, 0], [4.5, 1.0, -1.25], A + [0, 0, 2], [-2.0, 3.5, 2.25], [0.5, 0.25, 3.0]], np.float32)
    T = np.eye(4)
    T[:3, :3] = rr.rot([0, 0, 1], 0.7)
    T[:3, 3] = [2.3, 1.1, -3.2]
    target = np.concatenate([(source.astype(np.float64) @ T[:3, :3].T + T[:3, 3]), rng.normal(size=(30, 3)) * 20 + 100]).astype(np.float32)
    tf = rng.normal(size=(len(target), 8)).astype(np.float32)
    sf = tf[: len(source)] + np.float32(0.001)
    return {"source": source, "target": target, "target_features": tf, "source_features": sf, "T": T}


# (dof, sample, what): the explicit samples of the degenerate test
DEGENERATE_SAMPLES = ((6, (0, 1, 4), "two identical points and a third: H of rank 1"), (6, (0, 1, 3), "the same with the third along x: two columns of H exactly zero"),
                      (6, (0, 1, 2), "three identical points: H = 0"), (6, (4, 4, 6), "[i, i, j]"), (6, (3, 3, 3), "[i, i, i]: H = 0"),
                      (4, (0, 5, -1), "two points that differ in z only: the 2x2 block of H vanishes"), (4, (0, 1, -1), "two identical points: H = 0"))


ALIGN_SIZES = (255, 256, 257, 513)


@functools.lru_cache(maxsize=None)
def align_case(dof, n):
    """a noisy weighted N-point problem as in test_weighted_alignment_alone, a third of the weights zero and the points under them far off (they must not count)"""
    rng = np.random.default_rng(1000 * dof + n)
    T = np.eye(4)
    T[:3, :3] = rr.rot([0.3, 0.5, -1.0], 0.8) if dof == 6 else rr.rot([0, 0, 1], -2.1)
    T[:3, 3] = [1.0, -4.0, 0.3]
    s = rng.normal(size=(n, 3)) * 5
    t = s @ T[:3, :3].T + T[:3, 3] + rng.normal(size=(n, 3)) * 0.05
    w = rng.random(n) + 0.1
    zero = np.arange(n) % 3 == 1
    w[zero] = 0.0
    t[zero] += rng.normal(size=(int(zero.sum()), 3)) * 50
    return t, s, w

"""numpy restatement of the reference's voxelgrid_sampling / randomgrid_sampling (src/gtsam_points/types/point_cloud_cpu_funcs.cpp:119-295, 298-456) and the checks of
tests/test_sampling_gpu.py.  A helper, not a test; it reads nothing outside the repository.

voxelgrid_reference(points, attrs, resolution, block_size)
  key        :128,136  coord = fast_floor(double(p) * (1.0 / resolution)) + 2^20 per axis; :143-146  key = z << 42 | y << 21 | x
  invalid    :132-140  a point that is not finite, or whose offset coordinate leaves [0, 2^21 - 1], gets the key int64 max
  order      :156      sorted by key (here stably: ascending point index inside a key)
  rows       :188-245  block_size = 1024 restates the reference literally: the sorted array is cut into blocks of 1024 and every run of equal keys INSIDE a block
                       becomes a row (Averager, :95-116: f64 sum in ascending order / count) -- so a voxel that straddles a cut appears once per block, and the
                       invalid points form a trailing group of rows.  block_size = None is the device's contract: the valid points only, one row per voxel.
"""
import math

import numpy as np

COORD_BITS = 21
COORD_OFFSET = 1 << (COORD_BITS - 1)
COORD_MASK = (1 << COORD_BITS) - 1
INVALID_KEY = np.iinfo(np.int64).max  # :124


def voxel_keys(points, resolution):
    """-> (keys int64 [N] (INVALID_KEY where dropped), valid bool [N])"""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    inv = 1.0 / float(resolution)
    with np.errstate(invalid="ignore", over="ignore"):
        u = np.floor(p * inv)
        finite = np.isfinite(p).all(axis=1)
        ok = finite & (u >= -COORD_OFFSET).all(axis=1) & (u <= COORD_MASK - COORD_OFFSET).all(axis=1)
    c = np.where(ok[:, None], u, 0.0).astype(np.int64) + COORD_OFFSET
    keys = (c[:, 2] << (2 * COORD_BITS)) | (c[:, 1] << COORD_BITS) | c[:, 0]
    return np.where(ok, keys, INVALID_KEY), ok


def key_coords(keys):
    """packed key -> (x, y, z) voxel coordinates"""
    k = np.asarray(keys, dtype=np.int64)
    return np.stack([(k & COORD_MASK) - COORD_OFFSET, ((k >> COORD_BITS) & COORD_MASK) - COORD_OFFSET, ((k >> (2 * COORD_BITS)) & COORD_MASK) - COORD_OFFSET], axis=1)


def _as_rows(a, n):
    return np.asarray(a, dtype=np.float32).reshape(n, -1)


def voxelgrid_reference(points, attrs, resolution, block_size=None):
    """attrs: {name: float32 (N, w) or (N,)}.  -> dict(keys [R], counts [R], starts [R], order [N'], means {name: f64 (R, w)}, abs_sums {name: f64 (R, w)})
    abs_sums = sum |x_i| per row and column, the quantity the error bound of assert_voxelgrid needs."""
    n = len(points)
    keys, ok = voxel_keys(points, resolution)
    if block_size is None:
        idx = np.flatnonzero(ok)
        order = idx[np.argsort(keys[idx], kind="stable")]
    else:
        order = np.argsort(keys, kind="stable")
    sk = keys[order]
    m = len(order)
    if m == 0:
        z = np.zeros(0, np.int64)
        return dict(keys=z, counts=z, starts=z, order=order, means={a: np.zeros((0, _as_rows(v, n).shape[1])) for a, v in attrs.items()},
                    abs_sums={a: np.zeros((0, _as_rows(v, n).shape[1])) for a, v in attrs.items()})
    head = np.ones(m, bool)
    head[1:] = sk[1:] != sk[:-1]
    if block_size is not None:
        head[::block_size] = True  # :197: every block starts a row of its own
    starts = np.flatnonzero(head)
    counts = np.diff(np.append(starts, m))
    means, abs_sums = {}, {}
    for a, v in attrs.items():
        x = _as_rows(v, n)[order].astype(np.float64)
        with np.errstate(invalid="ignore"):
            means[a] = np.add.reduceat(x, starts, axis=0) / counts[:, None]
            abs_sums[a] = np.add.reduceat(np.abs(x), starts, axis=0)
    return dict(keys=sk[starts], counts=counts, starts=starts, order=order, means=means, abs_sums=abs_sums)


def collapse_blocks(lit):
    """the literal (block_size = 1024) rows with consecutive rows of equal key merged, weighted by count, and the invalid group dropped"""
    keep = lit["keys"] != INVALID_KEY
    keys, counts = lit["keys"][keep], lit["counts"][keep]
    head = np.ones(len(keys), bool)
    head[1:] = keys[1:] != keys[:-1]
    starts = np.flatnonzero(head)
    total = np.add.reduceat(counts, starts) if len(keys) else counts
    means = {}
    for a, mu in lit["means"].items():
        w = mu[keep] * counts[:, None]
        means[a] = (np.add.reduceat(w, starts, axis=0) / total[:, None]) if len(keys) else mu[keep]
    return dict(keys=keys[starts] if len(keys) else keys, counts=total, means=means)


def ulp32(x):
    """the spacing of float32 at |x| (x: f64 array)"""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def row_bound(ref, name):
    """|got - ref| <= ulp32(ref) + m 2^-52 sum |x_i|: an f64 sum of m f32 values, in whatever order, errs by at most the second term (and the division by one
    rounding more, which it covers: m >= 1 and the bound on a sum of m terms is (m - 1) 2^-53 sum |x_i|); two correctly rounded f32 values of f64 numbers that
    close lie at most one f32 ulp apart"""
    return ulp32(ref["means"][name]) + ref["counts"][:, None] * 2.0 ** -52 * ref["abs_sums"][name]


def assert_voxelgrid(got, ref, what="", quiet=False):
    """got: {name: float32 (V, w)} in voxel order; ref: voxelgrid_reference(..., block_size=None).  Same number of voxels, same order, every row inside row_bound.
    No row is exempt.  Names the first voxel that fails.  Returns {name: worst |got - ref| / bound}."""
    V = len(ref["keys"])
    figs = {}
    for a, g in got.items():
        g = np.asarray(g, dtype=np.float32).reshape(len(g), -1).astype(np.float64)
        r, bound = ref["means"][a], row_bound(ref, a)
        rows = min(len(g), V)
        with np.errstate(invalid="ignore"):
            bad = ~(np.abs(g[:rows] - r[:rows]) <= bound[:rows]).all(axis=1)
        if bad.any():
            v = int(np.flatnonzero(bad)[0])
            x, y, z = key_coords(ref["keys"][v : v + 1])[0]
            raise AssertionError(f"{what}: {a}: voxel {v} (coordinate {x}, {y}, {z}; {int(ref['counts'][v])} points): got {g[v]}, reference {r[v]}, bound {bound[v]}"
                                 + (f"; {len(g)} rows for {V} voxels" if len(g) != V else ""))
        if len(g) != V:
            raise AssertionError(f"{what}: {a}: {len(g)} rows for {V} voxels: voxel {rows} is {'missing' if len(g) < V else 'not in the reference'}")
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(bound > 0, np.abs(g - r) / bound, 0.0)
        figs[a] = float(ratio.max()) if ratio.size else 0.0
    if not quiet:
        print(f"{what}: {V} voxels, worst |got - ref| / bound " + ", ".join(f"{a} {f:.3f}" for a, f in figs.items()))
    return figs


# ---- randomgrid_sampling -------------------------------------------------------------------------------------------------------------------------------------------
def randomgrid_figures(points, resolution, rate):
    """:377-378 with N = the valid points and the voxels = the occupied voxels (the device's contract; the reference counts the key changes, invalid group included)"""
    keys, ok = voxel_keys(points, resolution)
    uniq, inverse, counts = np.unique(keys[ok], return_inverse=True, return_counts=True)
    N, V = int(ok.sum()), len(uniq)
    voxel_of = np.full(len(keys), -1, np.int64)
    voxel_of[ok] = inverse
    ppv = int(math.ceil((rate * N) / V)) if V else 0
    cap = int(N * rate * 1.2)
    uncapped = int(np.minimum(counts, ppv).sum())
    return dict(N=N, V=V, counts=counts, voxel_of=voxel_of, valid=ok, points_per_voxel=ppv, cap=cap, uncapped_total=uncapped, cap_binds=uncapped > cap)


def check_randomgrid(points, resolution, rate, indices, what="", figs=None):
    """indices strictly ascending and valid; per voxel min(count, points_per_voxel) rows whenever the cap does not bind, never more; the total <= the cap always (and
    equal to it when it binds); rate >= 0.99: every valid point.  Returns the per-voxel kept counts."""
    f = figs or randomgrid_figures(points, resolution, rate)
    idx = np.asarray(indices).astype(np.int64).reshape(-1)
    assert (np.diff(idx) > 0).all(), f"{what}: indices not strictly ascending"
    assert len(idx) == 0 or (idx[0] >= 0 and idx[-1] < len(f["valid"])), f"{what}: index out of range"
    assert f["valid"][idx].all(), f"{what}: a dropped point was selected"
    kept = np.bincount(f["voxel_of"][idx], minlength=f["V"])
    if rate >= 0.99:
        assert len(idx) == f["N"], f"{what}: rate {rate} must keep all {f['N']} valid points, kept {len(idx)}"
        return kept
    want = np.minimum(f["counts"], f["points_per_voxel"])
    assert (kept <= want).all(), f"{what}: voxel {int(np.flatnonzero(kept > want)[0])} keeps more than min(count, points_per_voxel)"
    assert len(idx) <= f["cap"], f"{what}: {len(idx)} points exceed the cap {f['cap']}"
    if f["cap_binds"]:
        assert len(idx) == f["cap"], f"{what}: the cap binds ({f['uncapped_total']} > {f['cap']}) but {len(idx)} points were kept"
    else:
        assert (kept == want).all(), f"{what}: voxel {int(np.flatnonzero(kept != want)[0])} keeps {kept[kept != want][0]} of min(count, points_per_voxel) = {want[kept != want][0]}"
    return kept


def _mix32(x):
    x = np.asarray(x, dtype=np.uint64) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def sample_hash(seed, index):
    """csrc/gp_sampling.hip sample_hash: the rank value of (seed, point index)"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    a = int(_mix32((seed & 0xFFFFFFFF) ^ 0x9E3779B9))
    b = int(_mix32(((seed >> 32) + 0x7F4A7C15 + a) & 0xFFFFFFFF))
    return _mix32((_mix32(np.asarray(index, dtype=np.uint64) ^ np.uint64(b)) + np.uint64(a)) & 0xFFFFFFFF).astype(np.uint32)


def randomgrid_reference(points, resolution, rate, seed):
    """the device's selection, restated: per voxel the points_per_voxel smallest (hash, index); beyond the cap the cap smallest (hash, index) of those; ascending"""
    f = randomgrid_figures(points, resolution, rate)
    valid = np.flatnonzero(f["valid"])
    if rate >= 0.99 or f["N"] == 0:
        return valid
    h = sample_hash(seed, valid).astype(np.int64)
    o = np.lexsort((valid, h, f["voxel_of"][valid]))  # by voxel, then hash, then index
    v_sorted = f["voxel_of"][valid][o]
    start = np.concatenate([[0], np.cumsum(f["counts"])[:-1]])
    rank = np.arange(len(o)) - start[v_sorted]
    sel = np.sort(valid[o[rank < f["points_per_voxel"]]])
    if len(sel) > f["cap"]:
        hs = sample_hash(seed, sel).astype(np.int64)
        sel = np.sort(sel[np.lexsort((sel, hs))[: f["cap"]]])
    return sel


def check_uniform(select_counts, trials, p, what=""):
    """every point's selection count within 5 standard deviations of trials * p (binomial: sigma = sqrt(trials p (1 - p)))"""
    c = np.asarray(select_counts, dtype=np.float64)
    mean, sigma = trials * p, math.sqrt(trials * p * (1.0 - p))
    worst = float(np.abs(c - mean).max() / sigma)
    assert worst <= 5.0, f"{what}: point {int(np.abs(c - mean).argmax())} selected {int(c[np.abs(c - mean).argmax()])} times of {trials}: {worst:.2f} sigma from {mean}"
    return worst

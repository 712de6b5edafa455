"""match_features_gpu against the brute-force search of tests/ransac_ref.py.

Bounds (derived, not measured):
  index      exact.  The random rows have no two targets at the same distance from a query (asserted on the restatement's own distances: ties == 1), and the gaps
             between the best and the second best are many orders above the rounding of a sum; for the planted duplicate the lower of the two indices, as the restatement's.
  distance   |d_gpu - d_ref| <= (D + 4) 2^-52 d_ref: D correctly rounded operations per sum, in either order or fused (2^-53 each, on either side), and the
             subtractions of f32 values in f64 (one rounding each, <= 2^-53 relative to a term)."""
import functools

import numpy as np
import pytest

import ransac_ref as rr

pytestmark = pytest.mark.gpu

DIMS = (1, 33, 125, 128)
TARGETS = (1, 255, 256, 257)
QUERIES = (1, 65)


@functools.lru_cache(maxsize=None)
def case(d, nt, nq, with_rows):
    rng = np.random.default_rng(1000 * d + 10 * nt + nq + int(with_rows))
    tf = rng.normal(size=(nt, d)).astype(np.float32)
    ns = nq if not with_rows else 3 * nq + 2
    sf = rng.normal(size=(ns, d)).astype(np.float32)
    rows = rng.integers(0, ns, size=nq).astype(np.int32) if with_rows else None  # (repeated rows allowed)
    idx, sq, ties = rr.match_features(tf, sf, rows)
    return tf, sf, rows, idx, sq, ties


@pytest.mark.parametrize("with_rows", [False, True])
@pytest.mark.parametrize("nq", QUERIES)
@pytest.mark.parametrize("nt", TARGETS)
@pytest.mark.parametrize("d", DIMS)
def test_nearest_feature_rows(gpu, d, nt, nq, with_rows):
    tf, sf, rows, idx, sq, ties = case(d, nt, nq, with_rows)
    assert (ties == 1).all()
    gi, gd = gpu.match_features_gpu(tf, sf, rows)
    gi, gd = gi.cpu().numpy(), gd.cpu().numpy()
    assert gi.dtype == np.int32 and gd.dtype == np.float64 and gi.shape == (nq,) and gd.shape == (nq,)
    assert np.array_equal(gi, idx)
    err = np.abs(gd - sq)
    bound = (d + 4) * 2.0 ** -52 * sq
    print(f"D {d} nt {nt} nq {nq}: worst |d_gpu - d_ref| = {float((err / np.maximum(bound, 1e-300)).max()):.3f} of the bound (D + 4) 2^-52 d")
    assert (err <= bound).all()


@pytest.mark.parametrize("d", DIMS)
def test_planted_duplicate_target_row(gpu, d):
    tf, sf, _, _, _, _ = case(d, 257, 65, False)
    tf = tf.copy()
    idx0, _, _ = rr.match_features(tf, sf)
    a = int(idx0[0])
    b = (a + 130) % 257  # another tile of 64 targets
    tf[b] = tf[a]
    idx, sq, ties = rr.match_features(tf, sf)
    assert ties[0] == 2
    gi, gd = gpu.match_features_gpu(tf, sf)
    gi, gd = gi.cpu().numpy(), gd.cpu().numpy()
    assert idx[0] == min(a, b) and np.array_equal(gi, idx)  # the lowest index among exact ties (b lies below a for some D, above for others)
    assert (np.abs(gd - sq) <= (d + 4) * 2.0 ** -52 * sq).all()


def test_torch_inputs_and_refusals(gpu):
    import torch

    tf, sf, rows, idx, sq, _ = case(33, 257, 65, True)
    gi, _ = gpu.match_features_gpu(torch.from_numpy(tf).cuda(), torch.from_numpy(sf).cuda(), torch.from_numpy(rows).cuda())
    assert np.array_equal(gi.cpu().numpy(), idx)
    with pytest.raises(gpu.GPError):
        gpu.match_features_gpu(np.zeros((4, 129), np.float32), np.zeros((4, 129), np.float32))  # D = 129
    with pytest.raises(gpu.GPError):
        gpu.match_features_gpu(np.zeros((4, 33), np.float32), np.zeros((4, 32), np.float32))
    with pytest.raises(gpu.GPError):
        gpu.match_features_gpu(np.zeros((0, 33), np.float32), np.zeros((4, 33), np.float32))
    with pytest.raises(IndexError):
        gpu.match_features_gpu(tf, sf, [0, len(sf)])

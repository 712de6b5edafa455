"""Inputs and f64 statements of the factor-domain sweep (tests/test_factor_domain_gpu.py, tests/test_factor_domain_ref_cpu.py).  A helper, not a test.

The scene is synthetic and analytic: three mutually non-parallel planes (a floor and two walls) inside a 24 m box, sampled at random positions (no lattice) with
1 cm of jitter along the normal, covariances V diag(1e-3, 1, 1) V^T = I - 0.999 n n^T from each plane's normal.  The target has 3 x 2000 points, the source
4097 (one 4096-point tile plus one) drawn anew from the same planes.  The source stays in its sensor frame; place() moves the target into a world frame W and
rounds it to f32, so that the reference sees the f32 inputs the device sees.

Condition on the inputs (tests/test_cloud_edges_gpu.py's): two correct f64 implementations only put a point into the same voxel when its voxel coordinate
u = l / leaf is not within rounding of an integer.  Points with |u - rint(u)| <= MARGIN * max(1, |u|) on any axis are removed, from the target when it is placed
and from the source when a case is made, BEFORE either side runs; no case may lose more than DROP_CAP of its source this way.

References: VGICP oracle/vgicp_oracle_np.py (all f64), ICP tests/icp_ref.py, GICP the oracle's C factor.  vgicp_terms() restates vgicp_linearize per point in any
numpy float type (np.longdouble for the precision check) and also returns the sums of the per-point norms of b's terms, the yardstick of "b is not a cancellation"."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import vgicp_oracle_np as onp  # noqa: E402

LEAF = 1.0
MARGIN = 1e-9
DROP_CAP = 0.01
SEED = 20250
N_TARGET_PER_PLANE, N_SOURCE = 2000, 4097
DISTANCES = [0.0, 100.0, 1000.0, 10000.0]
DIRECTION = np.array([0.6, -0.64, 0.48])  # unit, no axis, one negative component
AXIS = np.array([1.0, 2.0, -2.0]) / 3.0   # unit, skew
ROTATIONS = {"0.4rad": 0.4, "pi-1e-3": np.pi - 1e-3}
SMALL = np.array([0.01, -0.02, 0.015, 0.10, -0.05, 0.03])
CONTROL = np.array([1e-4, -2e-4, 1.5e-4, 0.10, -0.05, 0.03])  # both clouds far: a rotation of 1e-4 rad moves a point at 1 km by 0.1 m
EVAL = np.concatenate([np.zeros(3), 0.1 * np.array([0.48, 0.6, 0.64])])  # the 0.1 m offset of the evaluation pose (keeps b from being a pure cancellation)
SCALES = [0.01, 1.0, 100.0]
# (normal, a point of the plane, in-plane half extents)
PLANES = [
    (np.array([0.02, -0.03, 1.0]), np.array([0.0, 0.0, -1.8]), (11.5, 11.5)),
    (np.array([1.0, 0.04, 0.02]), np.array([11.0, 0.0, 0.6]), (11.0, 2.2)),
    (np.array([-0.03, 1.0, 0.05]), np.array([0.0, -10.5, 0.6]), (11.0, 2.2)),
]


def expmap(xi):
    return onp.expmap(xi)


def world_pose(distance, rotation):
    """W: rotation by ROTATIONS[rotation] about AXIS, translation distance * DIRECTION"""
    W = expmap(np.concatenate([ROTATIONS[rotation] * AXIS, np.zeros(3)]))
    W[:3, 3] = distance * DIRECTION
    return W


def _sample(rng, n_per_plane):
    pts, nrm = [], []
    for k, (n, c, (ha, hb)) in enumerate(PLANES):
        n = n / np.linalg.norm(n)
        u = np.cross(n, [0.0, 0.0, 1.0] if k else [1.0, 0.0, 0.0])
        u /= np.linalg.norm(u)
        v = np.cross(n, u)
        m = n_per_plane[k]
        a, b, e = rng.uniform(-ha, ha, m), rng.uniform(-hb, hb, m), rng.normal(0.0, 0.01, m)
        pts.append(c + a[:, None] * u + b[:, None] * v + e[:, None] * n)
        nrm.append(np.broadcast_to(n, (m, 3)))
    pts, nrm = np.concatenate(pts), np.concatenate(nrm)
    order = rng.permutation(len(pts))  # (a tile then holds points of every plane)
    return pts[order], nrm[order]


def plane_covs(normals):
    """V diag(1e-3, 1, 1) V^T with V's first column the normal"""
    return np.eye(3)[None] - 0.999 * normals[:, :, None] * normals[:, None, :]


_SCENES = {}


def scene(seed=SEED):
    """f64 scene in the sensor frame: target / source points, unit normals, covariances (shared between the tests, never written to)"""
    if seed not in _SCENES:
        rng = np.random.default_rng(seed)
        tp, tn = _sample(rng, [N_TARGET_PER_PLANE] * 3)
        sp, sn = _sample(rng, [N_SOURCE - 2 * (N_SOURCE // 3), N_SOURCE // 3, N_SOURCE // 3])
        assert np.abs(tp).max() < 12.0 and np.abs(sp).max() < 12.0 and len(sp) == N_SOURCE
        s = dict(target_points=tp, target_normals=tn, target_covs=plane_covs(tn), source_points=sp, source_normals=sn, source_covs=plane_covs(sn))
        for a in s.values():
            a.setflags(write=False)
        _SCENES[seed] = s
    return _SCENES[seed]


def face_margins(points, delta, leaf):
    """per point: the smallest distance, in cells, of a transformed voxel coordinate from an integer, relative to max(1, |u|)"""
    delta = np.asarray(delta, dtype=np.float64)
    u = (np.asarray(points, dtype=np.float64) @ delta[:3, :3].T + delta[:3, 3]) * (1.0 / float(leaf))
    return (np.abs(u - np.rint(u)) / np.maximum(np.abs(u), 1.0)).min(axis=1)


def move(points, normals, covs, W, scale=1.0):
    """(W p, R n, R C R^T) * (scale, 1, scale^2), rounded to f32 (what both sides are given)"""
    R, t = W[:3, :3], W[:3, 3]
    p = ((points @ R.T + t) * scale).astype(np.float32)
    n = (normals @ R.T).astype(np.float32)
    c = (np.einsum("ij,njk,lk->nil", R, covs, R) * scale**2).astype(np.float32)
    return p, n, c


def place(s, W, leaf=LEAF, scale=1.0):
    """the target of scene `s` in world frame W (scaled), f32, without the points on a voxel face; the source in its sensor frame (scaled), f32"""
    tp, tn, tc = move(s["target_points"], s["target_normals"], s["target_covs"], W, scale)
    keep = face_margins(tp, np.eye(4), leaf) > MARGIN
    sp, sn, sc = move(s["source_points"], s["source_normals"], s["source_covs"], np.eye(4), scale)
    return dict(target_points=tp[keep], target_normals=tn[keep], target_covs=tc[keep], source_points=sp, source_normals=sn, source_covs=sc, W=W, leaf=leaf,
                target_dropped=int((~keep).sum()))


def with_margin(d, delta, leaf=None):
    """the placed inputs `d` with the source points on a voxel face at `delta` removed -> (inputs, dropped share)"""
    keep = face_margins(d["source_points"], delta, leaf or d["leaf"]) > MARGIN
    out = dict(d)
    for k in ("source_points", "source_normals", "source_covs"):
        out[k] = d[k][keep]
    return out, float((~keep).mean())


def scan_to_map(distance, rotation, seed=SEED):
    """case (a): target in W, source in its sensor frame -> (inputs, delta, delta_eval, dropped share)"""
    W = world_pose(distance, rotation)
    d = place(scene(seed), W)
    delta = W @ expmap(SMALL)
    d, dropped = with_margin(d, delta)
    return d, delta, delta @ expmap(EVAL), dropped


def both_far(distance=1000.0, rotation="0.4rad", seed=SEED):
    """case (b): source and target both in W, the relative pose near identity"""
    W = world_pose(distance, rotation)
    s = scene(seed)
    d = place(s, W)
    d["source_points"], d["source_normals"], d["source_covs"] = move(s["source_points"], s["source_normals"], s["source_covs"], W)
    delta = expmap(CONTROL)
    d, dropped = with_margin(d, delta)
    return d, delta, delta @ expmap(EVAL), dropped


def scaled(scale, seed=SEED):
    """case (c): the whole scene in units of 1 / scale metres, at the origin"""
    d = place(scene(seed), np.eye(4), LEAF * scale, scale)
    delta = expmap(SMALL)
    delta[:3, 3] *= scale
    step = expmap(EVAL)
    step[:3, 3] *= scale
    d, dropped = with_margin(d, delta)
    return d, delta, delta @ step, dropped


def vgicp_reference(d, delta, delta_eval=None):
    """oracle/vgicp_oracle_np.py on the placed inputs -> (record at delta, error at delta_eval on delta's correspondences or None)"""
    vm = onp.VoxelMapNP(d["leaf"])
    vm.insert(d["target_points"], d["target_covs"])
    L = onp.vgicp_linearize(vm, d["source_points"], d["source_covs"], delta)
    e = None if delta_eval is None else onp.vgicp_linearize(vm, d["source_points"], d["source_covs"], delta, delta_eval)["error"]
    return L, e


def _hat(v, dt):
    z = np.zeros(len(v), dtype=dt)
    return np.stack([np.stack([z, -v[:, 2], v[:, 1]], -1), np.stack([v[:, 2], z, -v[:, 0]], -1), np.stack([-v[:, 1], v[:, 0], z], -1)], -2)


def _inv3(A):
    """inverse of (N,3,3) matrices by cofactors, in A's own float type (numpy.linalg has no long double)"""
    a, b, c, d, e, f, g, h, i = (A[:, r, s] for r in range(3) for s in range(3))
    co = np.stack([np.stack([e * i - f * h, c * h - b * i, b * f - c * e], -1), np.stack([f * g - d * i, a * i - c * g, c * d - a * f], -1),
                   np.stack([d * h - e * g, b * g - a * h, a * e - b * d], -1)], -2)
    det = a * co[:, 0, 0] + b * co[:, 1, 0] + c * co[:, 2, 0]
    return co / det[:, None, None]


def vgicp_terms(d, delta, delta_eval=None, dtype=np.float64, subset=None):
    """vgicp_linearize restated point by point in `dtype` (sums included) on the first `subset` source points; the voxel means and covariances are accumulated in
    `dtype` as well.  Besides the record: term_b_source / term_b_target = sum_n ||J_n^T M_n r_n||, the size b would have if nothing cancelled."""
    dt = dtype
    tp, tc = d["target_points"].astype(dt), d["target_covs"].astype(dt).reshape(-1, 3, 3)
    coords = onp.fast_floor(d["target_points"].astype(np.float64) * (1.0 / d["leaf"]))
    uniq, inv = np.unique(coords, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    cnt = np.bincount(inv, minlength=len(uniq)).astype(dt)
    means, covs = np.zeros((len(uniq), 3), dt), np.zeros((len(uniq), 3, 3), dt)
    np.add.at(means, inv, tp)
    np.add.at(covs, inv, tc)
    means, covs = means / cnt[:, None], covs / cnt[:, None, None]
    index = {tuple(k): i for i, k in enumerate(uniq.tolist())}
    p = d["source_points"][:subset].astype(dt)
    CA = d["source_covs"][:subset].astype(dt).reshape(-1, 3, 3)
    T, Te = np.asarray(delta).astype(dt), np.asarray(delta if delta_eval is None else delta_eval).astype(dt)
    R, t, Re, te = T[:3, :3], T[:3, 3], Te[:3, :3], Te[:3, 3]
    ql = p @ R.T + t
    vid = np.array([index.get(tuple(k), -1) for k in onp.fast_floor(ql.astype(np.float64) * (1.0 / d["leaf"])).tolist()], dtype=np.int64)
    ok = vid >= 0
    p, CA, vid = p[ok], CA[ok], vid[ok]
    M = _inv3(covs[vid] + np.einsum("ij,njk,lk->nil", R, CA, R))
    q = p @ Re.T + te
    r = means[vid] - q
    eye = np.broadcast_to(np.eye(3, dtype=dt), (len(q), 3, 3))
    Jt = np.concatenate([-_hat(q, dt), eye], axis=2)
    Js = np.concatenate([np.einsum("ij,njk->nik", Re, _hat(p, dt)), np.broadcast_to(-Re, (len(q), 3, 3))], axis=2)
    Mr = np.einsum("nij,nj->ni", M, r)
    bt, bs = np.einsum("nki,nk->ni", Jt, Mr), np.einsum("nki,nk->ni", Js, Mr)
    return dict(
        num_inliers=int(ok.sum()),
        error=(r * Mr).sum(),
        H_target=np.einsum("nki,nkl,nlj->ij", Jt, M, Jt),
        H_source=np.einsum("nki,nkl,nlj->ij", Js, M, Js),
        H_target_source=np.einsum("nki,nkl,nlj->ij", Jt, M, Js),
        b_target=bt.sum(0),
        b_source=bs.sum(0),
        term_b_target=float(np.sqrt((bt * bt).sum(1).astype(np.float64)).sum()),
        term_b_source=float(np.sqrt((bs * bs).sum(1).astype(np.float64)).sum()),
    )


def subset_inputs(d, n):
    out = dict(d)
    for k in ("source_points", "source_normals", "source_covs"):
        out[k] = d[k][:n]
    return out


def worst_block(got, ref):
    """(largest norm-wise relative error over the five blocks, its block) -- the figure each sweep test prints; helpers.assert_linearized_close asserts"""
    from helpers import BLOCKS, rel_err

    errs = {k: rel_err(getattr(got, k) if not isinstance(got, dict) else got[k], ref[k] if isinstance(ref, dict) else getattr(ref, k)) for k in BLOCKS}
    k = max(errs, key=errs.get)
    return errs[k], k, errs

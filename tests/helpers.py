"""Shared helpers of the test-suite (parity metrics, tiny LM driver)."""
import numpy as np

BLOCKS = ["H_target", "H_source", "H_target_source", "b_target", "b_source"]


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    n = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / n) if n > 0 else float(np.linalg.norm(a - b))


def assert_linearized_close(got, ref, tol, what=""):
    """norm-wise relative parity on every block (||dH||_F/||H||_F, ||db||_2/||b||_2), error and inlier count"""
    for k in BLOCKS:
        e = rel_err(getattr(got, k), getattr(ref, k) if not isinstance(ref, dict) else ref[k])
        assert e <= tol, f"{what} {k}: relative error {e:.3e} > {tol:.1e}"
    ref_err = ref["error"] if isinstance(ref, dict) else ref.error
    ref_inl = ref["num_inliers"] if isinstance(ref, dict) else ref.num_inliers
    assert abs(got.error - ref_err) <= tol * max(abs(ref_err), 1e-300), f"{what} error {got.error} vs {ref_err}"
    assert got.num_inliers == ref_inl, f"{what} num_inliers {got.num_inliers} vs {ref_inl}"


def expmap(xi):
    from gtsam_points_amd.synthetic import expmap as e

    return e(xi)


def pose_error(T_est, T_gt):
    d = np.linalg.inv(T_gt) @ T_est
    ang = np.arccos(np.clip((np.trace(d[:3, :3]) - 1) / 2, -1, 1))
    return float(ang), float(np.linalg.norm(d[:3, 3]))


def lm_optimize(linearize_all, error_all, values, keys, fixed=(), max_iter=30, rel_tol=1e-4, lam0=1e-5):
    """Minimal Levenberg-Marquardt over SE(3) poses with right perturbations (GTSAM Pose3 retract = Expmap here),
    mirroring LevenbergMarquardtOptimizerExt's loop shape (levenberg_marquardt_ext.cpp:354-398): linearise via the
    hook, try lambdas until the nonlinear error decreases.
      linearize_all(values) -> list of HessianFactor-like (keys, G blocks, g, f)
      error_all(values)     -> total nonlinear error  (sum of factor errors, GTSAM's 0.5 factor is irrelevant here)"""
    free = [k for k in keys if k not in fixed]
    idx = {k: i for i, k in enumerate(free)}
    lam = lam0
    values = dict(values)
    factors = linearize_all(values)
    err = sum(f.f for f in factors)
    for _ in range(max_iter):
        n = 6 * len(free)
        H = np.zeros((n, n))
        g = np.zeros(n)
        for f in factors:
            for (i, j), blk in f.G.items():
                ki, kj = f.keys[i], f.keys[j]
                if ki in idx and kj in idx:
                    a, b = idx[ki] * 6, idx[kj] * 6
                    H[a : a + 6, b : b + 6] += blk
                    if i != j:
                        H[b : b + 6, a : a + 6] += blk.T
            for i, gi in enumerate(f.g):
                if f.keys[i] in idx:
                    a = idx[f.keys[i]] * 6
                    g[a : a + 6] += gi
        improved = False
        for _try in range(12):
            dx = np.linalg.solve(H + lam * np.diag(np.diag(H)) + 1e-9 * np.eye(n), g)
            new_values = dict(values)
            for k in free:
                new_values[k] = values[k] @ expmap(dx[idx[k] * 6 : idx[k] * 6 + 6])
            # evaluate with correspondences frozen at the linearisation point (error() semantics)
            new_err = error_all(new_values)
            if new_err < err:
                improved = True
                lam = max(lam / 10.0, 1e-12)
                break
            lam *= 10.0
        if not improved:
            break
        rel = (err - new_err) / max(err, 1e-300)
        values = new_values
        factors = linearize_all(values)
        err = sum(f.f for f in factors)
        if rel < rel_tol:
            break
    return values


def host_system(records, slots, n_slots):
    """DenseLinearSystemBuilder (linear_system_builder.cpp:39-48) on the host: scatter the Hessian blocks by key"""
    A, b, c = np.zeros((6 * n_slots, 6 * n_slots)), np.zeros(6 * n_slots), 0.0
    for rec, (st, ss) in zip(records, slots):
        Ht, Hs, Hts = rec[2:38].reshape(6, 6).T, rec[38:74].reshape(6, 6).T, rec[74:110].reshape(6, 6).T
        bt, bs = rec[110:116], rec[116:122]
        c += rec[1]
        if st >= 0:
            A[6 * st : 6 * st + 6, 6 * st : 6 * st + 6] += Ht
            b[6 * st : 6 * st + 6] -= bt
        if ss >= 0:
            A[6 * ss : 6 * ss + 6, 6 * ss : 6 * ss + 6] += Hs
            b[6 * ss : 6 * ss + 6] -= bs
        if st >= 0 and ss >= 0:
            A[6 * st : 6 * st + 6, 6 * ss : 6 * ss + 6] += Hts
            A[6 * ss : 6 * ss + 6, 6 * st : 6 * st + 6] += Hts.T
    return A, b, c


def kitti_graph(gpu, kitti07, n=5, pairs=None):
    """the kitti07 graph of the LM tests: one voxel map (1 m) per cloud, factors over every pair (or `pairs`), truth and a perturbed start (pose 0 = truth)"""
    import bench_lm

    clouds = [gpu.PointCloudGPU(kitti07[f"points_{i}"], kitti07[f"covs_{i}"]) for i in range(n)]
    maps = []
    for c in clouds:
        vm = gpu.GaussianVoxelMapGPU(1.0, target_points_drop_rate=0.0)
        vm.insert(c)
        maps.append(vm)
    pairs = pairs or [(i, j) for i in range(n) for j in range(i + 1, n)]
    factors = [gpu.IntegratedVGICPFactorGPU(i, j, maps[i], clouds[j]) for i, j in pairs]
    truth = np.stack([np.asarray(T, dtype=np.float64) for T in kitti07["poses"][:n]])
    v0 = truth @ bench_lm.expmap_many(np.random.default_rng(8191).uniform(-0.1, 0.1, (n, 6)))
    v0[0] = truth[0]
    return factors, pairs, truth, v0, (clouds, maps)


def rigid(values):
    """nearest rotations (the fixture's poses come from 6-digit text: orthonormal to 1e-6, which sends the host-pose entry points to the general kernels)"""
    out = np.array(values, dtype=np.float64)
    for T in out:
        u, _, vt = np.linalg.svd(T[:3, :3])
        T[:3, :3] = u @ vt
    return out


def reference_bucket_lookup(buckets, info, coord):
    """lookup_voxel of cuda/kernels/vector3_hash.cuh:53-76 restated on the downloaded bucket table (rows of x, y, z, voxel index): linear probing over at most
    max_bucket_scan_count buckets, stop at an empty one"""
    M, mask = 0xC6A4A7935BD1E995, (1 << 64) - 1

    def combine(h, k):
        k = (k * M) & mask
        k ^= k >> 47
        k = (k * M) & mask
        h ^= k
        h = (h * M) & mask
        return (h + 0xE6546B64) & mask

    h = 0
    for c in coord:
        h = combine(h, int(c) & mask)
    for i in range(info.max_bucket_scan_count):
        b = buckets[((h + i) & mask) % info.num_buckets]
        if b[3] < 0:
            return -1
        if tuple(b[:3]) == tuple(int(c) for c in coord):
            return int(b[3])
    return -1


# the graphs of tests/test_solver_gpu.py::test_one_launch_step_is_bit_identical; tests/test_sparse_cpu.py holds them to the forms of the one-launch step they reach
ONE_LAUNCH_GRAPHS = ["c3:64", "c1:2", "band:16", "band:100", "chain:128", "freechain:40", "isolated", "hub:13"]
ONE_LAUNCH_ORDERINGS = ["auto", "natural", "nd", "amd", "amd1"]


def one_launch_graph(graph):
    """(kind, P, factor slots) of a graph of ONE_LAUNCH_GRAPHS"""
    kind, _, num = graph.partition(":")
    if kind == "c3" or kind == "c1":  # BASELINE configs[2]'s / configs[0]'s graph: pose 0 held
        n = int(num)
        pairs = [(i, j) for i in range(n) for j in range(i + 1, min(i + 5, n))]
        pairs = (pairs + [(j, i) for i, j in pairs])[: 4 * n]
        return kind, n - 1, [(a - 1, b - 1) for a, b in pairs]
    if kind == "band":
        P = int(num)
        return kind, P, [(-1, 0)] + [(i, i + d) for i in range(P) for d in (1, 2, 5) if i + d < P]
    if kind == "chain":
        P = int(num)
        return kind, P, [(-1, 0)] + [(i, i + 1) for i in range(P - 1)]
    if kind == "freechain":  # no pose held: more than eight one-column subtrees under the minimum-degree orderings (several batches of lists per level)
        P = int(num)
        return kind, P, [(i, i + 1) for i in range(P - 1)]
    if kind == "hub":  # every pose tied to pose 0: in the natural order its column has P blocks (more than ten: the panel sweep's second pass of 64 rows)
        P = int(num)
        return kind, P, [(-1, 0)] + [(0, i) for i in range(1, P)]
    return kind, 12, [(-1, 0), (0, 1), (1, 2), (-1, 5), (5, 6), (6, 7), (7, 5), (-1, 11), (-1, 3), (3, 4), (-1, 8), (8, 9), (9, 10)]

"""Host-to-host time of ONE Levenberg-Marquardt iteration (a linearise plus the accepted trial) over GICP / ICP factors, in two forms on the same graph:

  host     driven from the host over the single-factor calls (gp_{gicp,icp}_factor_linearize / _compute_error per factor, the normal equations and the solve in numpy):
           the only way before gp_corr_batch_* -- 3 F launches and F waits per linearise, as many again per error evaluation
  device   LevenbergMarquardtGraphGPU(corr_factors=...): the values in device memory, one wait per trial (gp_lm_graph_create_with_factors)

on the kitti07 graph of tests/test_corr_lm_gpu.py (five submaps, all ten pairs: point-to-plane on (1, 2), point-to-point on (3, 4), GICP elsewhere; pose 0 held; start =
truth o Expmap(U(-0.02, 0.02)^6)).  Each form runs its loop from that start; after a handful of iterations the steps are tiny and every iteration does the same work, which
is what is timed: --warmup iterations (default 20), then --reps (default 200) timed ones, min and median.

Then the batch's synchronous linearise of a 256-factor graph (synthetic.make_c3_graph: 64 submaps of 20-25 k points, 256 GICP factors) against 256 single-factor
linearises of the same factors at the same poses.

Neither loop applies the accept test: every iteration takes its step (the device form calls accept() unconditionally), so that each timed iteration is the same work.

One JSON object per line; --out <file> writes them there too.  The device time of the kernels comes from a SEPARATE run of the LM part under rocprofv3 (kernel trace and
statistics only, no counters in the same run); its kernel statistics are kept as profiles/corr_lm_kernel_stats.csv.  Run each under a time limit:

  timeout -k 10 600 python scripts/corr_lm_time.py --out profiles/corr_lm_time.json
  timeout -k 10 300 rocprofv3 --kernel-trace --stats -d /tmp/corr_prof -o corr -- python scripts/corr_lm_time.py --only lm --reps 50 --warmup 10
  (the statistics: /tmp/corr_prof/corr_kernel_stats.csv)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

torch.set_num_threads(16)
import bench_lm  # noqa: E402
import gtsam_points_amd as gpa  # noqa: E402
from gtsam_points_amd import synthetic  # noqa: E402


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


reps, warmup, out_path, only = arg("--reps", 200), arg("--warmup", 20), arg("--out", ""), arg("--only", "")
assert torch.cuda.is_available(), "corr_lm_time.py measures on the GPU"
rows = []


def emit(**row):
    row["device"] = torch.cuda.get_device_name(0)
    rows.append(row)
    print(json.dumps(row), flush=True)


def stats(ms):
    a = np.asarray(ms)
    q1, q3 = np.percentile(a, [25, 75])
    return dict(reps=len(a), ms_min=round(float(a.min()), 4), ms_median=round(float(np.median(a)), 4), ms_iqr=round(float(q3 - q1), 4))


def record_of(L):
    return np.concatenate([[float(L.num_inliers), float(L.error)], L.H_target.T.ravel(), L.H_source.T.ravel(), L.H_target_source.T.ravel(), L.b_target, L.b_source])


class HostGraph(bench_lm._Graph):
    """the single-factor calls, one factor after the other (what tests/corr_graph_ref.py drives)"""

    def __init__(self, factors, pairs, n):
        super().__init__(pairs, n, fixed=0)
        self.f = factors

    def linearize(self, values):
        self.d_lin = self.deltas(values)
        rec = np.array([record_of(f.linearize_delta(d)) for f, d in zip(self.f, self.d_lin)])
        self.A, self.b, c = bench_lm.host_system(rec, self.factor_slots, self.num_slots)
        return c

    def solve(self, lam):
        return np.linalg.solve(self.A + lam * np.eye(len(self.b)), self.b)

    def error(self, values):
        return float(sum(f.error({f.keys()[0]: np.eye(4), f.keys()[1]: d}) for f, d in zip(self.f, self.deltas(values))))


def rigid(values):
    out = np.array(values, dtype=np.float64)
    for T in out:
        u, _, vt = np.linalg.svd(T[:3, :3])
        T[:3, :3] = u @ vt
    return out


def kitti07_graph():
    d = np.load(os.path.join(ROOT, "tests", "golden", "kitti07_dec4.npz"))
    n = 5
    clouds = [gpa.PointCloudGPU(d[f"points_{i}"], d[f"covs_{i}"]) for i in range(n)]
    for c in clouds:
        gpa.estimate_normals_gpu(c)  # (read off the covariances)
    trees = [gpa.KdTreeGPU(c) for c in clouds]
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
    factors = []
    for i, j in pairs:
        if (i, j) == (1, 2):
            factors.append(gpa.IntegratedICPFactorGPU(i, j, clouds[i], clouds[j], target_tree=trees[i], use_point_to_plane=True))
        elif (i, j) == (3, 4):
            factors.append(gpa.IntegratedICPFactorGPU(i, j, clouds[i], clouds[j], target_tree=trees[i]))
        else:
            factors.append(gpa.IntegratedGICPFactorGPU(i, j, clouds[i], clouds[j]))
    truth = rigid(np.stack([np.asarray(T, dtype=np.float64) for T in d["poses"][:n]]))
    v0 = truth @ bench_lm.expmap_many(np.random.default_rng(8191).uniform(-0.02, 0.02, (n, 6)))
    v0[0] = truth[0]
    return factors, pairs, rigid(v0), (clouds, trees)


def lm_iteration_times():
    factors, pairs, v0, keep = kitti07_graph()
    n, lam = len(v0), 1e-5
    points = int(sum(f.source.size() for f in factors))
    # (a) the host-driven loop: linearise, solve, retract, error at the new values, take the step
    host = HostGraph(factors, pairs, n)
    values, ms = v0.copy(), []
    for it in range(warmup + reps):
        t = time.perf_counter()
        host.linearize(values)
        new = host.retract(values, host.solve(lam))
        host.error(new)
        values = new
        if it >= warmup:
            ms.append((time.perf_counter() - t) * 1e3)
    emit(graph="kitti07: 5 submaps, 10 factors (8 GICP, 1 ICP point, 1 ICP plane)", form="host: single-factor calls", source_points=points, **stats(ms))
    # (b) the device-resident graph: linearise, the trial (step + retract + error evaluation: one wait), accept
    for spec in (True, False):
        g = gpa.LevenbergMarquardtGraphGPU([], [], n, fixed=(0,), corr_factors=factors, corr_pairs=pairs)
        g.set_speculation(spec)
        g.set_values(v0)
        ms = []
        for it in range(warmup + reps):
            t = time.perf_counter()
            g.linearize()
            g.try_lambda(lam)
            g.accept()
            if it >= warmup:
                ms.append((time.perf_counter() - t) * 1e3)
        g.sync()
        emit(graph="kitti07: 5 submaps, 10 factors (8 GICP, 1 ICP point, 1 ICP plane)", form="device: LevenbergMarquardtGraphGPU(corr_factors)", speculation=spec,
             source_points=points, **stats(ms))
        g.close()
    del keep


def batch_linearize_times():
    g = synthetic.make_c3_graph()
    clouds = [gpa.PointCloudGPU(p, c) for p, c in g["clouds"]]
    factors = [gpa.IntegratedGICPFactorGPU(i, j, clouds[i], clouds[j]) for i, j in g["pairs"]]
    deltas = rigid(np.stack(g["deltas"]))
    batch = gpa.CorrespondenceFactorBatchGPU(factors)
    points = int(sum(f.source.size() for f in factors))
    r = reps
    for _ in range(3):
        recs = batch.linearize_deltas(deltas)
        single = [f.linearize_delta(d) for f, d in zip(factors, deltas)]
    same = all(np.array_equal(a.H_source, b.H_source) and a.error == b.error for a, b in zip(recs, single))
    p16 = batch._records_order(deltas)
    out = np.zeros((len(factors), 122))
    tb, ts = [], []
    for _ in range(r):
        t = time.perf_counter()
        gpa._capi.check(batch._lib.gp_corr_batch_linearize(batch._h, p16.ctypes.data, 1, out.ctypes.data), "gp_corr_batch_linearize")
        tb.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter()
        for f, d in zip(factors, deltas):
            f.linearize_delta(d)
        ts.append((time.perf_counter() - t) * 1e3)
    emit(graph="make_c3_graph: 256 GICP factors over 64 submaps", form="gp_corr_batch_linearize", source_points=points, bit_identical_to_single_calls=bool(same), **stats(tb))
    emit(graph="make_c3_graph: 256 GICP factors over 64 submaps", form="256 x gp_gicp_factor_linearize", source_points=points, **stats(ts))
    batch.close()


if only in ("", "lm"):
    lm_iteration_times()
if only in ("", "batch"):
    batch_linearize_times()
if out_path:
    with open(out_path, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")

"""pose_factor_time.py -- what Pose3 between / prior factors cost the device-resident LM graph (gp_lm_graph_*, csrc/gp_lm.hip + csrc/gp_pose_factors.hip).

  c3        BASELINE configs[2] (256 VGICP factors / 64 submaps) from ground truth o Expmap(U(-0.1, 0.1)^6): pose 0 held, against the same graph plus a prior on pose 0
            (precision 1e6) and 63 between factors along the chain, nothing held; gp_lm_graph_optimize's ms per iteration, median of repeated runs
  pgo       a pure pose graph of 1000 poses (chain + a loop closure every 25 poses, one prior), the same figure
  --kernel-only   only the runs a rocprofv3 --kernel-trace --stats pass needs (the c3 graph with pose factors, a few optimize calls)

Prints one JSON line; --out FILE writes it too."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench_lm  # noqa: E402


def _rigid(values):
    out = np.array(values, dtype=np.float64)
    for T in out:
        u, _, vt = np.linalg.svd(T[:3, :3])
        T[:3, :3] = u @ vt
    return out


def _inv(T):
    return bench_lm.inv_many(T[None])[0]


def _exp(xi):
    return bench_lm.expmap_many(np.asarray(xi, dtype=np.float64).reshape(1, 6))[0]


def _time(g, v0, reps):
    """-> (median ms per iteration, iterations, inner iterations) of gp_lm_graph_optimize from v0"""
    per, s = [], None
    for _ in range(reps):
        g.set_values(v0)
        g.sync()
        t0 = time.perf_counter()
        _, s = g.optimize(max_iterations=30)
        per.append((time.perf_counter() - t0) * 1e3 / max(s["iterations"], 1))
    return float(np.median(per)), s["iterations"], s["inner_iterations"]


def c3(gpa, reps, kernel_only):
    from gtsam_points_amd import synthetic

    g = synthetic.make_c3_graph()
    clouds = [gpa.PointCloudGPU(p, c) for p, c in g["clouds"]]
    maps = []
    for c in clouds:
        m = gpa.GaussianVoxelMapGPU(1.0, target_points_drop_rate=0.0)
        m.insert(c)
        maps.append(m)
    factors = [gpa.IntegratedVGICPFactorGPU(t, s, maps[t], clouds[s]) for t, s in g["pairs"]]
    n = len(g["clouds"])
    truth = _rigid(np.stack(g["stations"][:n]))
    v0 = _rigid(truth @ bench_lm.expmap_many(np.random.default_rng(8191).uniform(-0.1, 0.1, (n, 6))))
    v0[0] = truth[0]
    rng = np.random.default_rng(99)
    sig = np.array([0.01] * 3 + [0.1] * 3)
    pose_factors = [gpa.PriorFactorPose3(0, truth[0], information=1e6 * np.eye(6))]
    for k in range(n - 1):
        Z = _rigid((_inv(truth[k]) @ truth[k + 1] @ _exp(0.2 * sig * rng.normal(size=6)))[None])[0]
        pose_factors.append(gpa.BetweenFactorPose3(k, k + 1, Z, sigmas=sig))
    out = {}
    legs = [("with_pose_factors", dict(fixed=(), pose_factors=pose_factors))]
    if not kernel_only:
        legs = [("vgicp_only", dict(fixed=(0,)))] + legs
    for name, kw in legs:
        lm = gpa.LevenbergMarquardtGraphGPU(factors, g["pairs"], n, **kw)
        one = lm.set_one_launch(True)
        _time(lm, v0, 2)  # warm-up
        ms, it, inner = _time(lm, v0, reps)
        out[name] = dict(ms_per_iteration=round(ms, 4), iterations=it, inner_iterations=inner, one_launch_step=one, factors=len(factors) + len(kw.get("pose_factors", ())))
        lm.close()
    return out


def pgo(gpa, reps, N=1000):
    rng = np.random.default_rng(41)
    truth = [np.eye(4)]
    for k in range(1, N):
        truth.append(truth[-1] @ _exp([0.0, 0.0, 0.05, 1.0, 0.0, 0.0]))
    truth = np.stack(truth)
    sig = np.array([0.01] * 3 + [0.05] * 3)
    factors = [gpa.PriorFactorPose3(0, truth[0], information=1e6 * np.eye(6))]
    for a, b in [(k, k + 1) for k in range(N - 1)] + [(k, k + 20) for k in range(0, N - 20, 25)]:
        factors.append(gpa.BetweenFactorPose3(a, b, _inv(truth[a]) @ truth[b] @ _exp(sig * rng.normal(size=6)), sigmas=sig))
    v0 = _rigid(truth @ bench_lm.expmap_many(rng.normal(scale=[0.02] * 3 + [0.2] * 3, size=(N, 6))))
    lm = gpa.LevenbergMarquardtGraphGPU([], [], N, fixed=(), pose_factors=factors)
    _time(lm, v0, 2)
    ms, it, inner = _time(lm, v0, reps)
    lm.close()
    return dict(poses=N, factors=len(factors), ms_per_iteration=round(ms, 4), iterations=it, inner_iterations=inner)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import gtsam_points_amd as gpa

    gpa.load()
    res = dict(device=torch.cuda.get_device_name(0), reps=args.reps, c3=c3(gpa, args.reps, args.kernel_only))
    if not args.kernel_only:
        res["pgo_1000"] = pgo(gpa, args.reps)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

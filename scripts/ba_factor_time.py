"""Host-to-host time of one bundle-adjustment step on the device: BundleAdjustmentFactorsGPU.linearize_on_device from host values (the values go up through torch,
the record tensor is allocated, two launches, the torch stream and the library stream are each waited for) + SparseLinearSystemGPU.step, and beside it
BundleAdjustmentFactorsGPU.linearize (gp_ba_factors_linearize: values up, two launches, records down, one wait), over a
synthetic set of --features (default 4096) plane and edge features (two planes to one edge) seen from --poses (default 16) poses, each from 2 to 6 of them with 12 to
40 points; pose 0 is held.  --warmup steps (default 10), then --reps (default 100) timed ones at values that move a little every step; min, median and
inter-quartile range of each linearise alone, the solver step alone and linearize_on_device + step.

One JSON object per line; --out <file> writes them there too.  Run under a time limit:

  timeout -k 10 300 python scripts/ba_factor_time.py --out profiles/ba_factor_time.json"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

torch.set_num_threads(16)
import gtsam_points_amd as gpa  # noqa: E402
from gtsam_points_amd import synthetic  # noqa: E402


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


F, P, reps, warmup, out_path = arg("--features", 4096), arg("--poses", 16), arg("--reps", 100), arg("--warmup", 10), arg("--out", "")
assert torch.cuda.is_available(), "ba_factor_time.py measures on the GPU"
rows = []


def emit(**row):
    row["device"] = torch.cuda.get_device_name(0)
    rows.append(row)
    print(json.dumps(row), flush=True)


def stats(ms):
    a = np.asarray(ms)
    q1, q3 = np.percentile(a, [25, 75])
    return dict(reps=len(a), ms_min=round(float(a.min()), 4), ms_median=round(float(np.median(a)), 4), ms_iqr=round(float(q3 - q1), 4))


rng = np.random.default_rng(0)
truth = np.stack([synthetic.expmap(np.array([0.02 * rng.standard_normal(), 0.02 * rng.standard_normal(), 0.05 * k, 0.5 * k, 0.1 * np.sin(k), 0.0])) for k in range(P)])
inv = np.linalg.inv(truth)
factors, total = [], 0
for i in range(F):
    f = gpa.EdgeEVMFactorGPU() if i % 3 == 2 else gpa.PlaneEVMFactorGPU()
    Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    n = int(rng.integers(12, 41))
    seen = rng.choice(P, size=int(rng.integers(2, 7)), replace=False)
    across = (4e-3 * rng.standard_normal(n)) if i % 3 == 2 else rng.uniform(-0.45, 0.45, n)
    w = np.array([0.5 * seen[0], 0.0, 3.0]) + rng.uniform(-2, 2, 3) + np.outer(rng.uniform(-1, 1, n), Q[:, 0]) + np.outer(across, Q[:, 1]) + np.outer(2e-3 * rng.standard_normal(n), Q[:, 2])
    for j in range(n):
        k = int(seen[j % len(seen)])
        f.add(inv[k, :3, :3] @ w[j] + inv[k, :3, 3], k)
    factors.append(f)
    total += n
ba = gpa.BundleAdjustmentFactorsGPU(factors, P)
slot = np.array([-1] + list(range(P - 1)), dtype=np.int32)
system = gpa.SparseLinearSystemGPU(P - 1, ba.factor_slots(slot))
sizes = dict(features=F, poses=P, points=total, records=len(ba))
lin, step, sync = [], [], []
for it in range(warmup + reps):
    values = np.stack([synthetic.expmap(1e-3 * (1.0 + 1e-2 * it) * np.array([1.0, -2.0, 1.5, 3.0, -1.0, 2.0]) * (k % 3)) @ truth[k] for k in range(P)])
    t0 = time.perf_counter()
    rec = ba.linearize_on_device(values)
    t1 = time.perf_counter()
    system.step(rec, lam=1.0)
    t2 = time.perf_counter()
    ba.linearize(values)
    t3 = time.perf_counter()
    if it >= warmup:
        lin.append((t1 - t0) * 1e3)
        step.append((t2 - t1) * 1e3)
        sync.append((t3 - t2) * 1e3)
emit(what="linearize_on_device from host values: torch copy of the values up, record tensor allocated, feature launch + record launch, two waits", **sizes, **stats(lin))
emit(what="linearize (gp_ba_factors_linearize): values up, feature launch + record launch, records down to the host, one wait", **sizes, **stats(sync))
emit(what="SparseLinearSystemGPU.step on the records", **sizes, **stats(step))
emit(what="linearize_on_device + step", **sizes, **stats(np.asarray(lin) + np.asarray(step)))
if out_path:
    with open(out_path, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")

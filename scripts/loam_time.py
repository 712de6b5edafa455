"""Host-to-host time of one synchronous linearise (search + sums + finalize) and of one error evaluation on the stored correspondences (sums + finalize, no search) for
the factors that keep K = 1, 2 and 3 nearest targets per source point -- point-to-point ICP, LOAM point-to-edge, LOAM point-to-plane -- at the fixture size of
tests/test_loam_gpu.py (kitti00_dec8.npz: every second target point as the target, the whole source).  The search's share is the difference of the two.  The calls
alternate between the factors and every linearise is at a new pose; --warmup (default 20) then --reps (default 200), min / median / inter-quartile range.

One JSON object per line; --out <file> writes them there too.  Run under a time limit:

  timeout -k 10 300 python scripts/loam_time.py --out profiles/loam_time.json"""
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
from gtsam_points_amd.synthetic import expmap  # noqa: E402


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


reps, warmup, out_path = arg("--reps", 200), arg("--warmup", 20), arg("--out", "")
assert torch.cuda.is_available(), "loam_time.py measures on the GPU"
d = np.load(os.path.join(ROOT, "tests", "golden", "kitti00_dec8.npz"))
tgt = gpa.PointCloudGPU(np.ascontiguousarray(d["target_points"][0::2]))
src = gpa.PointCloudGPU(d["source_points"])
tree = gpa.KdTreeGPU(tgt)
factors = {1: gpa.IntegratedICPFactorGPU(0, 1, tgt, src, target_tree=tree), 2: gpa.IntegratedPointToEdgeFactorGPU(0, 1, tgt, src, target_tree=tree),
           3: gpa.IntegratedPointToPlaneFactorGPU(0, 1, tgt, src, target_tree=tree)}
rng = np.random.default_rng(3)
lin, err = {k: [] for k in factors}, {k: [] for k in factors}
for it in range(warmup + reps):
    delta = expmap(rng.uniform(-0.02, 0.02, 6))
    near = delta @ expmap(rng.uniform(-0.002, 0.002, 6))
    for k, f in factors.items():
        t = time.perf_counter()
        f.linearize_delta(delta)
        t1 = time.perf_counter()
        f.error({0: np.eye(4), 1: near})
        t2 = time.perf_counter()
        if it >= warmup:
            lin[k].append((t1 - t) * 1e3)
            err[k].append((t2 - t1) * 1e3)
rows = []
for k in factors:
    for what, ms in (("linearise (search + sums + finalize)", lin[k]), ("error on the stored correspondences", err[k])):
        a = np.asarray(ms)
        q1, q3 = np.percentile(a, [25, 75])
        rows.append(dict(K=k, what=what, target_points=tgt.size(), source_points=src.size(), reps=len(a), ms_min=round(float(a.min()), 4), ms_median=round(float(np.median(a)), 4),
                         ms_iqr=round(float(q3 - q1), 4), device=torch.cuda.get_device_name(0)))
        print(json.dumps(rows[-1]), flush=True)
if out_path:
    with open(out_path, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")

"""Host-to-host time of ONE synchronous linearise of IntegratedColoredGICPFactorGPU beside IntegratedGICPFactorGPU's on the same clouds, and of the intensity-gradient
estimate the colored factor needs once per target.

The clouds are the kitti00 pair of tests/golden (7,792 target and 15,576 source points) with their covariances; normals are read off the covariances on the device,
and, the scans carrying no intensity, a smooth synthetic field I = 0.5 + 0.3 sin(0.2 x) cos(0.15 y) + 0.02 z is sampled at both clouds' points: the photometric term
reads the same bytes whatever the values are.  The two factors are called in alternation, every linearise at a new pose (XI scaled by 1 + 1e-3 i), so that each call
searches and no call finds the other's lines warm more than the other does: --warmup calls each (default 20), then --reps (default 200) timed ones, min, median and
inter-quartile range, and the ratio of the medians.  The error evaluation on the stored correspondences is timed the same way.

One JSON object per line; --out <file> writes them there too.  Run under a time limit:

  timeout -k 10 300 python scripts/colored_gicp_time.py --out profiles/colored_gicp_time.json"""
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


reps, warmup, out_path = arg("--reps", 200), arg("--warmup", 20), arg("--out", "")
assert torch.cuda.is_available(), "colored_gicp_time.py measures on the GPU"
rows = []


def emit(**row):
    row["device"] = torch.cuda.get_device_name(0)
    rows.append(row)
    print(json.dumps(row), flush=True)


def stats(ms):
    a = np.asarray(ms)
    q1, q3 = np.percentile(a, [25, 75])
    return dict(reps=len(a), ms_min=round(float(a.min()), 4), ms_median=round(float(np.median(a)), 4), ms_iqr=round(float(q3 - q1), 4))


def field(p):
    p = np.asarray(p, dtype=np.float64)
    return (0.5 + 0.3 * np.sin(0.2 * p[:, 0]) * np.cos(0.15 * p[:, 1]) + 0.02 * p[:, 2]).astype(np.float32)


d = np.load(os.path.join(ROOT, "tests", "golden", "kitti00_dec8.npz"))
tgt = gpa.PointCloudGPU(d["target_points"], d["target_covs"], intensities=field(d["target_points"]))
src = gpa.PointCloudGPU(d["source_points"], d["source_covs"], intensities=field(d["source_points"]))
gpa.estimate_normals_gpu(tgt)  # (read off the covariances)
tree = gpa.KdTreeGPU(tgt)
sizes = dict(target_points=tgt.size(), source_points=src.size())

ms = []
for it in range(warmup + reps):
    t = time.perf_counter()
    grads = gpa.estimate_intensity_gradients_gpu(tgt, 10)
    if it >= warmup:
        ms.append((time.perf_counter() - t) * 1e3)
emit(what="estimate_intensity_gradients_gpu(target, k = 10): grid build + search + kernel", num_short=grads.num_short, **sizes, **stats(ms))

colored = gpa.IntegratedColoredGICPFactorGPU(0, 1, tgt, src, target_tree=tree, target_gradients=grads)
gicp = gpa.IntegratedGICPFactorGPU(0, 1, tgt, src)
XI = np.array([0.01, -0.02, 0.015, 0.10, -0.05, 0.03])
lin = {"colored": [], "gicp": []}
err = {"colored": [], "gicp": []}
for it in range(warmup + reps):
    delta = synthetic.expmap(XI * (1.0 + 1e-3 * it))
    near = delta @ synthetic.expmap(0.1 * XI)
    for name, f in (("colored", colored), ("gicp", gicp)):
        t = time.perf_counter()
        L = f.linearize_delta(delta)
        t1 = time.perf_counter()
        f.error({0: np.eye(4), 1: near})
        t2 = time.perf_counter()
        if it >= warmup:
            lin[name].append((t1 - t) * 1e3)
            err[name].append((t2 - t1) * 1e3)
for name in ("colored", "gicp"):
    emit(what=f"{name}: one synchronous linearise (search + tile kernel + finalize)", **sizes, **stats(lin[name]))
    emit(what=f"{name}: one error evaluation on the stored correspondences", **sizes, **stats(err[name]))
emit(what="ratio of the medians, colored / gicp", linearize=round(float(np.median(lin["colored"]) / np.median(lin["gicp"])), 3),
     error=round(float(np.median(err["colored"]) / np.median(err["gicp"])), 3), bytes_per_matched_point="132 / 100")
if out_path:
    with open(out_path, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")

"""Host-to-host time of ONE synchronous linearise of IntegratedCTICPFactorGPU and IntegratedCTGICPFactorGPU beside IntegratedICPFactorGPU's (point-to-plane) and
IntegratedGICPFactorGPU's on the same clouds.

The clouds are the kitti00 pair of tests/golden (15,584 target and 15,576 source points) with their covariances; normals are read off the covariances on the device.
The scans carry no times: point i of the source is stamped 0.1 * i / n seconds, ring-major as the scan is stored, which the factor groups into 100 bins.  The four
factors are called in alternation, every linearise at new poses (XI scaled by 1 + 1e-3 i; the CT factors between pose0 = I and pose1 = that pose), so that each
call searches and no call finds the other's lines warm more than the other does: --warmup calls each (default 20), then --reps (default 200) timed ones, min,
median and inter-quartile range, and the ratios of the medians.  The error evaluation on the stored correspondences is timed the same way.

One JSON object per line; --out <file> writes them there too.  Run under a time limit:

  timeout -k 10 300 python scripts/ct_factor_time.py --out profiles/ct_factor_time.json"""
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
assert torch.cuda.is_available(), "ct_factor_time.py measures on the GPU"
rows = []


def emit(**row):
    row["device"] = torch.cuda.get_device_name(0)
    rows.append(row)
    print(json.dumps(row), flush=True)


def stats(ms):
    a = np.asarray(ms)
    q1, q3 = np.percentile(a, [25, 75])
    return dict(reps=len(a), ms_min=round(float(a.min()), 4), ms_median=round(float(np.median(a)), 4), ms_iqr=round(float(q3 - q1), 4))


d = np.load(os.path.join(ROOT, "tests", "golden", "kitti00_dec8.npz"))
tgt = gpa.PointCloudGPU(d["target_points"], d["target_covs"])
src = gpa.PointCloudGPU(d["source_points"], d["source_covs"])
gpa.estimate_normals_gpu(tgt)  # (read off the covariances)
src.add_times((0.1 * np.arange(src.size()) / src.size()).astype(np.float32))
tree = gpa.KdTreeGPU(tgt)
factors = {
    "ct_icp": gpa.IntegratedCTICPFactorGPU(0, 1, tgt, src, target_tree=tree),
    "ct_gicp": gpa.IntegratedCTGICPFactorGPU(0, 1, tgt, src, target_tree=tree),
    "icp_plane": gpa.IntegratedPointToPlaneICPFactorGPU(0, 1, tgt, src, target_tree=tree),
    "gicp": gpa.IntegratedGICPFactorGPU(0, 1, tgt, src),
}
sizes = dict(target_points=tgt.size(), source_points=src.size(), time_bins=len(factors["ct_icp"].time_table()[0]))
XI = np.array([0.01, -0.02, 0.015, 0.10, -0.05, 0.03])
lin = {k: [] for k in factors}
err = {k: [] for k in factors}
for it in range(warmup + reps):
    values = {0: np.eye(4), 1: synthetic.expmap(XI * (1.0 + 1e-3 * it))}
    near = {0: np.eye(4), 1: values[1] @ synthetic.expmap(0.1 * XI)}
    for name, f in factors.items():
        t = time.perf_counter()
        f.linearize(values)
        t1 = time.perf_counter()
        f.error(near)
        t2 = time.perf_counter()
        if it >= warmup:
            lin[name].append((t1 - t) * 1e3)
            err[name].append((t2 - t1) * 1e3)
for name in factors:
    emit(what=f"{name}: one synchronous linearise (pose table + search + tile kernel + finalize)" if name.startswith("ct") else
         f"{name}: one synchronous linearise (search + tile kernel + finalize)", **sizes, **stats(lin[name]))
    emit(what=f"{name}: one error evaluation on the stored correspondences", **sizes, **stats(err[name]))
emit(what="ratios of the medians", ct_icp_over_icp_plane=round(float(np.median(lin["ct_icp"]) / np.median(lin["icp_plane"])), 3),
     ct_gicp_over_gicp=round(float(np.median(lin["ct_gicp"]) / np.median(lin["gicp"])), 3))
if out_path:
    with open(out_path, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")

"""Host-to-host time of ONE synchronous linearise of IntegratedColorConsistencyFactorGPU and of IntegratedColoredGICPFactorGPU, each on a KdTreeGPU (3-D
correspondences) and on an IntensityKdTreeGPU (XYZI correspondences), and of the search launch alone, 3-D against 4-D, on the same queries.

The clouds are those of scripts/colored_gicp_time.py: the kitti00 pair of tests/golden (the sizes are in every output row) with their covariances, normals read
off the covariances on the device and the smooth synthetic field I = 0.5 + 0.3 sin(0.2 x) cos(0.15 y) + 0.02 z sampled at both clouds' points.  The four factors
are called in alternation, every linearise at a new pose (XI scaled by 1 + 1e-3 i) so that each call searches: --warmup calls each (default 10), then --reps
(default 31) timed ones; min, median and inter-quartile range.  The search alone is gp_knn_search (k = 1) against gp_intensity_grid_search, both with the 1 m
cut-off of the factors on the source points as queries, launch to end of stream, alternating in the same way; the ratio 4-D / 3-D is that of the medians of this run.

One JSON object per line; --out <file> writes them there too.  Run under a time limit:

  timeout -k 10 300 python scripts/color_consistency_time.py --out profiles/color_consistency_time.json"""
import ctypes as C
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
from gtsam_points_amd import _capi, synthetic  # noqa: E402


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


reps, warmup, out_path = arg("--reps", 31), arg("--warmup", 10), arg("--out", "")
assert torch.cuda.is_available(), "color_consistency_time.py measures on the GPU"
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
trees = {"3d": gpa.KdTreeGPU(tgt), "xyzi": gpa.IntensityKdTreeGPU(tgt)}
grads = gpa.estimate_intensity_gradients_gpu(tgt, 10)
sizes = dict(target_points=tgt.size(), source_points=src.size())

factors = {}
for search, tree in trees.items():
    factors[f"color consistency, {search} tree"] = gpa.IntegratedColorConsistencyFactorGPU(0, 1, tgt, src, target_tree=tree, target_gradients=grads)
    factors[f"colored GICP, {search} tree"] = gpa.IntegratedColoredGICPFactorGPU(0, 1, tgt, src, target_tree=tree, target_gradients=grads)
XI = np.array([0.01, -0.02, 0.015, 0.10, -0.05, 0.03])
lin = {name: [] for name in factors}
inliers = {}
for it in range(warmup + reps):
    delta = synthetic.expmap(XI * (1.0 + 1e-3 * it))
    for name, f in factors.items():
        t = time.perf_counter()
        L = f.linearize_delta(delta)
        if it >= warmup:
            lin[name].append((time.perf_counter() - t) * 1e3)
        inliers[name] = L.num_inliers
for name in factors:
    emit(what=f"{name}: one synchronous linearise (search + tile kernel + finalize)", num_inliers=inliers[name], **sizes, **stats(lin[name]))

# the search launch alone, on the source points as queries
lib = _capi.load()
m = src.size()
q3 = src.points_gpu
q4 = torch.cat([src.points_gpu.to(torch.float64), src.intensities_gpu.to(torch.float64).reshape(-1, 1)], dim=1).contiguous()
idx = torch.empty(m, dtype=torch.int32, device="cuda")
dist = torch.empty(m, dtype=torch.float64, device="cuda")
torch.cuda.synchronize()
ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731


def search_3d():
    _capi.check(lib.gp_knn_search(trees["3d"]._h, ptr(q3), m, 1, 1.0, ptr(idx), ptr(dist), None, None), "gp_knn_search")
    _capi.check(lib.gp_stream_synchronize(None), "sync")


def search_4d():
    _capi.check(lib.gp_intensity_grid_search(trees["xyzi"]._xyzi, ptr(q4), m, 1.0, ptr(idx), ptr(dist), None), "gp_intensity_grid_search")
    _capi.check(lib.gp_stream_synchronize(None), "sync")


ms = {"3d": [], "4d": []}
found = {}
for it in range(warmup + reps):
    for name, call in (("3d", search_3d), ("4d", search_4d)):
        t = time.perf_counter()
        call()
        if it >= warmup:
            ms[name].append((time.perf_counter() - t) * 1e3)
        found[name] = int((idx >= 0).sum())
emit(what="search launch alone, 3-D (gp_knn_search, k = 1, 1 m cut-off)", queries=m, matched=found["3d"], **stats(ms["3d"]))
emit(what="search launch alone, 4-D (gp_intensity_grid_search, 1 m cut-off)", queries=m, matched=found["4d"], **stats(ms["4d"]))
emit(what="ratio of the medians, 4-D search / 3-D search", ratio=round(float(np.median(ms["4d"]) / np.median(ms["3d"])), 3), candidate_bytes="20 / 16")
if out_path:
    with open(out_path, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")

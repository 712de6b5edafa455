"""median host wall time of a KdTreeGPU build on the hashed structure (grid_insert_kernel: the key table's claim) and on the binned one, a k = 1 search on the
hashed structure, a 1 M-point voxelgrid_sampling and an occupancy insert; every call ends in a synchronisation.  One JSON line (profiles/spatial_keying_time.json, leg "keyed").
usage: spatial_keying_time.py [tag]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gtsam_points_amd as gpa  # noqa: E402
from gtsam_points_amd import synthetic
gpa.load()
p = synthetic.make_c2_workload(1_000_000, 64_000, seed=42)["source_points"]
cloud = gpa.PointCloudGPU(p)
def med(f, reps=15):
    f(); f()
    t = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter(); f(); torch.cuda.synchronize(); t.append((time.perf_counter() - t0) * 1e3)
    q = np.percentile(t, [25, 50, 75])
    return {"median_ms": round(float(q[1]), 4), "iqr_ms": round(float(q[2] - q[0]), 4)}
out = {"tag": sys.argv[1] if len(sys.argv) > 1 else ""}
out["hashed_grid_build_1M"] = med(lambda: gpa.KdTreeGPU(cloud, cell_size=0.5, structure=1))
out["binned_grid_build_1M"] = med(lambda: gpa.KdTreeGPU(cloud, cell_size=0.5, structure=0))
tree = gpa.KdTreeGPU(cloud, cell_size=0.5, structure=1)
q = p[:200_000]
out["hashed_knn_search_k1_200k"] = med(lambda: tree.knn_search(q, 1))
f = gpa.PointCloudGPU(device="cuda:0"); f.add_points(p)
out["voxelgrid_sampling_1M"] = med(lambda: gpa.voxelgrid_sampling_gpu(f, 0.5))
out["occupancy_insert_1M"] = med(lambda: gpa.OccupancyGridGPU(0.5).insert(cloud))
print(json.dumps(out))

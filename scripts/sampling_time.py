"""Cost of voxelgrid_sampling_gpu (points + covariances + intensities) on the 2 M-point C2 target cloud at 0.5 m, next to merge_frames_gpu of that single frame at the
identity pose in the same process -- the only other device route to the same three outputs (the same binning plus a transform).

  voxelgrid_sampling   voxelgrid_sampling_gpu(frame, 0.5)                       host wall per call
  merge_frames         merge_frames_gpu([I], [frame], 0.5)                      host wall per call
  plan_build           gp_voxelgrid_plan_create + destroy                       host wall per call (the build waits once)
  average_<attr>       gp_voxelgrid_plan_average on a built plan                HIP events around 20 back-to-back launches, per launch
  randomgrid_sampling  randomgrid_sampling_gpu(frame, 0.5, 0.1)                 host wall per call

Median of 9 warm runs each, the two whole calls alternating.  One JSON object on stdout, written to --out <file> as well when given."""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
torch.set_num_threads(16)
import gtsam_points_amd as gpa
from gtsam_points_amd import synthetic

REPS, EVENT_REPS, RES = 9, 20, 0.5
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
n_target = int(sys.argv[sys.argv.index("--points") + 1]) if "--points" in sys.argv else 2_000_000

d = synthetic.make_c2_workload(64_000, n_target, seed=42)
rng = np.random.default_rng(0)
frame = gpa.PointCloudGPU(d["target_points"], d["target_covs"], intensities=rng.uniform(0, 255, size=n_target).astype(np.float32))
I = np.eye(4)


def wall(call):
    torch.cuda.synchronize()
    t = time.perf_counter()
    call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


calls = {"voxelgrid_sampling": lambda: gpa.voxelgrid_sampling_gpu(frame, RES), "merge_frames": lambda: gpa.merge_frames_gpu([I], [frame], RES, target_points_drop_rate=0.0)}
for c in calls.values():
    for _ in range(3):
        c()
ms = {k: [] for k in calls}
for rep in range(REPS):
    for k, c in calls.items():  # alternating
        ms[k].append(wall(c))
row = dict(cloud="c2_target", points=int(frame.size()), resolution=RES, reps=REPS, device=torch.cuda.get_device_name(0))
row["num_voxels"] = int(gpa.voxelgrid_sampling_gpu(frame, RES).size())
row["merge_frames_voxels"] = int(gpa.merge_frames_gpu([I], [frame], RES, target_points_drop_rate=0.0).size())
for k in calls:
    row[k + "_ms_median"], row[k + "_ms_min"] = round(float(np.median(ms[k])), 4), round(float(np.min(ms[k])), 4)
row["ratio_voxelgrid_over_merge"] = round(row["voxelgrid_sampling_ms_median"] / row["merge_frames_ms_median"], 3)


def build():
    gpa.VoxelGridPlan(frame, RES).close()


for _ in range(3):
    build()
t = [wall(build) for _ in range(REPS)]
row["plan_build_ms_median"], row["plan_build_ms_min"] = round(float(np.median(t)), 4), round(float(np.min(t)), 4)
plan = gpa.VoxelGridPlan(frame, RES)
for name, tensor in (("points", frame.points_gpu), ("covs", frame.covs_gpu), ("intensities", frame.intensities_gpu)):
    for _ in range(3):
        plan.average(tensor)
    us = []
    outs = [torch.empty((plan.num_voxels, tensor.shape[1]), dtype=torch.float32, device=tensor.device)]
    import ctypes as C
    from gtsam_points_amd import _capi
    launch = lambda: _capi.check(plan._lib.gp_voxelgrid_plan_average(plan._h, C.c_void_p(tensor.data_ptr()), int(tensor.shape[1]), C.c_void_p(outs[0].data_ptr())), "average")
    for rep in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(EVENT_REPS):
            launch()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / EVENT_REPS)
    row[f"average_{name}_us_median"], row[f"average_{name}_us_min"] = round(float(np.median(us)), 2), round(float(np.min(us)), 2)
plan.close()
rg = lambda: gpa.randomgrid_sampling_gpu(frame, RES, 0.1, seed=1)
for _ in range(3):
    rg()
t = [wall(rg) for _ in range(REPS)]
row["randomgrid_sampling_ms_median"], row["randomgrid_sampling_ms_min"] = round(float(np.median(t)), 4), round(float(np.min(t)), 4)
line = json.dumps(row)
print(line, flush=True)
if out_path:
    with open(out_path, "w") as f:
        f.write(json.dumps(row, indent=1) + "\n")

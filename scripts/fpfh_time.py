"""Host wall time (every call ends in a synchronisation) of estimate_fpfh_gpu on the two golden scans scripts/ransac_time.py uses, prepared on the device as a
registration front end would: voxelgrid_sampling_gpu at 0.5 m, estimate_normals_gpu at k = 10.

  clouds  tests/golden/kitti_00/000000.bin (target) and 000001.bin (source), downsampled; both are timed
  calls   search_radius 5.0 (the reference's default), 2.5 and 1.0, max_num_neighbors at its default; float32 output for every point
  phases  the stream time of the grid build (insert, sort, gather; it contains the sort's host wait), of the SPFH pass and of the FPFH pass, taken with events by the
          library itself (gp_debug_fpfh_phase_times) inside the same calls; mean and maximum neighbour count of each cloud and radius

Every call is warmed up; the calls then ALTERNATE for --reps rounds (default 31): median, minimum, inter-quartile range and range of each.  There is no CPU figure
beside these: the reference's FPFH is not among the sources oracle/ compiles.  Writes one JSON document to --out (default profiles/fpfh_time.json).  Run it under a
time limit:

  timeout -k 10 600 python scripts/fpfh_time.py"""
import ctypes as C
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
torch.set_num_threads(16)
import gtsam_points_amd as gpa

reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 31
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "fpfh_time.json")
assert torch.cuda.is_available(), "fpfh_time.py measures on the GPU"
assert reps >= 20
lib = gpa.load()


def cloud(name):
    raw = gpa.PointCloudGPU(np.fromfile(os.path.join(ROOT, "tests", "golden", "kitti_00", name), dtype=np.float32).reshape(-1, 3))
    down = gpa.voxelgrid_sampling_gpu(raw, 0.5)
    gpa.estimate_normals_gpu(down, 10)
    return raw.size(), down


clouds = {"target": cloud("000000.bin"), "source": cloud("000001.bin")}
radii = (5.0, 2.5, 1.0)
calls, phases, neighbours = [], {}, {}
for cname, (_, frame) in clouds.items():
    for r in radii:
        what = f"{cname}_r{r}"
        _, _, num, cut = gpa.estimate_fpfh_gpu(frame, gpa.FPFHEstimationParams(r), return_spfh=True)
        neighbours[what] = dict(mean=round(float(num.double().mean()), 2), max=int(num.max()), num_truncated=int(cut))
        phases[what] = []

        def call(frame=frame, r=r, what=what):
            gpa.estimate_fpfh_gpu(frame, gpa.FPFHEstimationParams(r))
            ms = (C.c_double * 3)()
            lib.gp_debug_fpfh_phase_times(1, ms)
            phases[what].append(list(ms))

        calls.append((what, call))
lib.gp_debug_fpfh_phase_times(1, None)
for what, call in calls:
    for _ in range(3):
        call()
    phases[what].clear()
ts = {what: [] for what, _ in calls}
for _ in range(reps):
    for what, call in calls:
        t = time.perf_counter()
        call()
        ts[what].append((time.perf_counter() - t) * 1e3)
lib.gp_debug_fpfh_phase_times(0, None)
rows = []
for what, _ in calls:
    a, ph = np.asarray(ts[what]), np.asarray(phases[what])
    q1, q3 = np.percentile(a, [25, 75])
    med = np.median(ph, axis=0)
    rows.append(dict(call=what, points=clouds[what.split("_")[0]][1].size(), search_radius=float(what.split("_r")[1]), reps=reps, ms_median=round(float(np.median(a)), 4),
                     ms_min=round(float(a.min()), 4), ms_iqr=round(float(q3 - q1), 4), ms_range=round(float(a.max() - a.min()), 4), ms_grid_build_median=round(float(med[0]), 4),
                     ms_spfh_pass_median=round(float(med[1]), 4), ms_fpfh_pass_median=round(float(med[2]), 4), neighbours=neighbours[what]))
    print(json.dumps(rows[-1]), flush=True)
props = torch.cuda.get_device_properties(0)
doc = dict(device=torch.cuda.get_device_name(0), arch=props.gcnArchName.split(":")[0], compute_units=props.multi_processor_count,
           what="host wall time per estimate_fpfh_gpu call in ms (float32 rows for every point), each call ending in a synchronisation; calls alternate within a round; "
                "the three phase figures are stream times between events inside the same calls",
           voxel_resolution=0.5, k_normals=10, max_num_neighbors=10000, raw_points={k: v[0] for k, v in clouds.items()},
           cpu_reference="none: the reference's fpfh_estimation.cpp is not among the sources oracle/ compiles", rows=rows)
with open(out_path, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")

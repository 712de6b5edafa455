"""Host wall time of ONE incremental insert into a steady-state sliding map (IncrementalGaussianVoxelMapGPU, lru_horizon 10, lru_clear_cycle 1) next to what the library
offered for the same map before: a one-shot GaussianVoxelMapGPU.insert of the concatenation of the frames still inside the horizon.

The sequence is the full scan tests/golden/kitti_00/000000.bin (about 1.2e5 points) moved 1 m per frame along x -- a vehicle's sliding local map -- at leaf 1.0 with a
constant isotropic covariance (the time does not depend on the covariances' values).  The map takes frames 0 .. 19, so that it is in its steady state and evicts at every
insert; the timed call is the insert of frame 20, after which the map holds the voxels that frames 11 .. 20 touched (stamp + 10 >= 21).  Each timed insert needs the same map, so each round clones the steady map first (not timed) and
inserts into the clone.  The one-shot build gets the ten frames 11 .. 20 already concatenated on the device (the copy is not timed either).  Both calls return when
the device has finished.  The calls alternate for --reps rounds (default 31): median, minimum, inter-quartile range and range of each.  A median over some tens of
calls on a shared machine shows a difference of tens of per cent, not of a few.  The two maps must hold the same voxels, which is checked (the incremental map's voxels also keep the points that earlier
frames gave them: upstream's semantics, which a rebuild from the window cannot give).
Writes one JSON document to --out (default profiles/incremental_map_time.json).  Run it under a time limit:

  timeout -k 10 600 python scripts/incremental_map_time.py"""
import ctypes as C, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
torch.set_num_threads(16)
import gtsam_points_amd as gpa
from gtsam_points_amd import _capi

reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 31
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "incremental_map_time.json")
assert torch.cuda.is_available(), "incremental_map_time.py measures on the GPU"
assert reps >= 20
lib = gpa.load()
LEAF, HORIZON, STEP, WARM = 1.0, 10, 1.0, 20

scan = np.fromfile(os.path.join(ROOT, "tests", "golden", "kitti_00", "000000.bin"), dtype=np.float32).reshape(-1, 3)
n = len(scan)
cov = np.tile((np.eye(3, dtype=np.float32) * np.float32(0.01)).reshape(1, 9), (n, 1))


def frame(k):
    return gpa.PointCloudGPU(scan + np.array([STEP * k, 0.0, 0.0], dtype=np.float32), cov.reshape(n, 3, 3))


frames = [frame(k) for k in range(WARM + 1)]
steady = gpa.IncrementalGaussianVoxelMapGPU(LEAF, lru_horizon=HORIZON, lru_clear_cycle=1)
for f in frames[:WARM]:
    steady.insert(f)
window = frames[WARM - HORIZON + 1 :]  # stamps WARM - HORIZON + 1 .. WARM survive the insert of frame WARM
concat = gpa.PointCloudGPU.from_device(torch.cat([f.points_gpu for f in window]).contiguous(), torch.cat([f.covs_gpu for f in window]).contiguous())
torch.cuda.synchronize()


def clone():
    h = C.c_void_p()
    _capi.check(lib.gp_voxelmap_clone_to_device(steady._h, 0, None, C.byref(h)), "gp_voxelmap_clone_to_device")
    return gpa.IncrementalGaussianVoxelMapGPU(LEAF, _handle=h)


def incremental(vm):
    vm.insert(frames[WARM])


def one_shot(vm):
    vm.insert(concat)


def fresh():
    return gpa.GaussianVoxelMapGPU(LEAF, target_points_drop_rate=0.0)


calls = [("incremental_insert", clone, incremental), ("one_shot_insert_of_the_window", fresh, one_shot)]
last = {}
for what, make, call in calls:
    for _ in range(5):
        vm = make()
        call(vm)
    last[what] = vm
ci = last["incremental_insert"].download_f64()[0]
co = last["one_shot_insert_of_the_window"].download_f64()[0]
assert ci.tobytes() == co.tobytes(), "the incremental map and the one-shot map of the window hold different voxels"
ts = {what: [] for what, _, _ in calls}
for _ in range(reps):
    for what, make, call in calls:
        vm = make()
        t = time.perf_counter()
        call(vm)
        ts[what].append((time.perf_counter() - t) * 1e3)
        del vm
rows = []
for what, _, _ in calls:
    a = np.asarray(ts[what])
    q1, q3 = np.percentile(a, [25, 75])
    rows.append(dict(call=what, frame_points=n, window_frames=len(window), window_points=concat.size(), voxels=int(len(ci)), leaf=LEAF, lru_horizon=HORIZON, reps=reps,
                     ms_median=round(float(np.median(a)), 4), ms_min=round(float(a.min()), 4), ms_iqr=round(float(q3 - q1), 4), ms_range=round(float(a.max() - a.min()), 4)))
    print(json.dumps(rows[-1]), flush=True)

props = torch.cuda.get_device_properties(0)  # (the name torch reports can be a generic one: the gfx target and the CU count place the figures)
doc = dict(device=torch.cuda.get_device_name(0), arch=props.gcnArchName.split(":")[0], compute_units=props.multi_processor_count,
           what="host wall time per call in ms, each call returning when the device has finished; calls alternate within a round", rows=rows)
with open(out_path, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")

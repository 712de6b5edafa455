"""Host wall time (every call ends in a synchronisation) of estimate_pose_ransac_gpu on the two golden scans at 5000 iterations, and of its two heavy kernels alone:

  target  tests/golden/kitti_00/000000.bin, source 000001.bin (full scans); D = 33 synthetic descriptors: a source row is the row of the nearest target point plus
          noise for ~60 % of the points, random otherwise (synthetic, so that the share of good matches is known; real ones come from estimate_fpfh_gpu)
  calls   ransac_5000            RANSACParams() as they are: 5000 iterations in chunks of 1024, early stop at 0.8 of the source
          ransac_5000_no_stop    early_stop_inlier_rate = 2: no chunk is skipped, all 5000 hypotheses are tried
          overlap_batch_1024     OccupancyGridGPU.calc_overlap_batch alone: the source cloud at 1024 poses (one chunk's scoring launch when every hypothesis survives)
          match_3072             match_features_gpu alone: 3072 sampled rows among the target's rows (one chunk's matching launch)
          grid_insert            OccupancyGridGPU(1.0).insert(target): what every RANSAC call builds first

Every call is warmed up; the calls then ALTERNATE for --reps rounds (default 31), so that the machine's noise is every call's noise: median, minimum, inter-quartile
range and range of each.  A median over some tens of calls on a shared machine shows a difference of tens of per cent, not of a few.  Writes one JSON document to
--out (default profiles/ransac_time.json).  Run it under a time limit:

  timeout -k 10 600 python scripts/ransac_time.py"""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
torch.set_num_threads(16)
import gtsam_points_amd as gpa

reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 31
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "ransac_time.json")
assert torch.cuda.is_available(), "ransac_time.py measures on the GPU"
assert reps >= 20
D = 33


def scan(name):
    return np.fromfile(os.path.join(ROOT, "tests", "golden", "kitti_00", name), dtype=np.float32).reshape(-1, 3)


rng = np.random.default_rng(3)
target_pts, source_pts = scan("000000.bin"), scan("000001.bin")
target, source = gpa.PointCloudGPU(target_pts), gpa.PointCloudGPU(source_pts)
# the nearest target point of every source point (the scans are 0.1 s apart: nearly aligned), through the library's own exact search
tree = gpa.KdTreeGPU(target)
nn = torch.empty((len(source_pts), 1), dtype=torch.int32, device=target.device)
sq = torch.empty((len(source_pts), 1), dtype=torch.float64, device=target.device)
import ctypes as C
gpa._capi.check(gpa.load().gp_knn_search(tree._h, source.ptr(source.points_gpu), len(source_pts), 1, float(np.finfo(np.float64).max), C.c_void_p(nn.data_ptr()), C.c_void_p(sq.data_ptr()),
                                         None, None), "gp_knn_search")
gpa._capi.check(gpa.load().gp_stream_synchronize(None), "sync")
nn = nn.cpu().numpy().reshape(-1)
tf = rng.normal(size=(len(target_pts), D)).astype(np.float32)
sf = rng.normal(size=(len(source_pts), D)).astype(np.float32)
good = (rng.random(len(source_pts)) < 0.6) & (nn >= 0)
sf[good] = tf[nn[good]] + (0.01 * rng.normal(size=(int(good.sum()), D))).astype(np.float32)
tf_d, sf_d = torch.from_numpy(tf).cuda(), torch.from_numpy(sf).cuda()
del tree

grid = gpa.OccupancyGridGPU(1.0).insert(target)
poses = np.stack([np.eye(4)] * 1024)
for k in range(1024):  # poses around the identity: most points fall into occupied blocks, as for RANSAC's surviving hypotheses
    a = 0.002 * k
    poses[k, :2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    poses[k, :3, 3] = [0.01 * k, -0.005 * k, 0.0]
poses_d = torch.from_numpy(np.ascontiguousarray(poses.transpose(0, 2, 1)).reshape(-1, 16)).cuda()
rows_d = torch.from_numpy(rng.integers(0, len(source_pts), size=3072).astype(np.int32)).cuda()
results = {}


def ransac(rate):
    def call():
        r = gpa.estimate_pose_ransac_gpu(target, source, tf_d, sf_d, gpa.RANSACParams(early_stop_inlier_rate=rate))
        results[rate] = r
    return call


calls = [("ransac_5000", ransac(0.8)), ("ransac_5000_no_stop", ransac(2.0)), ("overlap_batch_1024", lambda: grid.calc_overlap_batch(source, poses_d)),
         ("match_3072", lambda: gpa.match_features_gpu(tf_d, sf_d, rows_d)), ("grid_insert", lambda: gpa.OccupancyGridGPU(1.0).insert(target).close())]
for what, call in calls:
    for _ in range(3):
        call()
ts = {what: [] for what, _ in calls}
for _ in range(reps):
    for what, call in calls:
        t = time.perf_counter()
        call()
        ts[what].append((time.perf_counter() - t) * 1e3)
rows = []
for what, _ in calls:
    a = np.asarray(ts[what])
    q1, q3 = np.percentile(a, [25, 75])
    rows.append(dict(call=what, reps=reps, ms_median=round(float(np.median(a)), 4), ms_min=round(float(a.min()), 4), ms_iqr=round(float(q3 - q1), 4), ms_range=round(float(a.max() - a.min()), 4)))
    print(json.dumps(rows[-1]), flush=True)
slots, blocks = grid.table_info()
props = torch.cuda.get_device_properties(0)
doc = dict(device=torch.cuda.get_device_name(0), arch=props.gcnArchName.split(":")[0], compute_units=props.multi_processor_count,
           what="host wall time per call in ms, each call ending in a synchronisation; calls alternate within a round", target_points=len(target_pts), source_points=len(source_pts),
           dim=D, iterations=5000, chunk_iterations=1024, table_slots=slots, table_blocks=blocks, table_bytes=slots * 72, occupied_cells=grid.num_occupied_cells(),
           results={("default" if r == 0.8 else "no_stop"): dict(inlier_rate=v.inlier_rate, best_iteration=v.best_iteration, best_inliers=v.best_inliers, num_scored=v.num_scored,
                                                                early_stopped=v.early_stopped) for r, v in results.items()},
           rows=rows)
with open(out_path, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")

"""Host wall time (every step ends in a synchronisation) of remove_outliers_gpu(k = 10, std_thresh = 1) with a prebuilt KdTreeGPU, split into its steps, next to the
composition the library offered before the fused kernel existed -- gp_knn_search into device int[n][10] / double[n][10] arrays, then
gp_cloud_mean_neighbor_distances_from on the lists:

  c2         the 1 M-point synthetic.make_c2_workload(1_000_000, 64_000, seed=42)["source_points"] cloud
  kitti_00   the two full scans tests/golden/kitti_00/000000.bin and 000001.bin

Steps timed on their own: fused (gp_cloud_mean_neighbor_distances), search + from (the two-pass form, and each half), threshold (gp_cloud_inlier_threshold), compaction
(gp_cloud_select_below), gather (gp_cloud_gather of every attribute the cloud holds: points only here), and the whole remove_outliers_gpu call.  Every call is warmed up;
the calls then ALTERNATE for --reps rounds (default 31), so that the machine's noise is every call's noise: median, minimum, inter-quartile range and range of each.
A median over some tens of calls on a shared machine shows a difference of tens of per cent, not of a few.  The two forms must agree to the bit, which is checked.
Writes one JSON document to --out (default profiles/outliers_time.json).  Run it under a time limit:

  timeout -k 10 600 python scripts/outliers_time.py"""
import ctypes as C, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
torch.set_num_threads(16)
import gtsam_points_amd as gpa
from gtsam_points_amd import _capi, synthetic
from gtsam_points_amd.sampling import _gather_rows

reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 31
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "outliers_time.json")
assert torch.cuda.is_available(), "outliers_time.py measures on the GPU"
assert reps >= 20
lib = gpa.load()
K, STD = 10, 1.0
DBL_MAX = float(np.finfo(np.float64).max)


def clouds():
    yield "c2", synthetic.make_c2_workload(1_000_000, 64_000, seed=42)["source_points"]
    for name in ("000000.bin", "000001.bin"):
        yield "kitti_00/" + name, np.fromfile(os.path.join(ROOT, "tests", "golden", "kitti_00", name), dtype=np.float32).reshape(-1, 3)


def ptr(t):
    return C.c_void_p(t.data_ptr())


rows = []
for name, pts in clouds():
    n = len(pts)
    frame = gpa.PointCloudGPU(pts)
    tree = gpa.KdTreeGPU(frame, cell_size=0.25)
    dev = frame.device
    d_fused = torch.empty(n, dtype=torch.float64, device=dev)
    d_from = torch.empty(n, dtype=torch.float64, device=dev)
    nb = torch.empty((n, K), dtype=torch.int32, device=dev)
    sq = torch.empty((n, K), dtype=torch.float64, device=dev)
    idx = torch.empty(n, dtype=torch.int32, device=dev)
    stats = (C.c_double * 4)()
    kept = C.c_int(0)
    torch.cuda.synchronize()

    def sync():
        _capi.check(lib.gp_stream_synchronize(None), "sync")

    def fused():
        _capi.check(lib.gp_cloud_mean_neighbor_distances(tree._h, frame.ptr(frame.points_gpu), n, K, ptr(d_fused), None, None), "fused")
        sync()

    def search():
        _capi.check(lib.gp_knn_search(tree._h, frame.ptr(frame.points_gpu), n, K, DBL_MAX, ptr(nb), ptr(sq), None, None), "gp_knn_search")
        sync()

    def from_lists():
        _capi.check(lib.gp_cloud_mean_neighbor_distances_from(frame.ptr(frame.points_gpu), n, ptr(nb), K, ptr(d_from), None, None), "from")
        sync()

    def two_pass():
        _capi.check(lib.gp_knn_search(tree._h, frame.ptr(frame.points_gpu), n, K, DBL_MAX, ptr(nb), ptr(sq), None, None), "gp_knn_search")
        _capi.check(lib.gp_cloud_mean_neighbor_distances_from(frame.ptr(frame.points_gpu), n, ptr(nb), K, ptr(d_from), None, None), "from")
        sync()

    def threshold():
        _capi.check(lib.gp_cloud_inlier_threshold(ptr(d_fused), n, STD, stats, None), "threshold")

    def compaction():
        _capi.check(lib.gp_cloud_select_below(ptr(d_fused), n, stats[2], ptr(idx), C.byref(kept), None), "select_below")

    def gather():
        _gather_rows(frame, idx[: kept.value])

    def whole():
        return gpa.remove_outliers_gpu(frame, k=K, std_thresh=STD, tree=tree)

    calls = [("fused_mean_distances", fused), ("two_pass_mean_distances", two_pass), ("two_pass_search", search), ("two_pass_from_lists", from_lists), ("threshold", threshold),
             ("compaction", compaction), ("gather", gather), ("remove_outliers_gpu", whole)]
    for what, call in calls:
        for _ in range(5):
            r = call()
    assert d_fused.cpu().numpy().tobytes() == d_from.cpu().numpy().tobytes(), "the fused kernel and the two-pass form disagree"
    assert r.size() == kept.value and r.dist_thresh == stats[2]
    ts = {what: [] for what, _ in calls}
    for _ in range(reps):
        for what, call in calls:
            t = time.perf_counter()
            call()
            ts[what].append((time.perf_counter() - t) * 1e3)
    for what, _ in calls:
        a = np.asarray(ts[what])
        q1, q3 = np.percentile(a, [25, 75])
        rows.append(dict(cloud=name, points=n, k=K, std_thresh=STD, kept=kept.value, call=what, reps=reps, ms_median=round(float(np.median(a)), 4), ms_min=round(float(a.min()), 4),
                         ms_iqr=round(float(q3 - q1), 4), ms_range=round(float(a.max() - a.min()), 4)))
        print(json.dumps(rows[-1]), flush=True)
    del tree

props = torch.cuda.get_device_properties(0)  # (the name torch reports can be a generic one: the gfx target and the CU count place the figures)
doc = dict(device=torch.cuda.get_device_name(0), arch=props.gcnArchName.split(":")[0], compute_units=props.multi_processor_count, what="host wall time per call in ms, each call ending in a synchronisation; calls alternate within a round",
           list_bytes_per_point=12 * K, fused_bytes_per_point=8, rows=rows)
with open(out_path, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")

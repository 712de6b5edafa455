"""Host wall time of one synchronous linearise of the ICP factor (point-to-point and point-to-plane) next to the GICP factor's, on the same clouds, poses and cut-off
(1 m), and of the correspondence search alone (gp_knn_search, k = 1, on the transformed source points with the outputs allocated beforehand):

  kitti_00   the two full scans tests/golden/kitti_00/000000.bin (target) and 000001.bin (source), delta = Expmap(C1B_PERTURBATION)
  c5         the 1 M-point synthetic pair of BASELINE configs[4] (synthetic.make_c2_workload(1_000_000, 1_000_000, seed=42)), delta as bench_detail.py's C5 leg

Covariances and normals come from estimate_normals_covariances_gpu (k = 10).  Every factor is warmed up, then the four calls ALTERNATE for --reps rounds (default 31): median,
minimum and the spread (inter-quartile range and max - min) of each.  The yardstick is the GICP linearise of the same run: the ICP factor runs the same search and reads
28-40 B per matched point where GICP reads 96 B.  One JSON object per line; --out <file> appends them there too.  Run it under a time limit:

  timeout -k 10 900 python scripts/icp_time.py --out profiles/corr_factors_time.jsonl"""
import ctypes as C, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
torch.set_num_threads(16)
import gtsam_points_amd as gpa
from gtsam_points_amd import _capi, synthetic
from gtsam_points_amd.types import _pose16

reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 31
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
assert torch.cuda.is_available(), "icp_time.py measures on the GPU"
lib = gpa.load()


def emit(**row):
    line = json.dumps(row)
    print(line, flush=True)
    if out_path:
        with open(out_path, "a") as f:
            f.write(line + "\n")


def pairs():
    if only in (None, "kitti_00"):
        k = os.path.join(ROOT, "tests", "golden", "kitti_00")
        yield "kitti_00", np.fromfile(os.path.join(k, "000000.bin"), dtype=np.float32).reshape(-1, 3), np.fromfile(os.path.join(k, "000001.bin"), dtype=np.float32).reshape(-1, 3), \
            synthetic.expmap(synthetic.C1B_PERTURBATION)
    if only in (None, "c5"):
        d = synthetic.make_c2_workload(1_000_000, 1_000_000, seed=42)
        yield "c5", d["target_points"], d["source_points"], d["T_true"] @ synthetic.expmap([2e-4, -1e-4, 1.5e-4, 0.02, -0.01, 0.015])


for name, tp, sp, delta in pairs():
    tgt, src = gpa.PointCloudGPU(tp), gpa.PointCloudGPU(sp)
    gpa.estimate_normals_covariances_gpu(tgt, 10)
    gpa.estimate_covariances_gpu(src, 10)
    tree = gpa.KdTreeGPU(tgt, cell_size=0.25)  # the cell the GICP factor's own structure uses at a 1 m cut-off
    gicp = gpa.IntegratedGICPFactorGPU(0, 1, tgt, src)
    point = gpa.IntegratedICPFactorGPU(0, 1, tgt, src, target_tree=tree)
    plane = gpa.IntegratedPointToPlaneICPFactorGPU(0, 1, tgt, src, target_tree=tree)
    q = torch.from_numpy((sp.astype(np.float64) @ delta[:3, :3].T + delta[:3, 3]).astype(np.float32)).to(src.device)
    idx = torch.empty(len(sp), dtype=torch.int32, device=src.device)
    torch.cuda.synchronize()

    def search():
        _capi.check(lib.gp_knn_search(tree._h, C.c_void_p(q.data_ptr()), len(sp), 1, 1.0, C.c_void_p(idx.data_ptr()), None, None, None), "gp_knn_search")
        _capi.check(lib.gp_stream_synchronize(None), "sync")

    calls = [("gicp", lambda: gicp.linearize_delta(delta)), ("icp_point", lambda: point.linearize_delta(delta)), ("icp_plane", lambda: plane.linearize_delta(delta)),
             ("search_only", search)]
    inliers = {}
    for what, call in calls:
        for _ in range(5):
            r = call()
        inliers[what] = getattr(r, "num_inliers", int((idx >= 0).sum().item()))
    ts = {what: [] for what, _ in calls}
    for _ in range(reps):
        for what, call in calls:  # alternating: one call's noise is every call's noise
            t = time.perf_counter()
            call()
            ts[what].append((time.perf_counter() - t) * 1e3)
    for what, _ in calls:
        a = np.asarray(ts[what])
        q1, q3 = np.percentile(a, [25, 75])
        emit(cloud=name, call=what, source_points=len(sp), target_points=len(tp), inliers=inliers[what], reps=reps, ms_median=round(float(np.median(a)), 4), ms_min=round(float(a.min()), 4),
             ms_iqr=round(float(q3 - q1), 4), ms_range=round(float(a.max() - a.min()), 4))
    del gicp, point, plane, tree

"""Cost of the normal estimation next to gp_estimate_covariances (k = 10), with a given build of the library (--lib <file under gtsam_points_amd/>), on the three clouds
of profiles/r05_c5_ab.jsonl: the C5 config cloud (the 1 M-point C2 source), the denser map-like target sampling of the same scene, and a real kitti_00 scan.

  covariances   estimate_covariances_gpu                       host wall per call, median of 9 (alternating over the clouds, as bench.py does)
  fused         estimate_normals_covariances_gpu               the same
  normals_only  estimate_normals_gpu on a frame without covs   the same
  from_covs     gp_estimate_normals_from_covs                  HIP events around 50 back-to-back launches, per launch

--covariances-only: for a build that has no normal estimation (the parent commit's library in an A/B): the first row only.  A SHA-256 of every output array, so that
two builds can be held against each other bit for bit.  One JSON object per line on stdout, appended to --out <file> as well when given."""
import ctypes as C, hashlib, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
torch.set_num_threads(16)
from gtsam_points_amd import _capi
lib_name = sys.argv[sys.argv.index("--lib") + 1] if "--lib" in sys.argv else "libgtsam_points_hip.so"
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
cov_only = "--covariances-only" in sys.argv
_capi.LIB_PATH = os.path.join(ROOT, "gtsam_points_amd", lib_name)
if cov_only:  # (the binding table resolves every symbol at load)
    for name in ("gp_estimate_normals_from_covs", "gp_estimate_normals_covariances"):
        _capi._SIGNATURES.pop(name, None)
import gtsam_points_amd as gpa
from gtsam_points_amd import synthetic

REPS, EVENT_REPS = 9, 50
sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def emit(**row):
    line = json.dumps(dict(lib=lib_name, **row))
    print(line, flush=True)
    if out_path:
        with open(out_path, "a") as f:
            f.write(line + "\n")


d = synthetic.make_c2_workload(1_000_000, 1_000_000, seed=42)
kitti = os.path.join(ROOT, "tests", "golden", "kitti_00", "000000.bin")
clouds = [("c5_source", d["source_points"]), ("c5_target", d["target_points"])]
if os.path.exists(kitti):
    clouds.append(("kitti_00", np.fromfile(kitti, dtype=np.float32).reshape(-1, 3)))


def normals_only(fr):
    fr.covs_gpu = None  # (estimate_normals_gpu reads normals off covariances when the frame has them)
    return gpa.estimate_normals_gpu(fr, 10)


calls = [("covariances", lambda fr: gpa.estimate_covariances_gpu(fr, 10), ("covs",))]
if not cov_only:
    calls += [("fused", lambda fr: gpa.estimate_normals_covariances_gpu(fr, 10), ("covs", "normals")), ("normals_only", normals_only, ("normals",))]
for what, call, outputs in calls:
    frames = [(name, gpa.PointCloudGPU(p)) for name, p in clouds]
    for name, fr in frames:
        for _ in range(3):
            call(fr)
    ts = {name: [] for name, _ in frames}
    for rep in range(REPS):
        for name, fr in frames:  # alternating: neither call finds the other's scratch arrays waiting
            torch.cuda.synchronize()
            t = time.perf_counter()
            call(fr)
            ts[name].append(time.perf_counter() - t)
    for name, fr in frames:
        emit(call=what, cloud=name, points=int(fr.size()), ms_median=round(float(np.median(ts[name])) * 1e3, 4), ms_min=round(float(np.min(ts[name])) * 1e3, 4),
             **{"sha256_" + o: sha(fr.download(o)) for o in outputs})
if not cov_only:
    lib = gpa.load()
    for name, p in clouds:
        fr = gpa.PointCloudGPU(p)
        gpa.estimate_covariances_gpu(fr, 10)
        normals = torch.empty((fr.size(), 3), dtype=torch.float32, device=fr.device)
        launch = lambda: _capi.check(lib.gp_estimate_normals_from_covs(fr.ptr(fr.points_gpu), fr.ptr(fr.covs_gpu), fr.size(), C.c_void_p(normals.data_ptr()), None), "from_covs")
        for _ in range(5):
            launch()
        torch.cuda.synchronize()
        us = []
        for rep in range(REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(EVENT_REPS):
                launch()
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / EVENT_REPS)
        emit(call="from_covs", cloud=name, points=int(fr.size()), us_median=round(float(np.median(us)), 2), us_min=round(float(np.min(us)), 2), sha256_normals=sha(normals.cpu().numpy()))

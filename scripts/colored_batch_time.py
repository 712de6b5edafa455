"""Host-to-host time of 64 colored GICP factors linearised (and evaluated) TOGETHER through CorrespondenceFactorBatchGPU beside the same 64 factor objects through
their own single-factor calls.

The clouds are those of tests/test_colored_batch_gpu.py: colored_ref.two_plane_cloud() (4,000 points) with device-estimated covariances, normals and intensity
gradients as the one target, colored_ref.moved_copy() (2,500 points) with device-estimated covariances as the source; the 64 factors are over 64 device copies of
that source and share the target, its search structure and its gradients.  Every timed call is at a new pose (XI scaled by 1 + 1e-3 i, the same for all 64), so
every linearise searches.  The two forms are called in alternation -- the batch's synchronous host-pose linearise, its error evaluation, then the 64
linearize_delta calls and the 64 error calls -- so that neither finds the lines warmer than the other: --warmup rounds (default 10), then --reps (default 100)
timed ones, min, median and inter-quartile range per form, and the ratio of the medians.  Nothing is tuned: the batch is what LevenbergMarquardtGraphGPU would
build over these factors, the single calls are what a caller without it would make.

One JSON object per line; --out <file> writes them there too.  Run under a time limit:

  timeout -k 10 300 python scripts/colored_batch_time.py --out profiles/colored_batch_time.json"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

torch.set_num_threads(16)
import colored_ref  # noqa: E402
import gtsam_points_amd as gpa  # noqa: E402
from gtsam_points_amd import synthetic  # noqa: E402


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


reps, warmup, count, out_path = arg("--reps", 100), arg("--warmup", 10), arg("--factors", 64), arg("--out", "")
assert torch.cuda.is_available(), "colored_batch_time.py measures on the GPU"
rows = []


def emit(**row):
    row["device"] = torch.cuda.get_device_name(0)
    rows.append(row)
    print(json.dumps(row), flush=True)


def stats(ms):
    a = np.asarray(ms)
    q1, q3 = np.percentile(a, [25, 75])
    return dict(reps=len(a), ms_min=round(float(a.min()), 4), ms_median=round(float(np.median(a)), 4), ms_iqr=round(float(q3 - q1), 4))


XI = np.array([0.01, -0.02, 0.015, 0.10, -0.05, 0.03])
tp, tI = colored_ref.two_plane_cloud()
tgt = gpa.PointCloudGPU(tp, intensities=tI)
assert gpa.estimate_normals_covariances_gpu(tgt, 10) == 0
tree = gpa.KdTreeGPU(tgt)
grads = gpa.estimate_intensity_gradients_gpu(tgt, 10)
sp, sI = colored_ref.moved_copy(tp, tI, synthetic.expmap(XI))
first = gpa.PointCloudGPU(sp)
assert gpa.estimate_covariances_gpu(first, 10) == 0
scov = first.download("covs")
sources = [gpa.PointCloudGPU(sp, covs=scov, intensities=sI) for _ in range(count)]
factors = [gpa.IntegratedColoredGICPFactorGPU(0, 1, tgt, s, target_tree=tree, target_gradients=grads) for s in sources]
batch = gpa.CorrespondenceFactorBatchGPU(factors)
sizes = dict(factors=count, target_points=tgt.size(), source_points=sources[0].size())

eye = np.eye(4)
ms = {k: [] for k in ("batch_lin", "batch_err", "single_lin", "single_err")}
for it in range(warmup + reps):
    delta = synthetic.expmap(XI * (1.0 + 1e-3 * it))
    near = delta @ synthetic.expmap(0.1 * XI)
    deltas, nears = np.tile(delta, (count, 1, 1)), np.tile(near, (count, 1, 1))
    t0 = time.perf_counter()
    recs = batch.linearize_deltas(deltas)
    t1 = time.perf_counter()
    errs = batch.errors(deltas, nears)
    t2 = time.perf_counter()
    single = [f.linearize_delta(delta) for f in factors]
    t3 = time.perf_counter()
    single_errs = [f.error({0: eye, 1: near}) for f in factors]
    t4 = time.perf_counter()
    assert all(a.error == b.error and a.num_inliers == b.num_inliers for a, b in zip(recs, single)) and list(errs) == single_errs  # the two forms compute the same
    if it >= warmup:
        for k, dt in zip(ms, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
            ms[k].append(dt * 1e3)
inliers = int(recs[0].num_inliers)
emit(what=f"batch: one synchronous linearise of {count} colored GICP factors (search + tile kernel + finalize, one launch each)", inliers_per_factor=inliers, **sizes,
     **stats(ms["batch_lin"]))
emit(what=f"batch: one error evaluation of {count} colored GICP factors on the stored correspondences", **sizes, **stats(ms["batch_err"]))
emit(what=f"single: {count} linearize_delta calls, one factor each (three launches and a wait per call)", **sizes, **stats(ms["single_lin"]))
emit(what=f"single: {count} error calls, one factor each", **sizes, **stats(ms["single_err"]))
emit(what="ratio of the medians, single calls / batch", linearize=round(float(np.median(ms["single_lin"]) / np.median(ms["batch_lin"])), 3),
     error=round(float(np.median(ms["single_err"]) / np.median(ms["batch_err"])), 3), bytes_per_matched_point=132)
batch.close()
if out_path:
    with open(out_path, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")

"""Host-to-host time of one LM iteration of BASELINE configs[2]'s graph (synthetic.make_c3_graph: 256 VGICP factors over 64 poses, pose 0 held) through
bench_lm.GpuTrialGraph -- the values in device memory (gp_lm_graph_*), in two forms:

  trial    the interpreter driving linearize / try_lambda / accept (bench_lm.run_lm): every host entry of the graph is crossed once per trial
  native   the library's own loop over the same three calls (gp_lm_graph_optimize)

Each form runs its loop from the same start --reps times (default 15) after two warm-up runs, the two forms alternating; per form the median, minimum and
inter-quartile range of the runs' ms per iteration.  One JSON object per line; --out <file> writes them there too.  For comparing two builds of the library: fresh
processes, alternating.  Run it under a time limit:

  timeout -k 10 120 python scripts/lm_trial_time.py --out profiles/lm_trial_time.json"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench_lm  # noqa: E402
import gtsam_points_amd as gpa  # noqa: E402
from gtsam_points_amd import synthetic  # noqa: E402


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


reps, out_path = arg("--reps", 15), arg("--out", "")
assert torch.cuda.is_available(), "lm_trial_time.py measures on the GPU"
g = synthetic.make_c3_graph()
clouds = [gpa.PointCloudGPU(p, c) for p, c in g["clouds"]]
maps = []
for c in clouds:
    maps.append(gpa.GaussianVoxelMapGPU(1.0, target_points_drop_rate=0.0))
    maps[-1].insert(c)
factors = [gpa.IntegratedVGICPFactorGPU(t, s, maps[t], clouds[s]) for t, s in g["pairs"]]
truth = np.stack(g["stations"][: len(clouds)])
v0 = truth @ bench_lm.expmap_many(np.random.default_rng(8191).uniform(-0.1, 0.1, (len(clouds), 6)))
v0[0] = truth[0]
tg = bench_lm.GpuTrialGraph(gpa, factors, g["pairs"], len(clouds), fixed=0)
forms = dict(trial=lambda: bench_lm.run_lm(tg, v0, max_iterations=30), native=lambda: tg.native_loop(v0, max_iterations=30))
ms = {k: [] for k in forms}
shape = {}
for rep in range(reps + 2):
    for k, fn in forms.items():
        r = fn()
        shape[k] = (r["iterations"], r["inner_iterations"])
        if rep >= 2:
            ms[k].append(1e3 * r["seconds"] / r["iterations"])
rows = []
for k, a in ms.items():
    q1, q3 = np.percentile(a, [25, 75])
    rows.append(dict(graph="make_c3_graph: 256 VGICP factors over 64 poses", form=k, iterations=shape[k][0], inner_iterations=shape[k][1], reps=len(a),
                     ms_per_iteration_median=round(float(np.median(a)), 4), ms_per_iteration_min=round(float(np.min(a)), 4), ms_per_iteration_iqr=round(float(q3 - q1), 4),
                     device=torch.cuda.get_device_name(0)))
    print(json.dumps(rows[-1]), flush=True)
tg.close()
if out_path:
    with open(out_path, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")

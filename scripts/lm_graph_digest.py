"""SHA-256 digests of what the device-resident LM graph (gp_lm.hip) returns, for comparing two builds of the library bit for bit: run it on each build, diff the outputs.

Over the graphs of tests/lm_groups_graphs.py -- every non-empty subset of {VGICP, correspondence, pose factors}, on the block-sparse and on the dense one-pose system --
and each of the four settings (one-launch step or not, speculation or not): x, b, c, the trial error and the trial values of a rejected and of an accepted trial, and
the records after accept() + linearize(); then, per graph, the summary and the values of one optimize() from the same start.
One JSON object per line; --out <file> writes them there too.  Run it under a time limit:

  timeout -k 10 300 python scripts/lm_graph_digest.py --out profiles/lm_graph_digest.jsonl"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import gtsam_points_amd as gpa  # noqa: E402
import lm_groups_graphs as G  # noqa: E402

out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
assert torch.cuda.is_available(), "lm_graph_digest.py runs the graphs on the GPU"
out_file = open(out_path, "w") if out_path else None
sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def emit(**row):
    line = json.dumps(row)
    print(line, flush=True)
    if out_file:
        out_file.write(line + "\n")


scene = G.make_scene(gpa, np.load(os.path.join(ROOT, "tests", "golden", "kitti07_dec4.npz")))
for case in G.graph_cases():
    for form in ("sparse", "dense"):
        v0 = scene["v0"][: case[4]]
        for one_launch, spec in G.SETTINGS:
            g = G.make_graph(gpa, scene, case, form)
            emit(graph=case[0], form=form, one_launch=one_launch, speculation=spec, **{k: sha(a) for k, a in G.flat(G.run_protocol(g, v0, one_launch, spec))})
            g.close()
        g = G.make_graph(gpa, scene, case, form)
        values, summary = g.optimize(v0, max_iterations=8)
        emit(graph=case[0], form=form, optimize=summary, values=sha(values))
        g.close()
if out_file:
    out_file.close()

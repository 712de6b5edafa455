"""Host-to-host time of the public calls of the single-process sharded batch (gp_vgicp_multi_batch_*, csrc/gp_multi.hip) on the 10-factor graph of
tests/test_multi_gpu.py (tests/golden/kitti07_dec4.npz): construction, linearize and compute_error, for the plans a one-GPU box can run --

  use_rccl = 0 with 1, 2 and 4 contiguous shards (gp_shard_plan), and round-robin over 3 shards (non-contiguous: rows copied out one by one)
  use_rccl = 1 (all-reduce) and use_rccl = 2 (in-place all-gather) with one rank

The pass is host orchestration around the batch's kernels, so the wall time of the call is the measure.  Two forms:

  python scripts/multi_batch_time.py [--tree DIR] [--reps 40] [--creates 8]
      one process, one JSON line: per plan and call the median, minimum and inter-quartile range in ms.  --tree DIR imports the package (and with it the library)
      from another checkout that has been built; the graph's data always comes from this one.
  python scripts/multi_batch_time.py --compare PARENT_TREE [--processes 5] [--out profiles/multi_batch_split.json]
      for comparing two builds of the library: fresh processes of the first form, PARENT_TREE and this tree alternating (P1 N1 P2 N2 ...), never two at a time; stops
      at the first process that fails.  Per plan and call: every process's median, the parent's lowest-to-highest process median, the result's median of process
      medians and whether it lies inside the parent's range.

Run it under a time limit:  timeout -k 10 600 python scripts/multi_batch_time.py --compare ../parent --out profiles/multi_batch_split.json"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("create", "linearize", "compute_error")


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def measure(tree, reps, creates):
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ctypes as C

    import torch

    import gtsam_points_amd as gpa
    from gtsam_points_amd.distributed import MultiDeviceBatch, partition_factors
    from helpers import expmap

    assert torch.cuda.is_available(), "multi_batch_time.py measures on the GPU"
    assert os.path.realpath(os.path.dirname(gpa.__file__)) == os.path.realpath(os.path.join(tree, "gtsam_points_amd")), gpa.__file__
    lib = gpa.load()
    d = np.load(os.path.join(ROOT, "tests", "golden", "kitti07_dec4.npz"))
    rng = np.random.default_rng(8191)
    clouds = [gpa.PointCloudGPU(d[f"points_{i}"], d[f"covs_{i}"]) for i in range(5)]
    maps = []
    for c in clouds:
        maps.append(gpa.GaussianVoxelMapGPU(1.0, target_points_drop_rate=0.0))
        maps[-1].insert(c)
    pairs = [(0, 1), (1, 2), (2, 3), (3, 4), (0, 2), (1, 3), (2, 4), (0, 3), (1, 4), (0, 4)]
    factors = [gpa.IntegratedVGICPFactorGPU(i, j, maps[i], clouds[j]) for i, j in pairs]
    F = len(factors)
    values = {k: d["poses"][k] @ expmap(rng.uniform(-0.05, 0.05, 6)) for k in range(5)}
    deltas = [np.linalg.inv(values[i]) @ values[j] for i, j in pairs]
    poses = np.stack([np.ascontiguousarray(m.T).reshape(16) for m in deltas]).copy()
    poses2 = np.stack([np.ascontiguousarray((m @ expmap(rng.uniform(-0.01, 0.01, 6))).T).reshape(16) for m in deltas]).copy()
    weights = [int(lib.gp_vgicp_factor_num_points(f._h)) for f in factors]

    def contiguous(shards):
        shard_of = np.zeros(F, np.int32)
        for k, (b, e) in enumerate(partition_factors(weights, shards)):
            shard_of[b:e] = k
        return dict(shard_of=shard_of, num_shards=shards, use_rccl=0)

    plans = {"no_collective_1": contiguous(1), "no_collective_2": contiguous(2), "no_collective_4": contiguous(4),
             "no_collective_round_robin_3": dict(shard_of=np.arange(F) % 3, num_shards=3, use_rccl=0), "all_reduce_1_rank": dict(use_rccl=1), "all_gather_1_rank": dict(use_rccl=2)}
    out, err = np.zeros((F, 122)), np.zeros(F)
    result, first = {}, None
    for name, kwargs in plans.items():
        ms = {c: [] for c in CALLS}
        for rep in range(creates + 1):  # (the first construction of a plan is a warm-up, like the first three passes)
            t0 = time.perf_counter()
            mb = MultiDeviceBatch(factors, **kwargs)
            t1 = time.perf_counter()
            if rep:
                ms["create"].append(1e3 * (t1 - t0))
            if rep < creates:
                del mb
        for rep in range(reps + 3):
            t0 = time.perf_counter()
            gpa._capi.check(lib.gp_vgicp_multi_batch_linearize(mb._h, poses.ctypes.data, out.ctypes.data), "linearize")
            t1 = time.perf_counter()
            gpa._capi.check(lib.gp_vgicp_multi_batch_compute_error(mb._h, poses.ctypes.data, poses2.ctypes.data, err.ctypes.data), "compute_error")
            t2 = time.perf_counter()
            if rep >= 3:
                ms["linearize"].append(1e3 * (t1 - t0))
                ms["compute_error"].append(1e3 * (t2 - t1))
        first = (out.copy(), err.copy()) if first is None else first
        assert np.array_equal(out, first[0]) and np.array_equal(err, first[1]), name  # every plan gives the same bits
        del mb
        result[name] = {c: dict(median=round(float(np.median(a)), 4), min=round(float(np.min(a)), 4), iqr=round(float(np.subtract(*np.percentile(a, [75, 25]))), 4), reps=len(a))
                        for c, a in ms.items()}
    print(json.dumps(dict(tree=os.path.realpath(tree), device=torch.cuda.get_device_name(0), ms=result)), flush=True)


def compare(parent, processes, out_path):
    trees = dict(parent=os.path.realpath(parent), result=ROOT)
    runs = {k: [] for k in trees}
    for i in range(processes):
        for k, tree in trees.items():
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", tree, "--reps", str(arg("--reps", 40)), "--creates", str(arg("--creates", 8))],
                               capture_output=True, text=True, timeout=240)
            if p.returncode != 0:  # nothing more is started on the device behind a process that failed
                sys.exit(f"{k} process {i + 1} ended with {p.returncode}:\n{p.stderr[-2000:]}")
            runs[k].append(json.loads([line for line in p.stdout.splitlines() if line.startswith('{"tree"')][-1]))  # (RCCL may print a banner of its own at exit)
            print(f"{k} {i + 1}: linearize no_collective_1 {runs[k][-1]['ms']['no_collective_1']['linearize']['median']} ms", flush=True)
    rows = []
    for plan in runs["parent"][0]["ms"]:
        for call in CALLS:
            per = {k: [r["ms"][plan][call]["median"] for r in runs[k]] for k in trees}
            lo, hi, med = min(per["parent"]), max(per["parent"]), round(float(np.median(per["result"])), 4)
            rows.append(dict(plan=plan, call=call, parent_process_medians_ms=per["parent"], result_process_medians_ms=per["result"], parent_range_ms=[lo, hi],
                             parent_median_ms=round(float(np.median(per["parent"])), 4), result_median_ms=med, result_range_ms=[min(per["result"]), max(per["result"])],
                             inside_parent_range=bool(lo <= med <= hi)))
            print(json.dumps(rows[-1]), flush=True)
    doc = dict(what="scripts/multi_batch_time.py --compare: fresh processes alternating parent, result; per-process medians of the public calls' wall time in ms",
               graph="tests/golden/kitti07_dec4.npz: 10 VGICP factors over 5 clouds", device=runs["result"][0]["device"], processes_per_tree=processes,
               reps_per_process=arg("--reps", 40), creates_per_process=arg("--creates", 8), calls=rows, outside_parent_range=[f"{r['plan']}.{r['call']}" for r in rows if not r["inside_parent_range"]])
    if out_path:
        with open(out_path, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    if "--compare" in sys.argv:
        compare(arg("--compare", ""), arg("--processes", 5), arg("--out", ""))
    else:
        measure(os.path.realpath(arg("--tree", ROOT)), arg("--reps", 40), arg("--creates", 8))

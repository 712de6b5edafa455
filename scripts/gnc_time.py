"""Host wall time (every call ends in a synchronisation) of estimate_pose_gnc_gpu on the two golden scans and of its stages alone:

  target  tests/golden/kitti_00/000000.bin, source 000001.bin (full scans); D = 33 synthetic descriptors as in scripts/ransac_time.py: a source row is the row of the
          nearest target point plus noise for ~60 % of the points, random otherwise (the library takes descriptors as an input)
  calls   gnc_default            estimate_pose_gnc_gpu, GNCParams() as they are: 5000 queries, reciprocal check, no tuple test, the loop
          match_forward          match_features_gpu: the 5000 query rows among the other cloud's rows (the first matching launch)
          match_reciprocal       match_features_gpu: the 5000 forward matches among the query cloud's rows (the second)
          correspondences        find_feature_correspondences_gpu: both launches and the compaction
          correspondences_tuple  ... with tuple_check and 500 tuples (the ~2000 pairs are fewer than 3 x the default 1000, which would skip the stage): the tuple
                                 stage is the difference to `correspondences`
          loop_one_launch        gnc_align_correspondences_gpu on the pairs of `correspondences`: diameter, gather and the one-launch loop behind one wait
          loop_host_driven       the same number of alignments driven from the host through align_points_se3_gpu with uniform weights on the same pairs' points
                                 (one launch, one wait and one read of the pose per alignment: the public path before the loop existed; its weights would cost more)

Every call is warmed up; the calls then ALTERNATE for --reps rounds (default 31), so that the machine's noise is every call's noise: median, minimum, inter-quartile
range and range of each.  A median over some tens of calls on a shared machine shows a difference of tens of per cent, not of a few.  Writes one JSON document to
--out (default profiles/gnc_time.json).  Run it under a time limit:

  timeout -k 10 600 python scripts/gnc_time.py"""
import ctypes as C
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
torch.set_num_threads(16)
import gtsam_points_amd as gpa

reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 31
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "gnc_time.json")
assert torch.cuda.is_available(), "gnc_time.py measures on the GPU"
assert reps >= 20
D = 33


def scan(name):
    return np.fromfile(os.path.join(ROOT, "tests", "golden", "kitti_00", name), dtype=np.float32).reshape(-1, 3)


rng = np.random.default_rng(3)
target_pts, source_pts = scan("000000.bin"), scan("000001.bin")
target, source = gpa.PointCloudGPU(target_pts), gpa.PointCloudGPU(source_pts)
tree = gpa.KdTreeGPU(target)
nn = torch.empty((len(source_pts), 1), dtype=torch.int32, device=target.device)
sq = torch.empty((len(source_pts), 1), dtype=torch.float64, device=target.device)
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

params = gpa.GNCParams()
first, pairs = gpa.estimate_pose_gnc_gpu(target, source, tf_d, sf_d, params, return_pairs=True)
swapped = first.swapped  # the smaller scan queries
qf_d, of_d = (tf_d, sf_d) if swapped else (sf_d, tf_d)
nq = len(target_pts) if swapped else len(source_pts)
K = min(nq, params.max_init_samples)
rows_d = torch.tensor([j * nq // K + int(gpa.load().gp_ransac_sample_index(params.seed, j, 0, (j + 1) * nq // K - j * nq // K)) for j in range(K)], dtype=torch.int32).cuda()
forward_d, _ = gpa.match_features_gpu(of_d, qf_d, rows_d)
pr = pairs.cpu().numpy()
t64 = torch.from_numpy(target_pts[pr[:, 0]].astype(np.float64)).cuda()
s64 = torch.from_numpy(source_pts[pr[:, 1]].astype(np.float64)).cuda()
results = {}


def host_driven():
    for _ in range(first.num_alignments):
        gpa.align_points_se3_gpu(t64, s64)


def default():
    results["default"] = gpa.estimate_pose_gnc_gpu(target, source, tf_d, sf_d, params)


def with_tuples():
    results["tuple_pairs"] = int(gpa.find_feature_correspondences_gpu(target, source, tf_d, sf_d, gpa.GNCParams(tuple_check=True, max_num_tuples=500)).shape[0])


calls = [("gnc_default", default), ("match_forward", lambda: gpa.match_features_gpu(of_d, qf_d, rows_d)), ("match_reciprocal", lambda: gpa.match_features_gpu(qf_d, of_d, forward_d)),
         ("correspondences", lambda: gpa.find_feature_correspondences_gpu(target, source, tf_d, sf_d, params)), ("correspondences_tuple", with_tuples),
         ("loop_one_launch", lambda: gpa.gnc_align_correspondences_gpu(target, source, pairs, params)), ("loop_host_driven", host_driven)]
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
props = torch.cuda.get_device_properties(0)
v = results["default"]
doc = dict(device=torch.cuda.get_device_name(0), arch=props.gcnArchName.split(":")[0], compute_units=props.multi_processor_count,
           what="host wall time per call in ms, each call ending in a synchronisation; calls alternate within a round", target_points=len(target_pts), source_points=len(source_pts),
           dim=D, queries=K, swapped=bool(swapped), pairs=int(pr.shape[0]), pairs_after_tuple_test=results["tuple_pairs"], tuples=500, num_alignments=v.num_alignments, inlier_rate=v.inlier_rate,
           final_mu=v.final_mu, pair_array_bytes=int(pr.shape[0]) * 24, rows=rows)
with open(out_path, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")

"""The graphs of tests/test_lm_groups_gpu.py and scripts/lm_graph_digest.py: every non-empty subset of {VGICP, correspondence, pose factors} in the device-resident LM
graph, each as a graph with one pose held (the block-sparse system) and with all but one held (the dense one-pose system), and the protocol both run on them.

Shapes: with both batches present (F, G) = (3, 1) and (1, 3) over three poses, so that each group in turn is the largest of LmPoseView::threads() = max(F, G, N); the pose factors alone
over four poses (F = G = 0: the poses are).  Sources are slices of 257, 255 and 1 points of the kitti07 submaps (the sizes that straddle the tile and wave edges in
the correspondence tests), targets the whole submaps."""
import itertools

import numpy as np

import bench_lm
import normals_ref
import pose3_ref
from helpers import rigid

SIZES = (257, 255, 1)
VG_PAIRS = [(0, 1), (1, 2), (0, 2)]
CORR_PAIRS = [(0, 1), (1, 2), (0, 2)]  # GICP, ICP point-to-plane, ICP point-to-point
SETTINGS = list(itertools.product((True, False), (True, False)))  # (one_launch, speculation)
LAMBDA_REJECTED, LAMBDA_ACCEPTED = 1e4, 1e-3


def make_scene(gpu, kitti07):
    n = 4
    pts = [np.ascontiguousarray(kitti07[f"points_{i}"]) for i in range(n)]
    covs = [np.ascontiguousarray(kitti07[f"covs_{i}"]) for i in range(n)]
    targets, trees, maps = [], [], []
    for p, c in zip(pts, covs):
        targets.append(gpu.PointCloudGPU(p, c, normals=np.ascontiguousarray(normals_ref.reference_normals(p, c).astype(np.float32))))
        trees.append(gpu.KdTreeGPU(targets[-1]))
        maps.append(gpu.GaussianVoxelMapGPU(1.0, target_points_drop_rate=0.0))
        maps[-1].insert(targets[-1])

    def source(j, k):  # slice k of SIZES out of submap j (a different stretch per k)
        lo = 100 + 1000 * k
        return gpu.PointCloudGPU(np.ascontiguousarray(pts[j][lo : lo + SIZES[k]]), np.ascontiguousarray(covs[j][lo : lo + SIZES[k]]))

    vg = [gpu.IntegratedVGICPFactorGPU(i, j, maps[i], source(j, k)) for k, (i, j) in enumerate(VG_PAIRS)]
    corr = [gpu.IntegratedGICPFactorGPU(0, 1, targets[0], source(1, 0)),
            gpu.IntegratedICPFactorGPU(1, 2, targets[1], source(2, 1), target_tree=trees[1], use_point_to_plane=True),
            gpu.IntegratedICPFactorGPU(0, 2, targets[0], source(2, 2), target_tree=trees[0])]
    truth = rigid(np.stack([np.asarray(T, dtype=np.float64) for T in kitti07["poses"][:n]]))
    v0 = rigid(truth @ bench_lm.expmap_many(np.random.default_rng(8191).uniform(-0.02, 0.02, (n, 6))))
    v0[0] = truth[0]
    sig = np.array([0.005] * 3 + [0.05] * 3)
    between = lambda a, b: gpu.BetweenFactorPose3(a, b, rigid((pose3_ref.inverse(truth[a]) @ truth[b])[None])[0], sigmas=sig)
    pose = [gpu.PriorFactorPose3(0, truth[0], information=1e6 * np.eye(6)), between(0, 1), between(1, 2), between(2, 3)]
    return dict(vg=vg, corr=corr, pose=pose, truth=truth, v0=v0, keep=(targets, trees, maps))


def graph_cases():
    """(name, F, G, number of pose factors, N)"""
    out = []
    for V, Cc, P in itertools.product((False, True), repeat=3):
        if not (V or Cc or P):
            continue
        shapes = [(3, 1), (1, 3)] if V and Cc else [(3 if V else 0, 3 if Cc else 0)]
        for F, G in shapes:
            N = 3 if F + G else 4
            out.append((f"F{F}_G{G}_P{N if P else 0}", F, G, N if P else 0, N))
    return out


def make_graph(gpu, scene, case, form):
    """form "sparse": pose 0 held; "dense": every pose but pose 1 held"""
    _, F, G, P, N = case
    fixed = (0,) if form == "sparse" else tuple(k for k in range(N) if k != 1)
    return gpu.LevenbergMarquardtGraphGPU(scene["vg"][:F], VG_PAIRS[:F], N, fixed=fixed, pose_factors=scene["pose"][:P], corr_factors=scene["corr"][:G], corr_pairs=CORR_PAIRS[:G])


def run_protocol(g, v0, one_launch, speculation):
    """a trial rejected at a large lambda, one that is accepted, then accept + linearize: everything they return, as arrays"""
    g.set_one_launch(one_launch)
    g.set_speculation(speculation)
    g.set_values(v0)
    g.linearize()
    out = {}
    for name, lam in (("rejected", LAMBDA_REJECTED), ("accepted", LAMBDA_ACCEPTED)):
        x, b, c, e, v = g.try_lambda(lam, want_values=True)
        out[name] = dict(x=x.copy(), b=b.copy(), c=np.float64(c), e=np.float64(e), values=v)
    g.accept()
    g.linearize()
    out["records"] = g.records().cpu().numpy()
    return out


def flat(result):
    """[(key, array)] of a run_protocol result in a fixed order"""
    items = [(f"{t}.{k}", np.ascontiguousarray(result[t][k])) for t in ("rejected", "accepted") for k in ("x", "b", "c", "e", "values")]
    return items + [("records", np.ascontiguousarray(result["records"]))]

"""SHA-256 digests of what the matching-cost factors on nearest-neighbour correspondences (gp_corr_factors.hip, gp_colored_factors.hip, gp_ct_factors.hip,
gp_corr_batch.hip) return, for comparing two builds of the library bit for bit: run it on each build, diff the outputs.

On tests/golden/kitti00_dec8.npz, for the GICP factor and both ICP modes (point-to-point, point-to-plane), at four linearisation poses

  identity | xi (the tests' XI) | general (xi with the 3x3 block orthonormal to 1e-6 only: the 92-sum kernels) | far (500 m above the scan: no correspondence)

and the source slices sp[100 : 100 + n], n in {1, 255, 257, 1024, 1025}, and the whole scan, each case does
  a linearise                                                                   -> record: the raw bytes of the gp_linearized6
  an error evaluation at a nearby pose on the stored correspondences            -> error_stored: the raw bytes of the double
  an error evaluation with a foreign pose_lin, which forces a new search        -> error_foreign
Behind those, on the slices only (and the whole scan for none of them):
  colored GICP (an intensity made up from the coordinates, gradients estimated on the device) and the LOAM factor as edge-only, plane-only and combined, with the
  validation off and on, through the same three calls
  one scripted sequence per kind that has update tolerances (ICP point, ICP plane, colored, LOAM combined), tolerances (0.05 rad, 0.5 m): linearise at A, linearise
  at a pose inside the tolerances, error with pose_lin = that pose, = A, = a foreign pose, linearise far away -> steps: one digest per call
  the continuous-time factors, both kinds: linearise, error, deskew (global and local)
  one batch of all six kinds interleaved (a combined LOAM member, an edge-only one, one with the validation on; slices of 1, 255, 257, 1024 and 1025 points):
  gp_corr_batch_linearize rigid and general, the device-pose entry into sets 0 and 1, the errors of both sets and of the host-pose call
One JSON object per line; --out <file> writes them there too.  The target normals are tests/normals_ref.reference_normals (host), so nothing but the factors is under test.
Run it under a time limit:

  timeout -k 10 300 python scripts/corr_factor_digest.py --out profiles/corr_family_digest.jsonl"""
import ctypes as C, hashlib, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import gtsam_points_amd as gpa
from gtsam_points_amd import _capi
from gtsam_points_amd.synthetic import expmap
from gtsam_points_amd.types import _pose16
import normals_ref

out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
assert torch.cuda.is_available(), "corr_factor_digest.py runs the factors on the GPU"
lib = gpa.load()
out_file = open(out_path, "w") if out_path else None

XI = np.array([0.01, -0.02, 0.015, 0.10, -0.05, 0.03])
NEARBY = np.array([0.002, -0.001, 0.003, 0.01, 0.02, -0.01])
FOREIGN = np.array([0.01, 0.0, -0.01, 0.05, 0.0, 0.02])
general = expmap(XI)
general[:3, :3] = general[:3, :3] @ (np.eye(3) + 1e-6 * np.random.default_rng(11).normal(size=(3, 3)))
POSES = [("identity", np.eye(4)), ("xi", expmap(XI)), ("general", general), ("far", expmap([0.0, 0.0, 0.0, 0.0, 0.0, 500.0]))]

d = np.load(os.path.join(ROOT, "tests", "golden", "kitti00_dec8.npz"))
tp, tc, sp, sc = d["target_points"], d["target_covs"], d["source_points"], d["source_covs"]
normals = np.ascontiguousarray(normals_ref.reference_normals(tp, tc).astype(np.float32))
tgt = gpa.PointCloudGPU(tp, tc, normals=normals)
tree = gpa.KdTreeGPU(tgt)
sha = lambda raw: hashlib.sha256(raw).hexdigest()


def emit(line):
    print(line, flush=True)
    if out_file:
        out_file.write(line + "\n")



for n in [1, 255, 257, 1024, 1025, len(sp)]:
    lo = 0 if n == len(sp) else 100
    src = gpa.PointCloudGPU(np.ascontiguousarray(sp[lo : lo + n]), np.ascontiguousarray(sc[lo : lo + n]))
    for what in ["gicp", "icp_point", "icp_plane"]:
        for pose_name, delta in POSES:
            if what == "gicp":
                f, prefix = gpa.IntegratedGICPFactorGPU(0, 1, tgt, src), "gp_gicp_factor"
            else:
                f, prefix = gpa.IntegratedICPFactorGPU(0, 1, tgt, src, target_tree=tree, use_point_to_plane=what == "icp_plane"), "gp_icp_factor"
            linearize, compute_error = getattr(lib, prefix + "_linearize"), getattr(lib, prefix + "_compute_error")
            rec, e_stored, e_foreign = _capi.Linearized6(), C.c_double(), C.c_double()
            _capi.check(linearize(f._h, _pose16(delta), C.byref(rec)), prefix + "_linearize")
            nearby = delta @ expmap(NEARBY)
            _capi.check(compute_error(f._h, _pose16(delta), _pose16(nearby), C.byref(e_stored)), prefix + "_compute_error")
            _capi.check(compute_error(f._h, _pose16(delta @ expmap(FOREIGN)), _pose16(nearby), C.byref(e_foreign)), prefix + "_compute_error")
            line = json.dumps(dict(factor=what, pose=pose_name, n=n, num_inliers=int(rec.num_inliers), record=sha(bytes(rec)), error_stored=sha(bytes(e_stored)),
                                   error_foreign=sha(bytes(e_foreign))))
            emit(line)
            del f

# ---- the rest of the family, on the slices ------------------------------------------------------------------------------------------------------------------------
intensity = lambda p: np.ascontiguousarray((0.5 + 0.25 * np.sin(0.7 * p[:, 0]) * np.cos(0.5 * p[:, 1]) + 0.1 * np.sin(1.3 * p[:, 2])).astype(np.float32))
SLICES = [1, 255, 257, 1024, 1025]
ctgt = gpa.PointCloudGPU(tp, tc, normals=normals, intensities=intensity(tp))
ctree = gpa.KdTreeGPU(ctgt)
grads = gpa.estimate_intensity_gradients_gpu(ctgt, 10)
te, tpl = gpa.PointCloudGPU(np.ascontiguousarray(tp[0::2])), gpa.PointCloudGPU(np.ascontiguousarray(tp[1::2]))
tree_e, tree_p = gpa.KdTreeGPU(te), gpa.KdTreeGPU(tpl)


def source(n, lo=100):
    return gpa.PointCloudGPU(np.ascontiguousarray(sp[lo : lo + n]), np.ascontiguousarray(sc[lo : lo + n]), intensities=intensity(sp[lo : lo + n]))


def make(what, src):
    """(factor, C prefix) of one member kind over the slice `src`"""
    if what == "gicp":
        return gpa.IntegratedGICPFactorGPU(0, 1, tgt, src), "gp_gicp_factor"
    if what in ("icp_point", "icp_plane"):
        return gpa.IntegratedICPFactorGPU(0, 1, tgt, src, target_tree=tree, use_point_to_plane=what == "icp_plane"), "gp_icp_factor"
    if what == "colored":
        return gpa.IntegratedColoredGICPFactorGPU(0, 1, ctgt, src, target_tree=ctree, target_gradients=grads), "gp_colored_gicp_factor"
    if what.startswith("loam_edge"):
        f = gpa.IntegratedPointToEdgeFactorGPU(0, 1, te, src, target_tree=tree_e)
    elif what.startswith("loam_plane"):
        f = gpa.IntegratedPointToPlaneFactorGPU(0, 1, tpl, src, target_tree=tree_p)
    else:
        f = gpa.IntegratedLOAMFactorGPU(0, 1, te, tpl, src, src, target_edges_tree=tree_e, target_planes_tree=tree_p)
    f.set_enable_correspondence_validation(what.endswith("_validated"))
    return f, "gp_loam_factor"


def call_linearize(f, prefix, delta):
    rec = _capi.Linearized6()
    _capi.check(getattr(lib, prefix + "_linearize")(f._h, _pose16(delta), C.byref(rec)), prefix + "_linearize")
    return rec


def call_error(f, prefix, lin, ev):
    e = C.c_double()
    _capi.check(getattr(lib, prefix + "_compute_error")(f._h, _pose16(lin), _pose16(ev), C.byref(e)), prefix + "_compute_error")
    return e


LOAMS = ["loam_edge", "loam_plane", "loam", "loam_edge_validated", "loam_plane_validated", "loam_validated"]
for n in SLICES:
    src = source(n)
    for what in ["colored"] + LOAMS:
        for pose_name, delta in POSES:
            f, prefix = make(what, src)
            rec = call_linearize(f, prefix, delta)
            nearby = delta @ expmap(NEARBY)
            e_stored = call_error(f, prefix, delta, nearby)
            e_foreign = call_error(f, prefix, delta @ expmap(FOREIGN), nearby)
            emit(json.dumps(dict(factor=what, pose=pose_name, n=n, num_inliers=int(rec.num_inliers), record=sha(bytes(rec)), error_stored=sha(bytes(e_stored)),
                                 error_foreign=sha(bytes(e_foreign)))))
            del f

# the update tolerances: A, a pose inside them, the three error evaluations, a pose far outside
A = expmap(XI)
INSIDE = A @ expmap([0.004, -0.003, 0.002, 0.05, -0.04, 0.03])
AWAY = A @ expmap([0.3, -0.2, 0.1, 2.0, -1.0, 0.5])
for n in SLICES:
    src = source(n)
    for what in ["icp_point", "icp_plane", "colored", "loam"]:
        f, prefix = make(what, src)
        f.set_correspondence_update_tolerance(0.05, 0.5)
        nearby = INSIDE @ expmap(NEARBY)
        steps = [bytes(call_linearize(f, prefix, A)), bytes(call_linearize(f, prefix, INSIDE)), bytes(call_error(f, prefix, INSIDE, nearby)),
                 bytes(call_error(f, prefix, A, nearby)), bytes(call_error(f, prefix, A @ expmap(FOREIGN), nearby)), bytes(call_linearize(f, prefix, AWAY))]
        emit(json.dumps(dict(factor=what, sequence="update_tolerance", n=n, steps=[sha(x) for x in steps])))
        del f

# the continuous-time factors
for n in SLICES:
    src = source(n)
    src.add_times((0.1 * np.arange(n) / n).astype(np.float32))
    for what, cls in [("ct_icp", gpa.IntegratedCTICPFactorGPU), ("ct_gicp", gpa.IntegratedCTGICPFactorGPU)]:
        f = cls(0, 1, tgt, src, target_tree=tree)
        v_lin, v_eval = {0: np.eye(4), 1: expmap(XI)}, {0: expmap(NEARBY), 1: expmap(XI) @ expmap(NEARBY)}
        fac = f.linearize(v_lin)
        rec = b"".join(np.ascontiguousarray(fac.G[k]).tobytes() for k in sorted(fac.G)) + b"".join(np.ascontiguousarray(g).tobytes() for g in fac.g)
        err = np.float64(f.error(v_eval)).tobytes()
        emit(json.dumps(dict(factor=what, n=n, num_inliers=int(f.num_inliers()), record=sha(rec), constant=sha(np.float64(fac.f).tobytes()), error=sha(err),
                             deskew=sha(f.deskewed_source_points(v_eval).tobytes()), deskew_local=sha(f.deskewed_source_points(v_eval, local=True).tobytes()))))
        del f

# one batch of all six kinds, interleaved
KINDS = ["loam", "gicp", "loam_edge", "colored", "icp_point", "loam_validated", "icp_plane", "colored"]
SIZES = [257, 1, 255, 1025, 1024, 1025, 257, 255]
STARTS = [3100, 7000, 500, 2000, 800, 4000, 100, 6000]
SCALES = [1.0, 0.8, 1.2, 0.6, 1.0, 0.9, 1.1, 0.7]
sources = [source(n, a) for n, a in zip(SIZES, STARTS)]
members = [make(k, s)[0] for k, s in zip(KINDS, sources)]
batch = gpa.CorrespondenceFactorBatchGPU(members)
deltas = np.stack([expmap(XI * s) for s in SCALES])
gen = deltas.copy()
gen[:, :3, :3] = gen[:, :3, :3] @ (np.eye(3) + 1e-6 * np.random.default_rng(11).normal(size=(3, 3)))
near = deltas @ expmap(NEARBY)
fields = ["H_target", "H_source", "H_target_source", "b_target", "b_source", "error", "num_inliers"]
records = lambda recs: sha(b"".join(np.ascontiguousarray(np.float64(getattr(r, k))).tobytes() for r in recs for k in fields))
for corr_set in (None, 0, 1):
    for rigid, poses in ((True, deltas), (False, gen)):
        recs = batch.linearize_deltas(poses, rigid=rigid, corr_set=corr_set)
        errs = batch.errors(poses, near, corr_set=corr_set)
        emit(json.dumps(dict(batch="six_kinds", corr_set=corr_set, rigid=rigid, num_inliers=[int(r.num_inliers) for r in recs], records=records(recs), errors=sha(errs.tobytes()))))
batch.close()
if out_file:
    out_file.close()

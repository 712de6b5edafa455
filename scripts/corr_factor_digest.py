"""SHA-256 digests of what the GICP and ICP factors (gp_corr_factors.hip) return, for comparing two builds of the library bit for bit: run it on each build, diff the outputs.

On tests/golden/kitti00_dec8.npz, for the GICP factor and both ICP modes (point-to-point, point-to-plane), at four linearisation poses

  identity | xi (the tests' XI) | general (xi with the 3x3 block orthonormal to 1e-6 only: the 92-sum kernels) | far (500 m above the scan: no correspondence)

and the source slices sp[100 : 100 + n], n in {1, 255, 257, 1024, 1025}, and the whole scan, each case does
  a linearise                                                                   -> record: the raw bytes of the gp_linearized6
  an error evaluation at a nearby pose on the stored correspondences            -> error_stored: the raw bytes of the double
  an error evaluation with a foreign pose_lin, which forces a new search        -> error_foreign
One JSON object per line; --out <file> writes them there too.  The target normals are tests/normals_ref.reference_normals (host), so nothing but the factors is under test.
Run it under a time limit:

  timeout -k 10 300 python scripts/corr_factor_digest.py --out profiles/corr_factor_digest.jsonl"""
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
            print(line, flush=True)
            if out_file:
                out_file.write(line + "\n")
            del f
if out_file:
    out_file.close()

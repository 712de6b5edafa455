"""bench.py's plain run on the GPU: it times exactly --steps steps, runs nothing behind the headline (no CPU baseline, no cold protocol, no detail file), and
--dump-outputs writes the records of its last timed step -- the same record the library's synchronous call computes on the same seeded inputs."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import BLOCKS, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step(gpu, tmp_path):
    from gtsam_points_amd import synthetic

    out, detail = tmp_path / "out", tmp_path / "bench_detail.json"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "3", "--device-warmup-ms", "50", "--source-points", "200000",
           "--target-points", "400000", "--dump-outputs", str(out), "--detail-file", str(detail)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    r = json.loads(p.stdout.rstrip("\n").splitlines()[-1])
    assert r["steps"] == 7 and r["warmup"] == 3 and r["ms_per_step"] > 0 and r["full"] is False
    assert abs(r["value"] - 200000 / (r["ms_per_step"] * 1e-3)) <= 0.02 * r["value"]
    assert r["cpu_baseline"] is None and r["ms_per_step_cold"] is None and r["legs"] == {} and r["detail_file"] is None and not detail.exists()

    got = {name: np.load(out / (name + ".npy")) for name in BLOCKS + ["error", "num_inliers"]}
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["H_target"].shape == (1, 6, 6) and got["b_source"].shape == (1, 6) and got["error"].shape == (1,) and got["num_inliers"].shape == (1,)

    # the same seeded workload and pose through the synchronous per-factor call
    d = synthetic.make_c2_workload(200000, 400000, seed=42)
    vm = gpu.GaussianVoxelMapGPU(0.5, target_points_drop_rate=0.0)
    vm.insert(gpu.PointCloudGPU(d["target_points"], d["target_covs"]))
    f = gpu.IntegratedVGICPFactorGPU(0, 1, vm, gpu.PointCloudGPU(d["source_points"], d["source_covs"]))
    delta = d["T_true"] @ synthetic.expmap([2e-4, -1e-4, 1.5e-4, 0.02, -0.01, 0.015])
    rec = gpu._capi.Linearized6()
    gpu._capi.check(f._lib.gp_vgicp_factor_linearize(f._h, gpu.types._pose16(delta), C.byref(rec)), "linearize")
    L = gpu.LinearizedSystem6(rec)
    assert int(got["num_inliers"][0]) == L.num_inliers > 100000
    for k in BLOCKS:
        assert rel_err(got[k][0], getattr(L, k)) <= 1e-12, k
    assert abs(got["error"][0] - L.error) <= 1e-12 * L.error

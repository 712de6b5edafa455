"""The arrival protocol of the fused finalize at the sizes where a single factor changes form, and the recovery of the by-factor linearise.

A single factor of the stream family selects its form by tile count: below 256 tiles the factor's last tile workgroup finalizes it (by factor), from 256 tiles up
the last workgroup of each of eight parts of the tile list does (by part), and from 65536 points up the tile list is a balanced plan.  Whatever the form, the fused
call (GP_TUNE_FUSED_FINALIZE 1) must return the bits of the two-kernel form (0), and a call whose completion words cannot arrive (GP_TUNE_TEST_ARRIVAL_SKEW) must
finish through the finalize kernel with the same bits and leave the next call fused again."""
import ctypes as C

import numpy as np
import pytest

from helpers import expmap

pytestmark = pytest.mark.gpu

FUSED, SKEW = 17, 20  # GP_TUNE_FUSED_FINALIZE, GP_TUNE_TEST_ARRIVAL_SKEW


@pytest.fixture(scope="module")
def scene(gpu):
    """one small map and 65536 source points (the sizes below are prefixes of them), six poses around the truth"""
    from gtsam_points_amd import synthetic

    d = synthetic.make_pair(65536, 20000, seed=23)
    assert len(d["source_points"]) == 65536
    tgt = gpu.PointCloudGPU(d["target_points"], d["target_covs"])
    vm = gpu.GaussianVoxelMapGPU(0.5, target_points_drop_rate=0.0)
    vm.insert(tgt)
    rng = np.random.default_rng(5)
    poses = [np.ascontiguousarray((d["T_true"] @ expmap(rng.uniform(-2e-3, 2e-3, 6))).T).reshape(1, 16).copy() for _ in range(6)]
    return dict(d=d, tgt=tgt, vm=vm, poses=poses)


def _source(gpu, scene, n):
    d = scene["d"]
    if n == 0:  # (a cloud needs an allocation: one point, none of them counted)
        c = gpu.PointCloudGPU(np.zeros((1, 3), np.float32), np.zeros((1, 3, 3), np.float32))
        c.num_points = 0
        return c
    return gpu.PointCloudGPU(d["source_points"][:n], d["source_covs"][:n])


class _Batch:
    def __init__(self, gpu, factors):
        self.gpu, self.lib, self.F = gpu, gpu.load(), len(factors)
        self.factors = factors
        self.h, self.s = C.c_void_p(), C.c_void_p()
        gpu._capi.check(self.lib.gp_stream_create(C.byref(self.s)), "stream")
        gpu._capi.check(self.lib.gp_vgicp_batch_create((C.c_void_p * self.F)(*[f._h.value for f in factors]), self.F, self.s, C.byref(self.h)), "batch")

    def tune(self, key, value):
        self.gpu._capi.check(self.lib.gp_vgicp_batch_set_tuning(self.h, key, value), "set_tuning")

    def linearize(self, P):
        out = np.full((self.F, 122), np.nan)
        self.gpu._capi.check(self.lib.gp_vgicp_batch_linearize(self.h, P.ctypes.data, out.ctypes.data), "linearize")
        return out

    def view(self, P):
        v = C.c_void_p()
        self.gpu._capi.check(self.lib.gp_vgicp_batch_linearize_view(self.h, P.ctypes.data, C.byref(v)), "linearize_view")
        return np.ctypeslib.as_array(C.cast(v, C.POINTER(C.c_double)), shape=(self.F, 122)).copy()

    def error(self, P, Q):
        e = np.full(self.F, np.nan)
        self.gpu._capi.check(self.lib.gp_vgicp_batch_compute_error(self.h, P.ctypes.data, Q.ctypes.data, e.ctypes.data), "compute_error")
        return e

    def fused_steps(self, reset=1):
        n = C.c_double()
        self.gpu._capi.check(self.lib.gp_vgicp_batch_device_times(self.h, reset, C.byref(n), None, None), "device_times")
        return n.value

    def close(self):
        self.lib.gp_vgicp_batch_destroy(self.h)
        self.lib.gp_stream_destroy(self.s)


@pytest.mark.parametrize("n", [65280, 65535, 65536])
def test_form_selection_at_its_edges(gpu, scene, n):
    """65280 points: 255 fixed 256-point tiles, by factor; 65535: 256 fixed tiles, by part without a plan; 65536: the smallest planned launch"""
    src = _source(gpu, scene, n)
    b = _Batch(gpu, [gpu.IntegratedVGICPFactorGPU(0, 1, scene["vm"], src)])
    poses = scene["poses"]
    try:
        recs, errs = {}, {}
        for mode in (1, 0):
            b.tune(FUSED, mode)
            b.fused_steps()
            recs[mode] = [b.linearize(p) for p in poses]
            errs[mode] = [b.error(poses[k], poses[(k + 1) % 6]) for k in range(6)]
            # the by-part fused linearise is the one that stamps its steps on the device clock
            assert b.fused_steps() == (6 if mode == 1 and n >= 65535 else 0), (n, mode)
        for k in range(6):
            assert recs[1][k][0, 0] > 1000 and np.isfinite(recs[1][k]).all(), (n, k)  # (the scan meets the map)
            assert np.array_equal(recs[1][k], recs[0][k]), (n, k)
            assert errs[1][k][0] > 0 and np.array_equal(errs[1][k], errs[0][k]), (n, k)
        if n != 65535:
            return
        # completion words that cannot arrive: the call finishes through the second kernel with the same bits, and the call after it is fused again
        b.tune(FUSED, 1)
        assert np.array_equal(b.linearize(poses[0]), recs[0][0])
        assert b.fused_steps() == 1
        b.tune(SKEW, 5)
        assert np.array_equal(b.linearize(poses[0]), recs[0][0])
        assert b.fused_steps(reset=0) == 0  # recovered: no device stamps
        assert np.array_equal(b.linearize(poses[0]), recs[0][0])
        assert b.fused_steps() == 1  # fused again
        b.tune(SKEW, 3)
        assert np.array_equal(b.error(poses[0], poses[1]), errs[0][0])
        assert np.array_equal(b.error(poses[0], poses[1]), errs[0][0])
        assert np.array_equal(b.linearize(poses[0]), recs[0][0])  # (the error's recovery reset the counters the linearise shares)
        assert b.fused_steps() == 1
    finally:
        b.close()


def test_by_factor_linearize_recovery(gpu, scene):
    """a batch of 300, 0 and 1000 points whose factor counter 0 is out of range: the linearise notices (word 0 does not arrive), cleans the counters and finishes through
    the finalize kernel -- every record, the empty factor's included, as the first call's and as the two-kernel form's; the call after it is fused again"""
    factors = [gpu.IntegratedVGICPFactorGPU(0, k + 1, scene["vm"], _source(gpu, scene, n)) for k, n in enumerate((300, 0, 1000))]
    b = _Batch(gpu, factors)
    P = np.ascontiguousarray(np.concatenate([scene["poses"][k] for k in range(3)]))
    try:
        b.tune(FUSED, 1)
        first = b.linearize(P)  # (the factor counters exist from here on)
        assert first[0, 0] > 0 and first[2, 0] > 0 and np.all(first[1] == 0.0)
        b.tune(SKEW, 1)
        second = b.linearize(P)
        third = b.linearize(P)
        viewed = b.view(P)
        b.tune(FUSED, 0)
        plain = b.linearize(P)
        for name, r in [("recovered", second), ("after the recovery", third), ("view", viewed), ("two-kernel form", plain)]:
            assert np.array_equal(r, first), name
    finally:
        b.close()

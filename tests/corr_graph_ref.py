"""The host-driven loop over GICP / ICP factors that the device-resident LM graph is compared against: run_lm's back end (bench_lm._Graph) over SINGLE-factor objects --
one linearize_delta call per factor, the records scattered into the normal equations by helpers.host_system, a numpy solve on A + lambda I, one error call per
factor on the correspondences of its last linearise.  This is the only way to optimise such factors without gp_corr_batch_* / gp_lm_graph_create_with_factors.

Optional extra record sources ride along in the documented record order of the device graph: VGICP records in FRONT (`vgicp`: a bench_lm.GpuGraph with
solver="host" over the same poses), pose factors BEHIND (`pose_factors`, through pose3_ref)."""
import numpy as np

import bench_lm
from helpers import host_system


def record_of(L):
    """a LinearizedSystem6-like object -> the 122 doubles of gp_linearized6 (6x6 blocks column-major)"""
    return np.concatenate([[float(L.num_inliers), float(L.error)], np.asarray(L.H_target).T.ravel(), np.asarray(L.H_source).T.ravel(), np.asarray(L.H_target_source).T.ravel(),
                           np.asarray(L.b_target), np.asarray(L.b_source)])


class HostCorrGraph(bench_lm._Graph):
    """factors[k]: an object with linearize_delta(delta) -> LinearizedSystem6-like and error_delta(lin_delta, delta) -> float (see DeviceFactor), between poses pairs[k]"""

    name = "host-corr"

    def __init__(self, factors, pairs, num_poses, fixed=0, vgicp=None, pose_factors=()):
        super().__init__(pairs, num_poses, fixed)
        self.f = list(factors)
        self.vgicp = vgicp
        self.pf = list(pose_factors)
        slots = [self.factor_slots]
        if vgicp is not None:
            slots.insert(0, vgicp.factor_slots)
        if self.pf:
            import pose3_ref

            slots.append(pose3_ref.factor_slots(self.pf, self.slot))
        self.slots_all = np.concatenate(slots).astype(np.int32)
        self.d_lin = None

    def close(self):
        if self.vgicp is not None:
            self.vgicp.close()

    def system(self, records):
        """(A, b, c) of the records in slots_all's order"""
        return host_system(np.asarray(records), self.slots_all, self.num_slots)

    def records(self, values):
        self.d_lin = self.deltas(values)
        recs = [record_of(f.linearize_delta(d)) for f, d in zip(self.f, self.d_lin)]
        if self.vgicp is not None:
            self.vgicp.linearize(values)
            recs = list(self.vgicp.rec_host) + recs
        if self.pf:
            import pose3_ref

            recs = recs + [pose3_ref.factor_record(f, values) for f in self.pf]
        return np.array(recs)

    def linearize(self, values):
        self.rec = self.records(values)
        self.A, self.b, c = self.system(self.rec)
        return c

    def solve(self, lam):
        return np.linalg.solve(self.A + lam * np.eye(len(self.b)), self.b), self.b, None

    def error(self, values):
        """at `values`, on the correspondences of the last linearize"""
        e = float(sum(f.error_delta(dl, d) for f, dl, d in zip(self.f, self.d_lin, self.deltas(values))))
        if self.vgicp is not None:
            e = self.vgicp.error(values) + e
        if self.pf:
            import pose3_ref

            e += float(sum(pose3_ref.factor_error(f, values) for f in self.pf))
        return e


class DeviceFactor:
    """an IntegratedGICPFactorGPU / IntegratedICPFactorGPU driven through its own single-factor entry points"""

    def __init__(self, factor):
        self.f = factor

    def linearize_delta(self, delta):
        return self.f.linearize_delta(delta)

    def error_delta(self, lin_delta, delta):
        assert np.array_equal(self.f.linearization_point, lin_delta)  # (the stored correspondences are those of lin_delta)
        return self.f.error({self.f.keys()[0]: np.eye(4), self.f.keys()[1]: delta})

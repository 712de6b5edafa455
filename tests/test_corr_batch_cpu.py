"""CPU checks of the correspondence-factor batch: the new entry points are declared, exported and bound, refuse bad arguments before any device work, and the host
graph the GPU tests compare against (tests/corr_graph_ref.py) assembles the normal equations as helpers.host_system does."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import corr_graph_ref
from helpers import host_system

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gp_corr_batch_create", "gp_corr_batch_destroy", "gp_corr_batch_size", "gp_corr_batch_stream", "gp_corr_batch_sync", "gp_corr_batch_issue_linearize_dev",
       "gp_corr_batch_issue_compute_error_dev", "gp_corr_batch_linearize", "gp_corr_batch_compute_error", "gp_lm_graph_create_with_factors"]


def test_new_symbols_are_declared_exported_and_bound():
    from gtsam_points_amd import _capi

    header = open(os.path.join(ROOT, "include", "gtsam_points_hip.h"), encoding="utf-8").read()
    exported = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    lib = _capi.load()
    for name in NEW:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert re.search(r" T " + name + r"$", exported, re.M), name
        assert name in _capi._SIGNATURES and getattr(lib, name).argtypes == _capi._SIGNATURES[name][1], name


def test_entry_points_refuse_bad_arguments_without_a_device():
    from gtsam_points_amd import _capi

    lib = _capi.load()
    h = C.c_void_p()
    assert lib.gp_corr_batch_create(None, 0, None, 0, None, C.byref(h)) == 1 and not h.value  # GP_ERROR_INVALID_ARGUMENT: an empty batch
    assert b"empty batch" in lib.gp_last_error()
    null = (C.c_void_p * 1)(None)
    assert lib.gp_corr_batch_create(null, 1, None, 0, None, C.byref(h)) == 1 and not h.value  # a NULL handle
    assert lib.gp_corr_batch_create(None, 1, None, 0, None, C.byref(h)) == 1 and lib.gp_corr_batch_create(None, 0, None, 0, None, None) == 1
    assert lib.gp_corr_batch_destroy(None) == 0 and lib.gp_corr_batch_size(None) == 0
    assert lib.gp_corr_batch_sync(None) == 1 and lib.gp_corr_batch_stream(None, None) == 1
    assert lib.gp_corr_batch_issue_linearize_dev(None, None, 1, 0, None) == 1 and lib.gp_corr_batch_issue_compute_error_dev(None, 0, None, None, None, None, 0) == 1
    assert lib.gp_corr_batch_linearize(None, None, 1, None) == 1 and lib.gp_corr_batch_compute_error(None, None, None, None) == 1
    # without a correspondence batch the new create is gp_lm_graph_create_with_pose_factors: a graph with no factor at all is refused there
    assert lib.gp_lm_graph_create_with_factors(None, None, None, None, None, 0, 2, None, 0, None, C.byref(h)) == 1 and not h.value
    assert b"gp_lm_graph_create_with_pose_factors" in lib.gp_last_error()


class _Rec:
    def __init__(self, rng):
        def spd():
            a = rng.normal(size=(6, 6))
            return a @ a.T

        self.num_inliers, self.error = int(rng.integers(1, 1000)), float(rng.uniform(1.0, 100.0))
        self.H_target, self.H_source, self.H_target_source = spd(), spd(), rng.normal(size=(6, 6))
        self.b_target, self.b_source = rng.normal(size=6), rng.normal(size=6)

    def linearize_delta(self, delta):
        return self

    def error_delta(self, lin_delta, delta):
        return self.error


def test_host_graph_assembles_like_helpers_host_system():
    rng = np.random.default_rng(3)
    pairs = [(0, 1), (1, 2), (0, 2), (2, 3), (3, 1)]
    recs = [_Rec(rng) for _ in pairs]
    g = corr_graph_ref.HostCorrGraph(recs, pairs, 4, fixed=0)
    values = np.tile(np.eye(4), (4, 1, 1))
    c = g.linearize(values)
    packed = np.array([corr_graph_ref.record_of(r) for r in recs])
    # record_of packs the 6x6 blocks column-major, as gp_linearized6 holds them
    assert packed.shape == (5, 122) and packed[2, 2 + 6 * 1 + 0] == recs[2].H_target[0, 1] and packed[2, 74 + 6 * 4 + 2] == recs[2].H_target_source[2, 4]
    assert np.array_equal(packed[:, 110:116], np.array([r.b_target for r in recs]))
    slots = [(-1, 0), (0, 1), (-1, 1), (1, 2), (2, 0)]  # pose 0 held: poses 1, 2, 3 are slots 0, 1, 2
    assert np.array_equal(g.slots_all, np.array(slots))
    A, b, cc = host_system(packed, slots, 3)
    assert np.array_equal(g.A, A) and np.array_equal(g.b, b) and c == cc == sum(r.error for r in recs)
    # ... and that is the sum of the blocks by hand: the diagonal block of pose 2 (slot 1) and the cross block of poses 3 -> 1 (slots 2, 0)
    assert np.allclose(A[6:12, 6:12], recs[1].H_source + recs[2].H_source + recs[3].H_target)
    assert np.allclose(A[12:18, 0:6], recs[4].H_target_source) and np.allclose(A[0:6, 12:18], recs[4].H_target_source.T)
    assert np.allclose(b[0:6], -(recs[0].b_source + recs[1].b_target + recs[4].b_source))
    assert g.error(values) == sum(r.error for r in recs)
    dx, bb, _ = g.solve(1e-3)
    assert np.allclose((A + 1e-3 * np.eye(18)) @ dx, b)

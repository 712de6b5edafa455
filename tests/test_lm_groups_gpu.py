"""The device-resident LM graph over its table of pairwise groups (gp_lm.hip: PairGroup) and its one damped-system seam
(gp::DampedSystem): every non-empty subset of {VGICP, correspondence, pose factors}, on the block-sparse and on the dense one-pose system (tests/lm_groups_graphs.py),
returns the same bytes whether the step is one launch or several and whether the next linearise is queued ahead or not; the poses follow tests/pose3_ref.py; and the
one create path refuses an all-held graph and a bad pair in either group."""
import ctypes as C

import numpy as np
import pytest

import lm_groups_graphs as G
import pose3_ref

pytestmark = pytest.mark.gpu
INVALID = 1  # GP_ERROR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def scene(gpu, kitti07):
    return G.make_scene(gpu, kitti07)


@pytest.fixture(scope="module")
def results(gpu, scene):
    """{(case name, form): [run_protocol result per setting of G.SETTINGS]}, computed once"""
    out = {}
    for case in G.graph_cases():
        for form in ("sparse", "dense"):
            runs = []
            for one_launch, spec in G.SETTINGS:
                g = G.make_graph(gpu, scene, case, form)
                assert g.n == (6 * (case[4] - 1) if form == "sparse" else 6)
                runs.append(G.run_protocol(g, scene["v0"][: case[4]], one_launch, spec))
                g.close()
            out[(case[0], form)] = runs
    return out


def test_the_cases_cover_every_subset_and_every_front_of_the_thread_count():
    cases = G.graph_cases()
    assert {(F > 0, Gc > 0, P > 0) for _, F, Gc, P, _ in cases} == {s for s in [(a, b, c) for a in (False, True) for b in (False, True) for c in (False, True)] if any(s)}
    shapes = {(F, Gc, N) for _, F, Gc, _, N in cases}
    assert (3, 1, 3) in shapes and (1, 3, 3) in shapes and (0, 0, 4) in shapes  # F, G and N in turn the (joint) largest of max(F, G, N)


@pytest.mark.parametrize("form", ["sparse", "dense"])
def test_trials_and_records_do_not_depend_on_launch_form_or_speculation(results, form):
    for case in G.graph_cases():
        runs = results[(case[0], form)]
        ref = G.flat(runs[0])
        assert ref[-1][1].shape == (case[1] + case[2] + case[3], 122)
        for (key, a) in ref:
            assert np.isfinite(a).all(), (case[0], form, key)
        # the larger lambda gives the shorter step, and both trials moved
        assert 0 < np.linalg.norm(runs[0]["rejected"]["x"]) < np.linalg.norm(runs[0]["accepted"]["x"]), (case[0], form)  # (|x(lambda)| falls with lambda)
        for setting, run in zip(G.SETTINGS[1:], runs[1:]):
            for (key, a), (_, b) in zip(ref, G.flat(run)):
                assert a.tobytes() == b.tobytes(), (case[0], form, setting, key)


@pytest.mark.parametrize("form", ["sparse", "dense"])
def test_trial_values_follow_pose3(results, scene, form):
    """the trial values are T Expmap(x of the pose's slot) for the free poses and the held poses as they were, to the 1e-13 of tests/test_lm_edges_gpu.py"""
    for case in G.graph_cases():
        N = case[4]
        v0 = scene["v0"][:N]
        free = list(range(1, N)) if form == "sparse" else [1]
        scale = max(1.0, float(np.abs(v0).max()))
        for trial in ("rejected", "accepted"):
            t = results[(case[0], form)][0][trial]
            for k in range(N):
                want = v0[k] @ pose3_ref.expmap(t["x"][6 * free.index(k) : 6 * free.index(k) + 6]) if k in free else v0[k]
                assert np.abs(t["values"][k] - want).max() <= 1e-13 * scale, (case[0], form, trial, k)


def test_relative_poses_follow_pose3(gpu, scene):
    """the VGICP group's relative poses after set_values are inverse(T_t) T_s, to the same 1e-13, with the correspondence group beside it in either proportion.
    gp_lm_graph_records hands out that one table only: the correspondence group's relative poses, and both groups' after a retract, are held through what is computed
    from them -- the records and trial errors of the byte comparisons above, and the trial values against pose3_ref"""
    lib = gpu.load()
    for case in [c for c in G.graph_cases() if c[1] > 0]:
        F, N = case[1], case[4]
        g = G.make_graph(gpu, scene, case, "sparse")
        v0 = scene["v0"][:N]
        g.set_values(v0)
        g.linearize()
        g.sync()
        rel_p = C.c_void_p()
        gpu._capi.check(lib.gp_lm_graph_records(g._h, None, C.byref(rel_p)), "gp_lm_graph_records")
        rel = np.zeros(16 * F)
        gpu._capi.check(lib.gp_memcpy_d2h(rel.ctypes.data, rel_p, 8 * rel.size, None), "gp_memcpy_d2h")
        gpu._capi.check(lib.gp_stream_synchronize(None), "gp_stream_synchronize")
        rel = rel.reshape(F, 4, 4).transpose(0, 2, 1)
        scale = max(1.0, float(np.abs(v0).max()))
        for f, (i, j) in enumerate(G.VG_PAIRS[:F]):
            assert np.abs(rel[f] - pose3_ref.inverse(v0[i]) @ v0[j]).max() <= 1e-13 * scale, (case[0], f)
        g.close()


def test_create_refuses_all_held_and_bad_pairs_in_either_group(gpu, scene):
    lib = gpu.load()
    case = next(c for c in G.graph_cases() if c[1] == 3 and c[2] == 1 and c[3] == 0)
    g = G.make_graph(gpu, scene, case, "sparse")  # (its two batches serve the refused creates)
    good_v, good_c = np.array(G.VG_PAIRS, dtype=np.int32), np.array(G.CORR_PAIRS[:1], dtype=np.int32)
    held0, held_all = np.array([1, 0, 0], dtype=np.uint8), np.ones(3, dtype=np.uint8)

    def create(vp, cp, held):
        h = C.c_void_p()
        rc = lib.gp_lm_graph_create_with_factors(g._batch, vp.ctypes.data, g._corr._h, cp.ctypes.data, None, 0, 3, held.ctypes.data, 4, None, C.byref(h))
        return rc, h

    rc, h = create(good_v, good_c, held0)
    assert rc == 0 and h.value  # (the arguments the refusals below spoil one at a time are good)
    lib.gp_lm_graph_destroy(h)
    for what, vp, cp, held in [("all held", good_v, good_c, held_all)] + [
            (f"{group} pair {bad}", np.array(G.VG_PAIRS[:2] + [bad], dtype=np.int32) if group == "vgicp" else good_v,
             np.array([bad], dtype=np.int32) if group == "corr" else good_c, held0)
            for group in ("vgicp", "corr") for bad in [(0, 3), (-1, 1), (2, 2)]]:
        rc, h = create(vp, cp, held)
        assert rc == INVALID and not h.value, what
    g.close()

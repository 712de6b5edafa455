"""CPU checks of the registration unit's build products: RANSAC's scoring kernel and the feature-search kernel as the compiler's resource remarks list them, neither
with scratch or spills; and the argument refusals that are made on the host before any device work."""
import ctypes as C
import os

from test_icp_build_cpu import ROOT, _assert_no_scratch

RES = os.path.join(ROOT, "gtsam_points_amd", "csrc", "gp_registration.resources.txt")


def _kernels():
    assert os.path.exists(RES), "build the HIP library first (python -c 'import __graft_entry__ as g; g.build()')"
    return {b.split()[0]: b for b in open(RES).read().split("remark: Function Name: ")[1:]}


def test_scoring_and_feature_search_kernels_use_no_scratch():
    ks = _kernels()
    hot = {k: v for k, v in ks.items() if "occupancy_overlap_batch_kernel" in k or "feature_nn_kernel" in k}
    assert len(hot) == 2, sorted(ks)
    _assert_no_scratch(hot)


def test_every_kernel_of_the_unit_uses_no_scratch():
    ks = _kernels()
    for name in ("occupancy_insert_kernel", "occupancy_rehash_kernel", "occupancy_overlaps_kernel", "align_points_kernel", "ransac_sample_kernel", "ransac_rows_kernel",
                 "ransac_hypothesis_kernel", "ransac_select_kernel"):
        assert sum(name in k for k in ks) == 1, name
    _assert_no_scratch(ks)


def test_entry_points_refuse_bad_arguments_without_a_device():
    from gtsam_points_amd import _capi

    lib = _capi.load()
    h = C.c_void_p()
    assert lib.gp_occupancy_grid_create(0.0, None, C.byref(h)) == 1 and not h.value and b"resolution" in lib.gp_last_error()
    assert lib.gp_occupancy_grid_destroy(None) == 0 and lib.gp_occupancy_grid_num_occupied_cells(None) == 0
    assert lib.gp_occupancy_grid_insert(None, None, 0, None) == 1 and lib.gp_occupancy_grid_overlap(None, None, 0, None, None) == 1
    fake = C.c_void_p(64)  # never dereferenced
    assert lib.gp_feature_nn_search(fake, 4, fake, 4, 129, None, 4, fake, fake, None) == 1 and b"128" in lib.gp_last_error()
    assert lib.gp_feature_nn_search(fake, 0, fake, 4, 33, None, 4, fake, fake, None) == 1
    p = _capi.RansacParams()
    lib.gp_ransac_params_default(C.byref(p))
    assert (p.max_iterations, p.dof, p.chunk_iterations, p.num_taboo, p.seed) == (5000, 6, 1024, 0, 5489)  # registration/ransac.hpp:18-27
    assert (p.early_stop_inlier_rate, p.poly_error_thresh, p.inlier_voxel_resolution, p.taboo_thresh_trans) == (0.8, 0.5, 1.0, 0.25)
    res = _capi.RansacResult()

    def call(nt=10, ns=10, dim=33):
        return lib.gp_ransac_estimate_pose(fake, nt, fake, ns, fake, fake, dim, C.byref(p), None, None, C.byref(res), None)

    assert call(ns=2) == 1 and b"fewer source points" in lib.gp_last_error()
    assert call(nt=0) == 1 and b"empty" in lib.gp_last_error()
    assert call(dim=129) == 1 and call(dim=0) == 1
    p.dof = 5
    assert call() == 1 and b"dof" in lib.gp_last_error()
    p.dof, p.num_taboo = 4, 65
    assert call(ns=2) == 1 and b"taboo" in lib.gp_last_error()
    assert lib.gp_align_points(fake, fake, fake, 3, 5, (C.c_double * 16)(), None) == 1 and lib.gp_align_points(fake, fake, fake, 0, 6, (C.c_double * 16)(), None) == 1

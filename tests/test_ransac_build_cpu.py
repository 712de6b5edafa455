"""CPU checks of the three registration units' build products (csrc/gp_registration.hip: RANSAC and the N-point alignment; csrc/gp_occupancy.hip: the occupancy set;
csrc/gp_feature_match.hip: the exact feature search): each unit emits exactly its kernels, as the compiler's resource remarks list them, none with scratch or spills,
and each kernel stays within the registers and LDS of the build before the one unit was split into three; and the argument refusals that are made on the host before
any device work.

The bounds are the figures of the unsplit gp_registration.hip (HIP 7.2 / AMD clang 22, gfx950): upper bounds on SGPRs, VGPRs and LDS (bytes per workgroup).  The build
this test came with sits ON every figure: its kernels are the unsplit unit's instruction for instruction (align_points_kernel up to the names of two registers)."""
import ctypes as C
import os
import re

from test_icp_build_cpu import ROOT, _assert_no_scratch

# unit -> kernel -> SGPRs, VGPRs, LDS
UNITS = {
    "gp_registration": {"align_points_kernel": (36, 68, 18432), "ransac_sample_kernel": (50, 16, 0), "ransac_rows_kernel": (16, 6, 0),
                        "ransac_hypothesis_kernel": (44, 112, 0), "ransac_select_kernel": (24, 14, 4096)},
    "gp_occupancy": {"occupancy_insert_kernel": (36, 22, 0), "occupancy_rehash_kernel": (26, 20, 0), "occupancy_overlaps_kernel": (42, 22, 0),
                     "occupancy_overlap_batch_kernel": (58, 22, 0)},
    "gp_feature_match": {"feature_nn_kernel": (55, 76, 41216)},
}
HELPERS = ("host_flag_kernel",)  # what gp_host.hpp instantiates in every unit


def _kernels(unit):
    res = os.path.join(ROOT, "gtsam_points_amd", "csrc", unit + ".resources.txt")
    assert os.path.exists(res), "build the HIP library first (python -c 'import __graft_entry__ as g; g.build()')"
    return {b.split()[0]: b for b in open(res).read().split("remark: Function Name: ")[1:]}


def test_scoring_and_feature_search_kernels_use_no_scratch():
    ks = {**_kernels("gp_occupancy"), **_kernels("gp_feature_match")}
    for name in ("occupancy_overlap_batch_kernel", "feature_nn_kernel"):
        assert sum(name in k for k in ks) == 1, (name, sorted(ks))
    assert not any("occupancy_overlap_batch_kernel" in k or "feature_nn_kernel" in k for k in _kernels("gp_registration"))
    _assert_no_scratch({k: v for k, v in ks.items() if "occupancy_overlap_batch_kernel" in k or "feature_nn_kernel" in k})


def test_every_kernel_of_the_unit_uses_no_scratch():
    for unit, want in UNITS.items():
        ks = _kernels(unit)
        own = [k for k in ks if not any(h in k for h in HELPERS)]
        for name in want:
            assert sum(name in k for k in own) == 1, (unit, name)
        assert len(own) == len(want), (unit, sorted(own))  # nothing else: each kernel is compiled in one unit only
        _assert_no_scratch(ks)


def test_every_kernel_keeps_within_the_figures_of_the_unsplit_unit():
    for unit, want in UNITS.items():
        ks = _kernels(unit)
        for frag, (sgprs, vgprs, lds) in want.items():
            (name,) = [k for k in ks if frag in k]
            get = lambda key: int(re.search(re.escape(key) + r":\s+(\d+)", ks[name]).group(1))  # noqa: E731
            got = dict(sgprs=get("TotalSGPRs"), vgprs=get("    VGPRs"), lds=get("LDS Size [bytes/block]"))
            print(name, got)
            assert got["sgprs"] <= sgprs and got["vgprs"] <= vgprs and got["lds"] <= lds, (name, got)


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

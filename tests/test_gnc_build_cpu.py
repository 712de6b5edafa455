"""CPU checks of the GNC unit's build products: every kernel of csrc/gp_gnc.hip as the compiler's resource remarks list them, none with scratch or spills; the defaults
of gp_gnc_params; and the argument refusals that are made on the host before any device work."""
import ctypes as C
import os
import re

from test_icp_build_cpu import ROOT, _assert_no_scratch

RES = os.path.join(ROOT, "gtsam_points_amd", "csrc", "gp_gnc.resources.txt")


def test_every_kernel_of_the_unit_uses_no_scratch():
    assert os.path.exists(RES), "build the HIP library first (python -c 'import __graft_entry__ as g; g.build()')"
    ks = {b.split()[0]: b for b in open(RES).read().split("remark: Function Name: ")[1:]}
    for name in ("gnc_query_rows_kernel", "gnc_keep_kernel", "gnc_pairs_kernel", "gnc_tuple_kernel", "gnc_tuple_pairs_kernel", "gnc_diameter_kernel", "gnc_gather_kernel",
                 "gnc_loop_kernel"):
        assert sum(name in k for k in ks) == 1, name
    assert sum("scan_onepass_kernel" in k for k in ks) == 2 and sum("select_scatter_kernel" in k for k in ks) == 2  # the one compaction, for its two flags
    _assert_no_scratch(ks)
    # the two one-workgroup kernels that reduce through gp_alignment.hpp: SGPRs, VGPRs, LDS (bytes per workgroup) of the build before they did, as upper bounds
    for frag, (sgprs, vgprs, lds) in {"gnc_loop_kernel": (82, 126, 18560), "gnc_diameter_kernel": (20, 25, 12288)}.items():
        (name,) = [k for k in ks if frag in k]
        get = lambda key: int(re.search(re.escape(key) + r":\s+(\d+)", ks[name]).group(1))  # noqa: E731
        got = dict(sgprs=get("TotalSGPRs"), vgprs=get("    VGPRs"), lds=get("LDS Size [bytes/block]"))
        print(name, got)
        assert got["sgprs"] <= sgprs and got["vgprs"] <= vgprs and got["lds"] <= lds, (name, got)


def test_defaults_are_the_reference_values():
    from gtsam_points_amd import GNCParams, _capi

    p = _capi.GncParams()
    _capi.load().gp_gnc_params_default(C.byref(p))
    # registration/graduated_non_convexity.hpp:19-34
    assert (p.max_init_samples, p.reciprocal_check, p.tuple_check, p.tuple_thresh, p.max_num_tuples) == (5000, 1, 0, 0.9, 1000)
    assert (p.div_factor, p.max_corr_dist, p.inner_iterations, p.max_iterations, p.dof, p.seed) == (1.4, 0.25, 3, 64, 6, 5489)
    q = GNCParams()
    assert (q.max_init_samples, q.reciprocal_check, q.tuple_check, q.tuple_thresh, q.max_num_tuples) == (5000, True, False, 0.9, 1000)
    assert (q.div_factor, q.max_corr_dist, q.inner_iterations, q.max_iterations, q.dof, q.seed) == (1.4, 0.25, 3, 64, 6, 5489)


def test_entry_points_refuse_bad_arguments_without_a_device():
    from gtsam_points_amd import _capi

    lib = _capi.load()
    fake = C.c_void_p(64)  # never dereferenced
    res = _capi.GncResult()
    n = C.c_int(0)

    def fresh(**kw):
        p = _capi.GncParams()
        lib.gp_gnc_params_default(C.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def estimate(p, nt=10, ns=10, dim=33):
        return lib.gp_gnc_estimate_pose(fake, nt, fake, ns, fake, fake, dim, C.byref(p), None, 0, None, None, C.byref(res), None)

    def align(p, nt=10, ns=10):
        return lib.gp_gnc_align_correspondences(fake, nt, fake, ns, fake, 4, C.byref(p), None, C.byref(res), None)

    def match(p, nt=10, ns=10, dim=33):
        return lib.gp_feature_correspondences(fake, nt, fake, ns, fake, fake, dim, C.byref(p), None, 0, fake, C.byref(n), None, None, None)

    for call in (estimate, align):
        assert call(fresh(dof=5)) == 1 and b"dof" in lib.gp_last_error()
        assert call(fresh(), nt=0) == 1 and b"empty" in lib.gp_last_error()
        assert call(fresh(), ns=0) == 1 and b"empty" in lib.gp_last_error()
        assert call(fresh(div_factor=1.0)) == 1 and b"div_factor" in lib.gp_last_error()
        assert call(fresh(div_factor=float("nan"))) == 1 and b"div_factor" in lib.gp_last_error()
        assert call(fresh(max_corr_dist=0.0)) == 1 and b"max_corr_dist" in lib.gp_last_error()
        assert call(fresh(max_iterations=0)) == 1 and b"max_iterations" in lib.gp_last_error()
        assert call(fresh(inner_iterations=0)) == 1 and b"inner_iterations" in lib.gp_last_error()
    for call in (estimate, match):
        assert call(fresh(), dim=129) == 1 and b"128" in lib.gp_last_error()
        assert call(fresh(), dim=0) == 1 and b"128" in lib.gp_last_error()
        assert call(fresh(max_init_samples=0)) == 1 and b"max_init_samples" in lib.gp_last_error()
        assert call(fresh(tuple_check=1, max_num_tuples=0)) == 1 and b"max_num_tuples" in lib.gp_last_error()
    assert match(fresh(), nt=0) == 1 and b"empty" in lib.gp_last_error()
    assert lib.gp_gnc_estimate_pose(fake, 10, fake, 10, fake, fake, 33, None, None, 0, None, None, C.byref(res), None) == 1 and b"NULL" in lib.gp_last_error()
    assert lib.gp_gnc_align_correspondences(fake, 10, fake, 10, fake, -1, C.byref(fresh()), None, C.byref(res), None) == 1

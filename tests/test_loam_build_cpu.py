"""CPU checks of the LOAM factors' build products: the tile kernels' resources as the compiler reports them, the unchanged GICP / ICP kernel counts, the exports and
the argument refusals that are made on the host before any device work."""
import ctypes as C

from test_icp_build_cpu import _assert_no_scratch, _tile_kernels


def test_loam_tile_kernels_use_no_scratch():
    for term in ("LoamEdgeTerm", "LoamPlaneTerm"):
        ks = _tile_kernels(term)
        assert len(ks) == 3, term  # linearise, error, general linearise
        _assert_no_scratch(ks)
    assert len(_tile_kernels("Loam")) == 6


def test_gicp_and_icp_kernel_counts_are_unchanged():
    assert len(_tile_kernels("IcpTerm")) == 6 and len(_tile_kernels("GicpTerm")) == 3
    assert len(_tile_kernels("")) == 15  # nothing else instantiates the tile kernel


def test_loam_entry_points_refuse_bad_arguments_without_a_device():
    from gtsam_points_amd import _capi

    lib = _capi.load()
    h = C.c_void_p()
    fake = C.c_void_p(64)  # never dereferenced: every call below is refused first
    INVALID = 1  # GP_ERROR_INVALID_ARGUMENT
    assert lib.gp_loam_factor_create(None, None, 0, None, 0, None, None, 0, None, 0, None, C.byref(h)) == INVALID and not h.value  # both parts absent
    assert b"gp_loam_factor_create" in lib.gp_last_error()
    assert lib.gp_loam_factor_create(fake, None, 1, fake, 1, None, None, 0, None, 0, None, C.byref(h)) == INVALID and not h.value  # a grid but NULL target points
    assert lib.gp_loam_factor_create(fake, fake, 1, None, 1, None, None, 0, None, 0, None, C.byref(h)) == INVALID and not h.value  # ... NULL source points
    assert lib.gp_loam_factor_create(None, None, 0, None, 0, fake, None, 1, fake, 1, None, C.byref(h)) == INVALID and not h.value  # the plane part likewise
    assert lib.gp_loam_factor_create(None, fake, 1, fake, 1, None, None, 0, None, 0, None, C.byref(h)) == INVALID and not h.value  # points but no grid
    assert lib.gp_loam_factor_create(fake, fake, 1, fake, 1, None, None, 0, None, 0, None, None) == INVALID
    assert lib.gp_loam_factor_destroy(None) == 0
    assert lib.gp_loam_factor_linearize(None, None, None) == INVALID and lib.gp_loam_factor_compute_error(None, None, None, None) == INVALID
    assert lib.gp_loam_factor_set_max_correspondence_distance(None, 1.0, 1.0) == INVALID
    assert lib.gp_loam_factor_set_enable_correspondence_validation(None, 1) == INVALID
    assert lib.gp_loam_factor_set_correspondence_update_tolerance(None, 0.1, 0.1) == INVALID
    assert lib.gp_loam_factor_num_correspondences(None, None, None) == INVALID
    assert lib.gp_loam_factor_get_correspondences(None, None, None) == INVALID


def test_batch_create_ex_is_exported_and_refuses_on_the_host():
    from gtsam_points_amd import _capi

    lib = _capi.load()
    assert hasattr(lib, "gp_corr_batch_create_ex") and "gp_corr_batch_create_ex" in _capi.EXPORTED_SYMBOLS
    h = C.c_void_p()
    assert lib.gp_corr_batch_create_ex(None, 0, None, 0, None, 0, None, C.byref(h)) == 1 and not h.value  # an empty batch
    assert lib.gp_corr_batch_create_ex(None, 0, None, 0, None, 1, None, C.byref(h)) == 1 and not h.value  # a count without the array
    null = (C.c_void_p * 1)(None)
    assert lib.gp_corr_batch_create_ex(None, 0, None, 0, null, 1, None, C.byref(h)) == 1 and not h.value  # a NULL member
    assert b"gp_corr_batch_create" in lib.gp_last_error()

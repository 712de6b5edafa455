"""CPU checks of the covariance unit's build products: the kernels csrc/gp_covariance.hip emits, as the compiler's resource remarks list them (gp_covariance.resources.txt),
are exactly the set the dispatch can launch, and each stays within the registers, scratch, spills and LDS -- and at the occupancy -- of the build before the unit was split.

The bounds are the figures of that build (HIP 7.2 / AMD clang 22, gfx950): upper bounds on VGPRs, scratch (bytes per lane), VGPR spills and LDS (bytes per workgroup),
lower bounds on the occupancy (waves per SIMD).  The build this test came with sits ON every figure below: its kernels are the unsplit build's instruction for
instruction.  With eig3_direct's compile-time columns (gp_eig3.hpp) in every kernel the same compiler gives, at the same VGPRs, occupancy and LDS, less scratch
(covariance_kernel<10, 4, true> 16 B, <10, 4, false> 40 B, <32, 1, false> 424 B, covariance_far_kernel<10> 512 B with 165 / 208 spills, covariance_settle_kernel<10> and
normals_from_covs_kernel none) -- and other last bits in a few ill-conditioned covariances, so that form did not ship."""
import os
import re

from test_icp_build_cpu import ROOT

RES = os.path.join(ROOT, "gtsam_points_amd", "csrc", "gp_covariance.resources.txt")

# fragment of the mangled name (both NORMALS values where the kernel has the flag: Lb0E / Lb1E behind it) -> VGPRs, scratch, {NORMALS: spills} or None, waves, LDS or None
TEMPLATED = {
    "covariance_kernelILi10ELi4ELb1E": (127, 48, {False: 2, True: 2}, 4, 16384),   # k == 10: full lists, straight-line insertion
    "covariance_kernelILi10ELi4ELb0E": (128, 64, {False: 8, True: 8}, 4, 0),       # k < 10
    "covariance_kernelILi32ELi1ELb0E": (175, 440, {False: 0, True: 0}, 2, 0),      # 10 < k <= 32
    "covariance_far_kernelILi10E": (128, 560, {False: 169, True: 212}, 4, 6208),
    "covariance_settle_kernelILi10E": (62, 32, None, 8, None),
    "nonfinite_identity_kernelI": (None, None, None, None, None),                  # (listed: both builds exist; no figure is held)
}
PLAIN = {
    "covariance_rows_kernelE": (110, 0, None, 4, 8412),
    "normals_from_covs_kernelE": (50, 32, None, 8, None),
    "heavy_first_order_kernelE": (None, None, None, None, None),
}
HELPERS = ("scan_onepass_kernel", "host_flag_kernel")  # what gp_scan.hpp and gp_host.hpp instantiate in every unit that scans or hands a word to the host


def _remarks():
    assert os.path.exists(RES), "build the HIP library first (python -c 'import __graft_entry__ as g; g.build()')"
    return {b.split()[0]: b for b in open(RES).read().split("remark: Function Name: ")[1:]}


def _expected():
    """mangled-name fragment -> (bounds, NORMALS or None)"""
    want = {frag + ("Lb1E" if normals else "Lb0E") + "E": (bounds, normals) for frag, bounds in TEMPLATED.items() for normals in (False, True)}
    want.update({frag: (bounds, None) for frag, bounds in PLAIN.items()})
    return want


def test_the_unit_emits_exactly_the_kernels_the_dispatch_can_launch():
    ks, want = _remarks(), _expected()
    own = [k for k in ks if not any(h in k for h in HELPERS)]
    for frag in want:
        assert sum(frag in k for k in own) == 1, frag
    assert len(own) == len(want), sorted(own)  # nothing else: no covariance_kernel<10, 1, false>, no probe kernel (gp_side_stream.hip)
    assert not any("covariance_kernelILi10ELi1E" in k or "pipe_probe" in k for k in ks)


def test_every_kernel_keeps_within_the_figures_of_the_unsplit_build():
    ks = _remarks()
    for frag, ((vgprs, scratch, spills, waves, lds), normals) in _expected().items():
        (name,) = [k for k in ks if frag in k]
        get = lambda key: int(re.search(re.escape(key) + r":\s+(\d+)", ks[name]).group(1))  # noqa: E731
        got = dict(vgprs=get("    VGPRs"), scratch=get("ScratchSize [bytes/lane]"), spills=get("VGPRs Spill"), waves=get("Occupancy [waves/SIMD]"), lds=get("LDS Size [bytes/block]"))
        print(name, got)
        assert vgprs is None or got["vgprs"] <= vgprs, (name, got)
        assert scratch is None or got["scratch"] <= scratch, (name, got)
        assert spills is None or got["spills"] <= spills[normals], (name, got)
        assert waves is None or got["waves"] >= waves, (name, got)
        assert lds is None or got["lds"] <= lds, (name, got)

"""The C++ mirror (gtsam_points_amd/host/) compiled against the REFERENCE'S OWN HEADERS and driven end to end.

oracle/host/Makefile builds oracle/_ref/test_host from tests/host/test_host.cpp + gtsam_points_amd/host/gtsam_points_hip_host.cpp + the
reference's own optimizers/linearization_hook.cpp, types/offloadable.cpp and types/point_cloud.cpp (compiled from /root/reference
where they lie), with the mirror classes deriving from the reference's NonlinearFactorGPU / NonlinearFactorSet / PointCloud /
GaussianVoxelMap / OffloadableGPU.  Only Eigen / GTSAM / boost are stand-ins (oracle/ref_shim/include).  The binary is built where
the reference tree is present and travels with the rest of oracle/_ref."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "oracle", "_ref", "test_host")


@pytest.mark.gpu
def test_cpp_host_mirror_end_to_end():
    assert os.path.exists(EXE), "oracle/_ref/test_host is missing: __graft_entry__.build() makes it where the reference tree is present"
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "HOST_TEST_OK" in out.stdout, out.stdout + out.stderr


@pytest.mark.skipif(not os.path.isdir("/root/reference"), reason="the reference tree is not mounted here")
def test_cpp_host_mirror_compiles_against_the_reference_headers():
    """CPU check: the mirror compiles as subclasses of the reference's own base classes and links the C-ABI library"""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle", "host"), "-s"])
    assert os.path.exists(EXE)
    # the binary really references the reference's own out-of-line symbols (LinearizationHook, OffloadableGPU, PointCloud)
    syms = subprocess.run(["nm", "-C", EXE], capture_output=True, text=True).stdout
    for needle in ["gtsam_points::LinearizationHook::linearize", "gtsam_points::OffloadableGPU::touch", "gtsam_points::PointCloud::has_points_gpu",
                   "gtsam_points::overlap_gpu(", "gtsam_points::merge_frames_gpu("]:
        assert needle in syms, needle

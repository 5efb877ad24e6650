"""The E-step builds of the HDP machine on the workgroup-per-alignment kernels (six and eight waves per workgroup,
-DSY_HDP -DSY_ESTEP: CPECAN_FLAG_WIDE_BANDS_HDP_ESTEP on an HDP batch of expectations) keep the family's budget: nothing
in scratch, at most 128 VGPRs -- four waves per SIMD -- and a static LDS that leaves room for the workgroups that
occupancy puts on a CU.  Each has one forward, one backward and one expectation kernel and nothing else: the HDP track
kernel is cpecan_kernel_prep.hip's.  Register and memory metadata only.  CPU-only: hipcc cross-compiles gfx950."""
import os
import shutil
import subprocess

import pytest

from cpecan_load import ROOT
from test_hdp_workgroup_resources import CSRC, HIPCC, LDS_PER_CU, VGPR_BUDGET, kernel_meta


def device_asm(tmp_path, rows):
    out = str(tmp_path / ("sy_he%d.s" % rows))
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                           "-fno-fast-math", "-Wno-unused-function", "-DSY_R=%d" % rows, "-DSY_HDP", "-DSY_ESTEP",
                           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--cuda-device-only", "-o", out,
                           os.path.join(CSRC, "cpecan_kernel_systolic.hip")], stderr=subprocess.DEVNULL)
    return open(out).read()


def test_hdp_estep_objects_are_built():
    lib = os.path.join(ROOT, "cpecan-signal_amd", "libcpecan_hip.so")
    if not os.path.exists(lib):
        pytest.skip("library not built")
    for rows in (6, 8):
        assert os.path.exists(os.path.join(CSRC, "cpecan_kernel_systolic_he%d.o" % rows)), rows
    if shutil.which("nm") is None:
        pytest.skip("nm not available: the exported symbols cannot be listed")
    names = set(l.split()[-1] for l in
                subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True).splitlines())
    assert {"cpecan_systolic_build_he6", "cpecan_systolic_build_he8"} <= names
    # ... beside the posterior builds, which stay
    assert {"cpecan_systolic_build_h6", "cpecan_systolic_build_h8", "cpecan_systolic_machine_hdp"} <= names


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("rows", [6, 8])
def test_hdp_estep_builds_keep_their_budget(tmp_path, rows):
    text = device_asm(tmp_path, rows)
    meta = text[text.index("amdhsa.kernels:"):]
    assert ".name:           cpecan_k_sy_track_hdp\n" not in meta  # defined once, in cpecan_kernel_prep.hip
    assert meta.count(".name: ") == 3, "three kernels to a build"
    for stem in ("cpecan_k_sy_forward", "cpecan_k_sy_backward", "cpecan_k_sy_expect"):
        name = "%s_he%d" % (stem, rows)
        m = kernel_meta(text, name)  # (asserts that the kernel is there once)
        assert m["threads"] == 64 * rows
        assert m["vgpr"] <= VGPR_BUDGET, "%s uses %d VGPRs" % (name, m["vgpr"])
        assert m["spill"] == 0 and m["scratch"] == 0, "%s spills to scratch" % name
        # at the budget's occupancy a CU holds 16 waves: 16 / rows workgroups share its LDS
        assert m["lds"] * max(1, 16 // rows) <= LDS_PER_CU, "%s takes %d bytes of static LDS" % (name, m["lds"])

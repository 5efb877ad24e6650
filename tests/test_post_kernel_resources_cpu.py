"""The post kernel (cpecan_k_wv_post<suffix>) of every wave build of the Makefile's list, from the compiler's metadata:
it runs at a window's boundary beside the assembly sweeps' waves, so it has to fit in what they leave -- 64 registers
beside a backward wave (tests/test_kernel_resources.py), nothing in scratch, and static LDS small enough for four of its
workgroups on a CU beside four forward and four backward assembly waves.  The LDS bound comes from the sizes the
generator of the sweeps writes into cpecan_asm_gen.h, at three and at two cells per lane."""
import os
import re

import pytest

from sweep_builds import AMD, HIPCC, builds, device_asm, kernel_meta

CU_LDS = 160 * 1024
WAVE_BUILDS = [b for b in builds() if b.family == "wave"]


def lds_bound():
    header = open(os.path.join(AMD, "csrc", "cpecan_asm_gen.h")).read()
    size = lambda name: int(re.search(r"^#define %s (\d+)$" % name, header, re.M).group(1))  # noqa: E731
    sweeps = max(size("ASM_LDS_F_BYTES") + size("ASM_LDS_B_BYTES"), size("ASM2_LDS_F_BYTES") + size("ASM2_LDS_B_BYTES"))
    return (CU_LDS - 4 * sweeps) // 4


def test_the_bound_leaves_room():
    assert 0 < lds_bound() < CU_LDS // 4


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("build", WAVE_BUILDS, ids=lambda b: b.name)
def test_post_kernel_fits_beside_the_sweeps(build):
    name = "cpecan_k_wv_post" + build.suffix
    m = kernel_meta(device_asm(build), name)
    assert m["threads"] == 256, "%s: %d threads" % (name, m["threads"])
    assert m["spill"] == 0 and m["scratch"] == 0 and "scratch_" not in m["body"], "%s spills to scratch" % name
    assert m["vgpr"] <= 64, "%s uses %d VGPRs" % (name, m["vgpr"])
    assert m["lds"] <= lds_bound(), "%s takes %d bytes of static LDS (at most %d)" % (name, m["lds"], lds_bound())

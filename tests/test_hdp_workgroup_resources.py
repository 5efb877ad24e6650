"""The HDP builds of the workgroup-per-alignment kernels (six and eight waves per workgroup, -DSY_HDP:
CPECAN_FLAG_WIDE_BANDS_HDP on an HDP posterior batch) keep the strawMan builds' budget: nothing in scratch, at most 128
VGPRs -- four waves per SIMD -- and a static LDS that leaves room for the workgroups that occupancy puts on a CU.  They
have no expectation kernel.  CPU-only: hipcc cross-compiles gfx950."""
import os
import re
import shutil
import subprocess

import pytest

from cpecan_load import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "cpecan-signal_amd", "csrc")
VGPR_BUDGET = 128  # four waves per SIMD (512 / 4): the strawMan builds' own contract
LDS_PER_CU = 160 * 1024


def device_asm(tmp_path, rows):
    out = str(tmp_path / ("sy_h%d.s" % rows))
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                           "-fno-fast-math", "-Wno-unused-function", "-DSY_R=%d" % rows, "-DSY_HDP",
                           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--cuda-device-only", "-o", out,
                           os.path.join(CSRC, "cpecan_kernel_systolic.hip")], stderr=subprocess.DEVNULL)
    return open(out).read()


def kernel_meta(text, name):
    kernels = text[text.index("amdhsa.kernels:"):].split("\n  - .agpr_count")
    meta = [m for m in kernels if ".name:           %s\n" % name in m]
    assert len(meta) == 1, "%s is not in the build" % name
    get = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, meta[0]).group(1))  # noqa: E731
    body = text[text.index("\n" + name + ":"):]
    body = body[:body.index("s_endpgm")]
    return dict(vgpr=get("vgpr_count"), spill=get("vgpr_spill_count"), lds=get("group_segment_fixed_size"),
                scratch=get("private_segment_fixed_size"), threads=get("max_flat_workgroup_size"), body=body)


def test_hdp_objects_are_built():
    lib = os.path.join(ROOT, "cpecan-signal_amd", "libcpecan_hip.so")
    if not os.path.exists(lib):
        pytest.skip("library not built")
    for rows in (6, 8):
        assert os.path.exists(os.path.join(CSRC, "cpecan_kernel_systolic_h%d.o" % rows)), rows
    if shutil.which("nm") is None:
        pytest.skip("nm not available: the exported symbols cannot be listed")
    names = set(l.split()[-1] for l in
                subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True).splitlines())
    assert {"cpecan_systolic_build_h6", "cpecan_systolic_build_h8", "cpecan_systolic_machine_hdp"} <= names
    assert "cpecan_systolic_build_h4" not in names  # the HDP wave builds reach 248: no four-wave build
    header = open(os.path.join(ROOT, "include", "cpecan_hip.h")).read()
    declared = set(re.findall(r"\b(cpecan_hip_[a-z0-9_]+)\s*\(", header))
    assert set(n for n in names if n.startswith("cpecan_hip_")) == declared  # no new entry point


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("rows", [6, 8])
def test_hdp_builds_keep_their_budget(tmp_path, rows):
    text = device_asm(tmp_path, rows)
    assert "cpecan_k_sy_expect" not in text  # no E-step on these builds
    for stem in ("cpecan_k_sy_forward", "cpecan_k_sy_backward"):
        name = "%s_h%d" % (stem, rows)
        m = kernel_meta(text, name)
        assert m["threads"] == 64 * rows
        assert m["vgpr"] <= VGPR_BUDGET, "%s uses %d VGPRs" % (name, m["vgpr"])
        assert m["spill"] == 0 and m["scratch"] == 0 and "scratch_" not in m["body"], "%s spills to scratch" % name
        # at the budget's occupancy a CU holds 16 waves: 16 / rows workgroups share its LDS
        assert m["lds"] * max(1, 16 // rows) <= LDS_PER_CU, "%s takes %d bytes of static LDS" % (name, m["lds"])

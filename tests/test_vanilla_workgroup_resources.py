"""The vanilla builds of the workgroup-per-alignment kernels (four, six and eight waves per workgroup, -DSY_VANILLA:
CPECAN_FLAG_WIDE_BANDS on a vanilla posterior batch) keep their budget: nothing in scratch, at most 168 VGPRs -- three
waves per SIMD, the occupancy step DESIGN 4 records for them (an eight-wave workgroup needs two) -- and a static LDS that
leaves room for the workgroups that occupancy puts on a CU.  The six strawMan builds of the same source keep the
registers and the LDS they had.  CPU-only: hipcc cross-compiles gfx950."""
import os
import re
import shutil
import subprocess

import pytest

from cpecan_load import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "cpecan-signal_amd", "csrc")
VGPR_BUDGET = 168  # three waves per SIMD (512 / 3, in allocation blocks of 8)
LDS_PER_CU = 160 * 1024

# (VGPRs, static LDS bytes) of the strawMan builds' forward and backward kernels before the vanilla switch was added
STRAWMAN = {
    1: dict(forward=(112, 13984), backward=(125, 2720)),
    2: dict(forward=(114, 15152), backward=(127, 3888)),
    3: dict(forward=(112, 16320), backward=(125, 5056)),
    4: dict(forward=(114, 17488), backward=(127, 6224)),
    6: dict(forward=(111, 19824), backward=(127, 8560)),
    8: dict(forward=(111, 22160), backward=(127, 10896)),
}


def device_asm(tmp_path, rows, vanilla):
    out = str(tmp_path / ("sy_%s%d.s" % ("v" if vanilla else "r", rows)))
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                           "-fno-fast-math", "-Wno-unused-function", "-DSY_R=%d" % rows]
                          + (["-DSY_VANILLA"] if vanilla else [])
                          + ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--cuda-device-only", "-o", out,
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


def test_vanilla_objects_are_built():
    lib = os.path.join(ROOT, "cpecan-signal_amd", "libcpecan_hip.so")
    if not os.path.exists(lib):
        pytest.skip("library not built")
    for rows in (4, 6, 8):
        assert os.path.exists(os.path.join(CSRC, "cpecan_kernel_systolic_v%d.o" % rows)), rows
    if shutil.which("nm") is not None:
        names = set(l.split()[-1] for l in
                    subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True).splitlines())
        assert {"cpecan_systolic_build_v4", "cpecan_systolic_build_v6", "cpecan_systolic_build_v8",
                "cpecan_systolic_machine_vanilla"} <= names
        header = open(os.path.join(ROOT, "include", "cpecan_hip.h")).read()
        declared = set(re.findall(r"\b(cpecan_hip_[a-z0-9_]+)\s*\(", header))
        assert set(n for n in names if n.startswith("cpecan_hip_")) == declared  # no new entry point


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("rows", [4, 6, 8])
def test_vanilla_builds_keep_their_budget(tmp_path, rows):
    text = device_asm(tmp_path, rows, True)
    assert "cpecan_k_sy_expect" not in text  # no E-step on these builds
    for stem in ("cpecan_k_sy_forward", "cpecan_k_sy_backward"):
        name = "%s_v%d" % (stem, rows)
        m = kernel_meta(text, name)
        assert m["threads"] == 64 * rows
        assert m["vgpr"] <= VGPR_BUDGET, "%s uses %d VGPRs" % (name, m["vgpr"])
        assert m["spill"] == 0 and m["scratch"] == 0 and "scratch_" not in m["body"], "%s spills to scratch" % name
        # at the budget's occupancy a CU holds 12 waves: 12 / rows workgroups (one at least) share its LDS
        assert m["lds"] * max(1, 12 // rows) <= LDS_PER_CU, "%s takes %d bytes of static LDS" % (name, m["lds"])


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("rows", sorted(STRAWMAN))
def test_strawman_builds_are_as_before(tmp_path, rows):
    text = device_asm(tmp_path, rows, False)
    suffix = "" if rows == 4 else "_r%d" % rows
    for stem, (vgpr, lds) in STRAWMAN[rows].items():
        name = "cpecan_k_sy_%s%s" % (stem, suffix)
        m = kernel_meta(text, name)
        assert (m["vgpr"], m["lds"]) == (vgpr, lds), name
        assert m["spill"] == 0 and m["scratch"] == 0, name
    assert "cpecan_k_sy_expect" + suffix in text

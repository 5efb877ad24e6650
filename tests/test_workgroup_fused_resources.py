"""The fused E-step builds of the strawMan machine on the workgroup-per-alignment kernels (one to four waves per
workgroup, -DSY_FUSED: CPECAN_FLAG_WORKGROUP_FUSED_ESTEP on a strawMan batch of expectations) sum the expectations
inside the sweep back, so that kernel carries eight accumulators, a gap-X sum and two more fetch buffers per in-flight
diagonal: it leaves the 128 VGPRs of the other strawMan builds, on purpose, and keeps to what two waves per SIMD allow
-- at most 256 VGPRs, nothing in scratch.  Each build has one forward and one backward kernel and nothing else (no
expectation kernel); the objects carry a name outside the pattern by which test_prep_kernels_cpu counts the sweep objects
(cpecan_kernel_systolic_fused_r<n>.o), so the rule that test holds those to -- an object defines its own build's kernels
only -- is held here.  The builds these stand beside keep their registers: tests/test_kernel_resources.py and
test_vanilla_workgroup_resources.py::test_strawman_builds_are_as_before, unchanged.  CPU-only: hipcc cross-compiles
gfx950."""
import os
import re
import shutil
import subprocess

import pytest

from cpecan_load import ROOT
from test_prep_kernels_cpu import AMD, ONCE, defined
from test_vanilla_workgroup_resources import CSRC, HIPCC, LDS_PER_CU, kernel_meta

ROWS = (1, 2, 3, 4)
VGPR_BUDGET = 256  # two waves per SIMD


def object_of(rows):
    return os.path.join(CSRC, "cpecan_kernel_systolic_fused_r%d.o" % rows)


def device_asm(tmp_path, rows):
    out = str(tmp_path / ("sy_f%d.s" % rows))
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                           "-fno-fast-math", "-Wno-unused-function", "-DSY_R=%d" % rows, "-DSY_FUSED",
                           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--cuda-device-only", "-o", out,
                           os.path.join(CSRC, "cpecan_kernel_systolic.hip")], stderr=subprocess.DEVNULL)
    return open(out).read()


@pytest.fixture(scope="module")
def library():
    lib = os.path.join(AMD, "libcpecan_hip.so")
    if not os.path.exists(lib):
        pytest.skip("library not built")
    if shutil.which("nm") is None:
        pytest.skip("nm not available: the symbols cannot be listed")
    return lib


def test_fused_builds_are_exported(library):
    names = defined(library, "-D")
    assert set("cpecan_systolic_build_f%d" % r for r in ROWS) <= names
    # ... beside the builds whose place they take on request, which stay
    assert {"cpecan_systolic_build_r1", "cpecan_systolic_build_r2", "cpecan_systolic_build_r3",
            "cpecan_systolic_build", "cpecan_systolic_machine"} <= names
    header = open(os.path.join(ROOT, "include", "cpecan_hip.h")).read()
    declared = set(re.findall(r"\b(cpecan_hip_[a-z0-9_]+)\s*\(", header))
    assert set(n for n in names if n.startswith("cpecan_hip_")) == declared  # no new entry point
    assert re.search(r"#define CPECAN_FLAG_WORKGROUP_FUSED_ESTEP 2048\b", header)


def test_fused_objects_are_linked_and_define_their_own_build_only(library):
    linked = [os.path.join(AMD, o) for o in subprocess.check_output(["make", "-s", "-C", AMD, "print-objects"],
                                                                    text=True).split()]
    for rows in ROWS:
        assert object_of(rows) in linked, rows
    if not all(os.path.exists(p) for p in linked):
        pytest.skip("the library's objects are not here")
    for rows in ROWS:
        names = defined(object_of(rows))
        kernels = set(n for n in names if n.startswith("cpecan_k_"))
        assert kernels == set("cpecan_k_sy_%s_f%d" % (stem, rows) for stem in ("forward", "backward"))
        assert not set(ONCE) & names
        assert "cpecan_systolic_build_f%d" % rows in names
        # the object of the same width keeps its three kernels
        suffix = "" if rows == 4 else "_r%d" % rows
        ring = defined(os.path.join(CSRC, "cpecan_kernel_systolic%s.o" % suffix))
        assert set(n for n in ring if n.startswith("cpecan_k_")) == set(
            "cpecan_k_sy_%s%s" % (stem, suffix) for stem in ("forward", "backward", "expect"))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("rows", ROWS)
def test_fused_builds_keep_their_budget(tmp_path, rows):
    text = device_asm(tmp_path, rows)
    meta = text[text.index("amdhsa.kernels:"):]
    assert meta.count(".name: ") == 2, "two kernels to a build: no expectation kernel"
    for stem in ("cpecan_k_sy_forward", "cpecan_k_sy_backward"):
        name = "%s_f%d" % (stem, rows)
        m = kernel_meta(text, name)  # (asserts that the kernel is there once)
        assert m["threads"] == 64 * rows
        assert m["vgpr"] <= VGPR_BUDGET, "%s uses %d VGPRs" % (name, m["vgpr"])
        assert m["spill"] == 0 and m["scratch"] == 0 and "scratch_" not in m["body"], "%s spills to scratch" % name
        # at two waves per SIMD a CU holds eight waves: 8 / rows workgroups share its LDS
        assert m["lds"] * (8 // rows) <= LDS_PER_CU, "%s takes %d bytes of static LDS" % (name, m["lds"])
    # the forward sweep is the other builds' E-step forward sweep: it stays within four waves per SIMD
    assert kernel_meta(text, "cpecan_k_sy_forward_f%d" % rows)["vgpr"] <= 128

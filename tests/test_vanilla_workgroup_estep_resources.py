"""The E-step builds of the vanilla machine on the workgroup-per-alignment kernels (four, six and eight waves per
workgroup, -DSY_VANILLA -DSY_ESTEP: CPECAN_FLAG_WIDE_BANDS_VANILLA_ESTEP on a vanilla batch of expectations) keep the
vanilla builds' budget: nothing in scratch, at most 168 VGPRs -- three waves per SIMD -- and a static LDS that leaves
room for the workgroups that occupancy puts on a CU.  Each has one forward, one backward and one expectation kernel and
nothing else: the vanilla track kernel is cpecan_kernel_prep.hip's.  Their objects carry a name outside the pattern by
which test_prep_kernels_cpu counts the sweep objects (cpecan_kernel_systolic_estep_v<n>.o), so the rule that test holds
those to -- an object defines its own build's kernels only -- is held here.  Register and memory metadata and symbol
tables only.  CPU-only: hipcc cross-compiles gfx950."""
import os
import re
import shutil
import subprocess

import pytest

from cpecan_load import ROOT
from test_prep_kernels_cpu import AMD, ONCE, defined
from test_vanilla_workgroup_resources import CSRC, HIPCC, LDS_PER_CU, VGPR_BUDGET, kernel_meta

ROWS = (4, 6, 8)


def object_of(rows):
    return os.path.join(CSRC, "cpecan_kernel_systolic_estep_v%d.o" % rows)


def device_asm(tmp_path, rows):
    out = str(tmp_path / ("sy_ve%d.s" % rows))
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                           "-fno-fast-math", "-Wno-unused-function", "-DSY_R=%d" % rows, "-DSY_VANILLA", "-DSY_ESTEP",
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


def test_vanilla_estep_builds_are_exported(library):
    names = defined(library, "-D")
    assert {"cpecan_systolic_build_ve4", "cpecan_systolic_build_ve6", "cpecan_systolic_build_ve8"} <= names
    # ... beside the posterior builds, which stay
    assert {"cpecan_systolic_build_v4", "cpecan_systolic_build_v6", "cpecan_systolic_build_v8",
            "cpecan_systolic_machine_vanilla"} <= names
    header = open(os.path.join(ROOT, "include", "cpecan_hip.h")).read()
    declared = set(re.findall(r"\b(cpecan_hip_[a-z0-9_]+)\s*\(", header))
    assert set(n for n in names if n.startswith("cpecan_hip_")) == declared  # no new entry point


def test_vanilla_estep_objects_are_linked_and_define_their_own_build_only(library):
    linked = [os.path.join(AMD, o) for o in subprocess.check_output(["make", "-s", "-C", AMD, "print-objects"],
                                                                    text=True).split()]
    for rows in ROWS:
        assert object_of(rows) in linked, rows
    if not all(os.path.exists(p) for p in linked):
        pytest.skip("the library's objects are not here")
    for rows in ROWS:
        names = defined(object_of(rows))
        kernels = set(n for n in names if n.startswith("cpecan_k_"))
        assert kernels == set("cpecan_k_sy_%s_ve%d" % (stem, rows) for stem in ("forward", "backward", "expect"))
        assert not kernels & set(ONCE) and not set(ONCE) & names
        assert "cpecan_systolic_build_ve%d" % rows in names
        # the posterior object of the same width keeps its two kernels
        posterior = defined(os.path.join(CSRC, "cpecan_kernel_systolic_v%d.o" % rows))
        assert set(n for n in posterior if n.startswith("cpecan_k_")) == {"cpecan_k_sy_forward_v%d" % rows,
                                                                         "cpecan_k_sy_backward_v%d" % rows}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("rows", ROWS)
def test_vanilla_estep_builds_keep_their_budget(tmp_path, rows):
    text = device_asm(tmp_path, rows)
    meta = text[text.index("amdhsa.kernels:"):]
    assert ".name:           cpecan_k_wv_track_vanilla\n" not in meta  # defined once, in cpecan_kernel_prep.hip
    assert meta.count(".name: ") == 3, "three kernels to a build"
    for stem in ("cpecan_k_sy_forward", "cpecan_k_sy_backward", "cpecan_k_sy_expect"):
        name = "%s_ve%d" % (stem, rows)
        m = kernel_meta(text, name)  # (asserts that the kernel is there once)
        assert m["threads"] == 64 * rows
        assert m["vgpr"] <= VGPR_BUDGET, "%s uses %d VGPRs" % (name, m["vgpr"])
        assert m["spill"] == 0 and m["scratch"] == 0 and "scratch_" not in m["body"], "%s spills to scratch" % name
        # at the budget's occupancy a CU holds 12 waves: 12 / rows workgroups (one at least) share its LDS
        assert m["lds"] * max(1, 12 // rows) <= LDS_PER_CU, "%s takes %d bytes of static LDS" % (name, m["lds"])

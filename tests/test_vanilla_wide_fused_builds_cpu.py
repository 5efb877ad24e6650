"""The vanilla machine's three fused builds of the workgroup file (vf4, vf6, vf8: the E-step summed inside the sweep back,
CPECAN_FLAG_WIDE_BANDS_VANILLA_FUSED_ESTEP) from the compiler's metadata.  The Makefile lists them apart from SY_BUILDS
(SY_FUSED_BUILDS, make print-fused-builds, objects cpecan_kernel_systolicfx_vf<n>.o: see the note there), so the table
of tests/test_sweep_build_resources.py and the object walk of tests/test_prep_kernels_cpu.py do not reach them; this
file asks of them what those two ask of a build: each object has exactly its two kernels and no expectation kernel,
defines nothing that is compiled once elsewhere, nothing spills or touches scratch, the static LDS keeps the _ve builds'
rule, and the forward sweep is the _ve build's of as many waves -- the same registers and static LDS.

The register line of the sweep back is 168 for all three: three waves per SIMD (512 / 3, in allocation blocks of 8).  The
compiler lands on 144 / 141 / 145 for four / six / eight waves, against 126 / 124 / 128 of the _ve sweep back: the four
F.gapX in flight, the two sums, their column and the record addresses are registers the 128 of the next step do not have
(held there the sweep spills twelve to fourteen), so the line is the step the builds are on; what crosses it
halves the workgroups a CU holds at six waves.
The library exports the three records under a name of their own and no entry point beside those the header declares.
CPU-only: hipcc cross-compiles gfx950."""
import os
import re
import shutil

import pytest

from cpecan_load import ROOT
from sweep_builds import AMD, HIPCC, Build, builds, defined, device_asm, kernel_meta, kernel_names, make_print
from test_sweep_build_resources import shares_cu

needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
KERNELS = ("forward", "backward")
EXPECTED = dict(("vf%d" % n, ("-DSY_R=%d" % n, "-DSY_VANILLA", "-DSY_FUSED")) for n in (4, 6, 8))
BACKWARD_VGPRS = {"vf4": 168, "vf6": 168, "vf8": 168}  # three waves per SIMD


def fused_builds():
    found = {}
    for line in make_print("print-fused-builds").splitlines():
        name, obj, src, defines = line.split("\t")
        assert src == "csrc/cpecan_kernel_systolic.hip"
        found[name] = Build(name, name[:-1], int(name[-1]), "_" + name, "systolic", os.path.join(AMD, obj),
                            os.path.join(AMD, src), tuple(defines.split()))
    return found


def test_the_three_builds_are_listed_apart_with_their_defines():
    found = fused_builds()
    assert sorted(found) == sorted(EXPECTED)
    for name, b in found.items():
        assert b.defines == EXPECTED[name] and b.tag == "vf" and b.rows == int(name[2])
        assert b.obj.endswith("csrc/cpecan_kernel_systolicfx_%s.o" % name)
    listed = set(b.name for b in builds())
    assert not listed & set(found)               # not in print-builds ...
    assert {"ve4", "ve6", "ve8"} <= listed       # ... where the builds they stand in for are
    objects = make_print("print-objects").split()
    for name in EXPECTED:                        # the library links them
        assert "csrc/cpecan_kernel_systolicfx_%s.o" % name in objects


@needs_hipcc
@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_a_build_holds_its_two_kernels_within_its_budget(name):
    b = fused_builds()[name]
    text = device_asm(b)
    assert kernel_names(text) == set("cpecan_k_sy_%s%s" % (s, b.suffix) for s in KERNELS)
    assert "cpecan_k_sy_expect" not in text
    lds_fits = shares_cu(12)
    for s in KERNELS:
        m = kernel_meta(text, "cpecan_k_sy_%s%s" % (s, b.suffix))
        print("%s%s: %d VGPRs, %d SGPRs, %d bytes of LDS" % (s, b.suffix, m["vgpr"], m["sgpr"], m["lds"]))
        assert m["threads"] == 64 * b.rows
        assert m["spill"] == 0 and m["scratch"] == 0 and "scratch_" not in m["body"], "%s%s spills" % (s, b.suffix)
        assert m["vgpr"] <= 256, "%s%s uses %d VGPRs" % (s, b.suffix, m["vgpr"])
        assert lds_fits(m["lds"], b.rows), "%s%s takes %d bytes of static LDS" % (s, b.suffix, m["lds"])
    back = kernel_meta(text, "cpecan_k_sy_backward" + b.suffix)
    assert back["vgpr"] <= BACKWARD_VGPRS[name], "backward%s uses %d VGPRs" % (b.suffix, back["vgpr"])


@needs_hipcc
@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_the_forward_sweep_is_the_ring_builds(name):
    """the fused build's forward sweep is the one of the build it stands in for: the same registers and static LDS"""
    b = fused_builds()[name]
    ring = dict((x.name, x) for x in builds())["ve%d" % b.rows]
    mine = kernel_meta(device_asm(b), "cpecan_k_sy_forward" + b.suffix)
    theirs = kernel_meta(device_asm(ring), "cpecan_k_sy_forward" + ring.suffix)
    print("forward%s: (%d, %d, %d); forward%s: (%d, %d, %d)" % (
        b.suffix, mine["vgpr"], mine["sgpr"], mine["lds"], ring.suffix, theirs["vgpr"], theirs["sgpr"], theirs["lds"]))
    assert (mine["vgpr"], mine["sgpr"], mine["lds"]) == (theirs["vgpr"], theirs["sgpr"], theirs["lds"])
    back = kernel_meta(device_asm(b), "cpecan_k_sy_backward" + b.suffix)
    ringback = kernel_meta(device_asm(ring), "cpecan_k_sy_backward" + ring.suffix)
    print("backward%s: %d VGPRs, %d bytes of LDS; backward%s: %d, %d" % (
        b.suffix, back["vgpr"], back["lds"], ring.suffix, ringback["vgpr"], ringback["lds"]))
    assert back["lds"] == ringback["lds"]  # the 60 bins live in LDS the E-step builds had and did not use


def test_an_object_defines_its_own_build_only():
    """as tests/test_prep_kernels_cpu.py asks of the listed builds: the object's kernels are the build's two, every one
    with the build's suffix, none of the kernels compiled once in cpecan_kernel_prep.hip, and the build's one record"""
    from test_prep_kernels_cpu import ONCE
    if shutil.which("nm") is None:
        pytest.skip("nm not available: the symbols cannot be listed")
    for name, b in fused_builds().items():
        if not os.path.exists(b.obj):
            pytest.skip("the library's objects are not here")
        names = defined(b.obj)
        kernels = set(n for n in names if n.startswith("cpecan_k_"))
        assert kernels == set("cpecan_k_sy_%s%s" % (s, b.suffix) for s in KERNELS), name
        assert not set(ONCE) & names
        assert set(n for n in names if "_build" in n and n.startswith("cpecan_")) == {"cpecan_systolicfx_build" + b.suffix}


def test_the_library_exports_the_three_records_and_no_new_entry_point():
    lib = os.path.join(AMD, "libcpecan_hip.so")
    if not os.path.exists(lib):
        pytest.skip("library not built")
    if shutil.which("nm") is None:
        pytest.skip("nm not available: the exported symbols cannot be listed")
    names = defined(lib, "-D")
    assert set(n for n in names if n.startswith("cpecan_systolicfx_build")) == set(
        "cpecan_systolicfx_build_vf%d" % n for n in (4, 6, 8))
    assert not any(re.match(r"cpecan_systolic_build_vf", n) for n in names)
    header = open(os.path.join(ROOT, "include", "cpecan_hip.h")).read()
    declared = set(re.findall(r"\b(cpecan_hip_[a-z0-9_]+)\s*\(", header))
    assert set(n for n in names if n.startswith("cpecan_hip_")) == declared

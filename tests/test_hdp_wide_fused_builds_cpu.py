"""The HDP machine's two fused builds of the workgroup file (hf6, hf8: the E-step summed inside the sweep back,
CPECAN_FLAG_WIDE_BANDS_HDP_FUSED_ESTEP) from the compiler's metadata.  The Makefile lists them apart from SY_BUILDS, from
SY_FUSED_BUILDS and from WV_HDP_FUSED_BUILDS (SY_HDP_FUSED_BUILDS, make print-hdp-wide-fused-builds, objects
cpecan_kernel_hdpwfx_hf<n>.o: see the note there), so the table of tests/test_sweep_build_resources.py and the object
walk of tests/test_prep_kernels_cpu.py do not reach them; this file asks of them what those two ask of a build: each
object has exactly its two kernels and no expectation kernel, defines nothing that is compiled once elsewhere, nothing
spills or touches scratch, the static LDS lets the workgroups per CU of the _he build of as many waves stay, and the
forward sweep is that _he build's -- the same registers and static LDS.

The register line of the sweep back is the occupancy step each build is documented to run at (the
note beside SY_BACKWARD_ATTR): 168 for hf6, three waves per SIMD (512 / 3 in allocation blocks of 8; the compiler lands
on 164 with the eight sums in LDS and the occupancy forced, two six-wave workgroups to a CU as on _he6), 256 for hf8, two
waves per SIMD (178 by itself, one eight-wave workgroup to a CU where _he8's 121 have two).
The library exports the two records under a name of their own and no entry point beside those the header declares.
CPU-only: hipcc cross-compiles gfx950."""
import os
import re
import shutil

import pytest

from cpecan_load import ROOT
from sweep_builds import AMD, HIPCC, Build, builds, defined, device_asm, kernel_meta, kernel_names, make_print
from test_sweep_build_resources import LDS_PER_CU, shares_cu

needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
KERNELS = ("forward", "backward")
EXPECTED = dict(("hf%d" % n, ("-DSY_R=%d" % n, "-DSY_HDP", "-DSY_FUSED")) for n in (6, 8))
BACKWARD_VGPRS = {"hf6": 168, "hf8": 256}  # three waves per SIMD, two waves per SIMD
TARGET = "print-hdp-wide-fused-builds"


def fused_builds():
    found = {}
    for line in make_print(TARGET).splitlines():
        name, obj, src, defines = line.split("\t")
        assert src == "csrc/cpecan_kernel_systolic.hip"
        found[name] = Build(name, name[:-1], int(name[-1]), "_" + name, "systolic", os.path.join(AMD, obj),
                            os.path.join(AMD, src), tuple(defines.split()))
    return found


def waves_per_cu(vgprs):
    """waves a CU holds of a kernel with that many registers: four SIMDs of 512, allocated in blocks of 8, eight waves at
    the most"""
    return 4 * min(8, 512 // ((vgprs + 7) // 8 * 8))


def test_the_two_builds_are_listed_apart_with_their_defines():
    found = fused_builds()
    assert sorted(found) == sorted(EXPECTED)
    for name, b in found.items():
        assert b.defines == EXPECTED[name] and b.tag == "hf" and b.rows == int(name[2])
        assert b.obj.endswith("csrc/cpecan_kernel_hdpwfx_%s.o" % name)
        assert not re.search(r"cpecan_kernel_(systolic|wave)_[a-z]+\d\.o", b.obj)
    listed = set(b.name for b in builds())
    assert not listed & set(found)               # not in print-builds ...
    assert {"he6", "he8"} <= listed              # ... where the builds they stand in for are
    for other in ("print-fused-builds", "print-hdp-fused-builds"):   # ... nor on the other two lists of fused builds
        assert not set(found) & set(l.split("\t")[0] for l in make_print(other).splitlines()), other
    assert [l.split("\t")[0] for l in make_print("print-fused-builds").splitlines()] == ["vf4", "vf6", "vf8"]
    assert [l.split("\t")[0] for l in make_print("print-hdp-fused-builds").splitlines()] == ["hf2", "hf3"]
    objects = make_print("print-objects").split()
    for name in EXPECTED:                        # the library links them
        assert "csrc/cpecan_kernel_hdpwfx_%s.o" % name in objects
    tool = open(os.path.join(ROOT, "tools", "kernel_diff.py")).read()
    assert TARGET in tool                        # the kernel diff compiles them too


@needs_hipcc
@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_a_build_holds_its_two_kernels_within_its_budget(name):
    b = fused_builds()[name]
    ring = dict((x.name, x) for x in builds())["he%d" % b.rows]
    text, ringtext = device_asm(b), device_asm(ring)
    assert kernel_names(text) == set("cpecan_k_sy_%s%s" % (s, b.suffix) for s in KERNELS)
    assert "cpecan_k_sy_expect" not in text
    for s in KERNELS:
        m = kernel_meta(text, "cpecan_k_sy_%s%s" % (s, b.suffix))
        r = kernel_meta(ringtext, "cpecan_k_sy_%s%s" % (s, ring.suffix))
        groups = max(1, waves_per_cu(r["vgpr"]) // b.rows)   # the workgroups per CU the _he kernel gets
        print("%s%s: %d VGPRs, %d SGPRs, %d bytes of LDS; %s%s: %d VGPRs, %d workgroups to a CU" % (
            s, b.suffix, m["vgpr"], m["sgpr"], m["lds"], s, ring.suffix, r["vgpr"], groups))
        assert m["threads"] == 64 * b.rows
        assert m["spill"] == 0 and m["scratch"] == 0 and "scratch_" not in m["body"], "%s%s spills" % (s, b.suffix)
        assert m["vgpr"] <= 256, "%s%s uses %d VGPRs" % (s, b.suffix, m["vgpr"])
        assert shares_cu(groups * b.rows)(m["lds"], b.rows) and m["lds"] * groups <= LDS_PER_CU, \
            "%s%s takes %d bytes of static LDS" % (s, b.suffix, m["lds"])
    back = kernel_meta(text, "cpecan_k_sy_backward" + b.suffix)
    assert back["vgpr"] <= BACKWARD_VGPRS[name], "backward%s uses %d VGPRs" % (b.suffix, back["vgpr"])
    if name == "hf6":   # the step it is on keeps the two workgroups of _he6 on a CU
        assert waves_per_cu(back["vgpr"]) // b.rows == 2


@needs_hipcc
@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_the_forward_sweep_is_the_ring_builds(name):
    """the fused build's forward sweep is the one of the build it stands in for: the same registers and static LDS"""
    b = fused_builds()[name]
    ring = dict((x.name, x) for x in builds())["he%d" % b.rows]
    mine = kernel_meta(device_asm(b), "cpecan_k_sy_forward" + b.suffix)
    theirs = kernel_meta(device_asm(ring), "cpecan_k_sy_forward" + ring.suffix)
    print("forward%s: (%d, %d, %d); forward%s: (%d, %d, %d)" % (
        b.suffix, mine["vgpr"], mine["sgpr"], mine["lds"], ring.suffix, theirs["vgpr"], theirs["sgpr"], theirs["lds"]))
    assert (mine["vgpr"], mine["sgpr"], mine["lds"]) == (theirs["vgpr"], theirs["sgpr"], theirs["lds"])


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
        assert set(n for n in names if "_build" in n and n.startswith("cpecan_")) == {"cpecan_hdpwfx_build" + b.suffix}


def test_the_library_exports_the_two_records_and_no_new_entry_point():
    lib = os.path.join(AMD, "libcpecan_hip.so")
    if not os.path.exists(lib):
        pytest.skip("library not built")
    if shutil.which("nm") is None:
        pytest.skip("nm not available: the exported symbols cannot be listed")
    names = defined(lib, "-D")
    assert set(n for n in names if n.startswith("cpecan_hdpwfx_build")) == set(
        "cpecan_hdpwfx_build_hf%d" % n for n in (6, 8))
    for prefix in ("cpecan_systolic_build", "cpecan_systolicfx_build", "cpecan_hdpfx_build", "cpecan_wave"):
        assert not any(re.match(prefix + r"\w*_hf[68]$", n) for n in names), prefix
    header = open(os.path.join(ROOT, "include", "cpecan_hip.h")).read()
    declared = set(re.findall(r"\b(cpecan_hip_[a-z0-9_]+)\s*\(", header))
    assert set(n for n in names if n.startswith("cpecan_hip_")) == declared

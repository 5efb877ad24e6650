"""The HDP machine's fused build of the wave file at four cells per lane (hf4: the E-step summed inside the sweep back,
CPECAN_FLAG_HDP_FOUR_CELLS_FUSED_ESTEP, bands of 185..248 k-mers) from the compiler's metadata.  The Makefile lists it
apart from WV_BUILDS and from WV_HDP_FUSED_BUILDS (WV_HDP_FUSED4_BUILDS, make print-hdp-four-cells-fused-builds, object
cpecan_kernel_hdpfx_hf4.o: see the note there), so neither the table of tests/test_sweep_build_resources.py nor
tests/test_hdp_fused_builds_cpu.py reaches it; this file asks of it what those ask of a build: the object has exactly
its seven kernels -- the forward sweep, the fused sweep back and the fused re-sweep, each with and without the gap Y ->
gap X term, and the post kernel -- and no ring sweep back, posterior re-sweep or expectation kernel, nothing spills or
touches scratch, and the forward sweeps and the post kernel's LDS are the _h4 build's.

The other counts are literals of the build as the compiler of this tree makes it.  At four cells a
forward wave (232 registers in blocks of 8; 248 with the gap Y -> gap X switch) and a fused backward wave (432; 448) do
not share a SIMD's 512 registers.  The ring build's pair does without the switch (232 + 272 = 504) and does not with
it (248 + 288 = 536): the figures the measurement of round 28 is read against."""
import os
import re
import shutil

import pytest

from cpecan_load import ROOT
from sweep_builds import AMD, HIPCC, Build, builds, defined, device_asm, kernel_meta, kernel_names, make_print

needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
KERNELS = ("forward", "forward_sw", "backward_fx", "backward_fx_sw", "resweep_fx", "resweep_fx_sw", "post")
EXPECTED = {"hf4": ("-DWV_L=4", "-DWV_HDP", "-DWV_FUSED")}
# registers (arch + acc) and static LDS per kernel
COUNTS = {
    "forward": (230, 16096), "forward_sw": (248, 16096),
    "backward_fx": (428, 8736), "backward_fx_sw": (448, 8736),
    "resweep_fx": (456, 8736), "resweep_fx_sw": (452, 8736),
    "post": (57, 11808),
}
# ... and of the ring build's sweep back, which parks the backward cells for cpecan_k_wv_expect_h4
RING_COUNTS = {"backward_em": (266, 8736), "backward_em_sw": (286, 8736)}
# forward + sweep back on one SIMD, each in allocation blocks of 8: (ring pair, fused pair), of 512
PAIRS = {"": (232 + 272, 232 + 432), "_sw": (248 + 288, 248 + 448)}


def fused_builds():
    found = {}
    for line in make_print("print-hdp-four-cells-fused-builds").splitlines():
        name, obj, src, defines = line.split("\t")
        assert src == "csrc/cpecan_kernel_wave.hip"
        found[name] = Build(name, name[:-1], int(name[-1]), "_" + name, "wave", os.path.join(AMD, obj),
                            os.path.join(AMD, src), tuple(defines.split()))
    return found


def ring_build():
    return dict((x.name, x) for x in builds())["h4"]


def block8(n):
    return (n + 7) // 8 * 8


def test_the_build_is_listed_apart_with_its_defines():
    found = fused_builds()
    assert sorted(found) == ["hf4"]
    b = found["hf4"]
    assert b.defines == EXPECTED["hf4"] and b.tag == "hf" and b.rows == 4
    assert b.obj.endswith("csrc/cpecan_kernel_hdpfx_hf4.o")
    listed = set(x.name for x in builds())
    assert "hf4" not in listed and "h4" in listed     # not in print-builds, where the build it stands in for is
    for target in ("print-fused-builds", "print-hdp-fused-builds", "print-hdp-wide-fused-builds"):
        assert "hf4" not in set(l.split("\t")[0] for l in make_print(target).splitlines()), target
    assert "csrc/cpecan_kernel_hdpfx_hf4.o" in make_print("print-objects").split()   # the library links it


@needs_hipcc
def test_the_build_holds_its_seven_kernels_and_none_spills():
    b = fused_builds()["hf4"]
    text = device_asm(b)
    assert kernel_names(text) == set("cpecan_k_wv_%s%s" % (s, b.suffix) for s in KERNELS)
    assert "cpecan_k_wv_expect" not in text and "cpecan_k_wv_backward_em" not in text   # no ring, no expectation kernel
    for s in KERNELS:
        m = kernel_meta(text, "cpecan_k_wv_%s%s" % (s, b.suffix))
        print("%s%s: %d VGPRs, %d SGPRs, %d bytes of LDS" % (s, b.suffix, m["vgpr"], m["sgpr"], m["lds"]))
        assert m["threads"] == (256 if s == "post" else 64)
        assert m["spill"] == 0 and m["scratch"] == 0 and "scratch_" not in m["body"], "%s%s spills" % (s, b.suffix)
        assert m["vgpr"] <= 512, "%s%s uses %d VGPRs" % (s, b.suffix, m["vgpr"])
        assert (m["vgpr"], m["lds"]) == COUNTS[s], s
    assert kernel_meta(text, "cpecan_k_wv_post" + b.suffix)["vgpr"] <= 64   # eight waves per SIMD, as the ring builds'


@needs_hipcc
def test_the_forward_sweeps_and_the_post_kernels_lds_are_the_ring_builds():
    b, ring = fused_builds()["hf4"], ring_build()
    for s in ("forward", "forward_sw"):
        mine = kernel_meta(device_asm(b), "cpecan_k_wv_%s%s" % (s, b.suffix))
        theirs = kernel_meta(device_asm(ring), "cpecan_k_wv_%s%s" % (s, ring.suffix))
        print("%s%s: (%d, %d, %d); %s%s: (%d, %d, %d)" % (s, b.suffix, mine["vgpr"], mine["sgpr"], mine["lds"], s,
                                                           ring.suffix, theirs["vgpr"], theirs["sgpr"], theirs["lds"]))
        assert (mine["vgpr"], mine["sgpr"], mine["lds"]) == (theirs["vgpr"], theirs["sgpr"], theirs["lds"])
    mine = kernel_meta(device_asm(b), "cpecan_k_wv_post" + b.suffix)
    theirs = kernel_meta(device_asm(ring), "cpecan_k_wv_post" + ring.suffix)
    assert mine["lds"] == theirs["lds"] and theirs["vgpr"] <= 64


@needs_hipcc
def test_the_ring_builds_sweep_back_and_who_shares_a_simd():
    """what the ring build reports for backward_em, and the forward + backward sums in allocation blocks of 8: the ring
    build's pair fits a SIMD's 512 registers on the kernels without the switch and misses them with it; the fused
    build's pair fits on neither, which is what the measurement of round 28 is read against"""
    b, ring = fused_builds()["hf4"], ring_build()
    for s, want in RING_COUNTS.items():
        m = kernel_meta(device_asm(ring), "cpecan_k_wv_%s%s" % (s, ring.suffix))
        print("%s%s: %d VGPRs, %d bytes of LDS" % (s, ring.suffix, m["vgpr"], m["lds"]))
        assert m["spill"] == 0 and m["scratch"] == 0
        assert (m["vgpr"], m["lds"]) == want, s
    for sw in ("", "_sw"):
        f = kernel_meta(device_asm(ring), "cpecan_k_wv_forward%s%s" % (sw, ring.suffix))["vgpr"]
        r = kernel_meta(device_asm(ring), "cpecan_k_wv_backward_em%s%s" % (sw, ring.suffix))["vgpr"]
        k = kernel_meta(device_asm(b), "cpecan_k_wv_backward_fx%s%s" % (sw, b.suffix))["vgpr"]
        print("forward%s %d + backward_em%s %d -> %d; + backward_fx%s %d -> %d of 512"
              % (sw, f, sw, r, block8(f) + block8(r), sw, k, block8(f) + block8(k)))
        assert (block8(f) + block8(r), block8(f) + block8(k)) == PAIRS[sw], sw
    assert PAIRS[""][0] <= 512 < PAIRS["_sw"][0] and min(PAIRS[""][1], PAIRS["_sw"][1]) > 512


def test_the_object_defines_its_own_build_only():
    """as tests/test_prep_kernels_cpu.py asks of the listed builds: the object's kernels are the build's seven, every one
    with the build's suffix, none of the kernels compiled once in cpecan_kernel_prep.hip, and exactly one record"""
    from test_prep_kernels_cpu import ONCE
    if shutil.which("nm") is None:
        pytest.skip("nm not available: the symbols cannot be listed")
    b = fused_builds()["hf4"]
    if not os.path.exists(b.obj):
        pytest.skip("the library's objects are not here")
    names = defined(b.obj)
    kernels = set(n for n in names if n.startswith("cpecan_k_"))
    assert kernels == set("cpecan_k_wv_%s%s" % (s, b.suffix) for s in KERNELS)
    assert not set(ONCE) & names
    assert set(n for n in names if re.match(r"cpecan_\w*_build", n)) == {"cpecan_hdpfx_build_hf4"}


def test_the_library_has_the_kernels_and_no_new_entry_point():
    """the library links the object (its kernels' host stubs are there) and exports no entry point beside those the header
    declares; the record is the dispatch table's alone and no dynamic symbol"""
    lib = os.path.join(AMD, "libcpecan_hip.so")
    if not os.path.exists(lib):
        pytest.skip("library not built")
    if shutil.which("nm") is None:
        pytest.skip("nm not available: the symbols cannot be listed")
    every = defined(lib)
    assert set("cpecan_k_wv_%s_hf4" % s for s in KERNELS) <= every
    assert "cpecan_hdpfx_build_hf4" in every
    names = defined(lib, "-D")
    assert "cpecan_hdpfx_build_hf4" not in names
    header = open(os.path.join(ROOT, "include", "cpecan_hip.h")).read()
    declared = set(re.findall(r"\b(cpecan_hip_[a-z0-9_]+)\s*\(", header))
    assert set(n for n in names if n.startswith("cpecan_hip_")) == declared

"""The HDP machine's two fused builds of the wave file (hf2, hf3: the E-step summed inside the sweep back,
CPECAN_FLAG_HDP_FUSED_ESTEP) from the compiler's metadata.  The Makefile lists them apart from WV_BUILDS
(WV_HDP_FUSED_BUILDS, make print-hdp-fused-builds, objects cpecan_kernel_hdpfx_hf<n>.o: see the note there), so the
table of tests/test_sweep_build_resources.py and the object walk of tests/test_prep_kernels_cpu.py do not reach them;
this file asks of them what those two ask of a build: each object has exactly its seven kernels -- the forward sweep, the
fused sweep back and the fused re-sweep, each with and without the gap Y -> gap X term, and the post kernel -- and no
ring sweep back, posterior re-sweep or expectation kernel, nothing spills or touches scratch, and the forward sweeps are
the _h2 / _h3 builds': the same registers and static LDS.

At two cells per lane a forward wave and a fused backward wave of the next window share a SIMD, as the ring builds' do:
their register counts, each rounded up to the allocation block of 8, sum to at most 512.  At three cells only the
absence of spills is asked.  The test prints the counts.
The library exports the two records under a name of their own and no entry point beside those the header declares.
CPU-only: hipcc cross-compiles gfx950."""
import os
import re
import shutil

import pytest

from cpecan_load import ROOT
from sweep_builds import AMD, HIPCC, Build, builds, defined, device_asm, kernel_meta, kernel_names, make_print

needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
KERNELS = ("forward", "forward_sw", "backward_fx", "backward_fx_sw", "resweep_fx", "resweep_fx_sw", "post")
EXPECTED = dict(("hf%d" % n, ("-DWV_L=%d" % n, "-DWV_HDP", "-DWV_FUSED")) for n in (2, 3))


def fused_builds():
    found = {}
    for line in make_print("print-hdp-fused-builds").splitlines():
        name, obj, src, defines = line.split("\t")
        assert src == "csrc/cpecan_kernel_wave.hip"
        found[name] = Build(name, name[:-1], int(name[-1]), "_" + name, "wave", os.path.join(AMD, obj),
                            os.path.join(AMD, src), tuple(defines.split()))
    return found


def block8(n):
    return (n + 7) // 8 * 8


def test_the_two_builds_are_listed_apart_with_their_defines():
    found = fused_builds()
    assert sorted(found) == sorted(EXPECTED)
    for name, b in found.items():
        assert b.defines == EXPECTED[name] and b.tag == "hf" and b.rows == int(name[2])
        assert b.obj.endswith("csrc/cpecan_kernel_hdpfx_%s.o" % name)
        assert not re.search(r"cpecan_kernel_(systolic|wave)_[a-z]+\d\.o", b.obj)
    listed = set(b.name for b in builds())
    assert not listed & set(found)               # not in print-builds ...
    assert {"h2", "h3"} <= listed                # ... where the builds they stand in for are
    assert not set(found) & set(l.split("\t")[0] for l in make_print("print-fused-builds").splitlines())
    objects = make_print("print-objects").split()
    for name in EXPECTED:                        # the library links them
        assert "csrc/cpecan_kernel_hdpfx_%s.o" % name in objects


@needs_hipcc
@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_a_build_holds_its_seven_kernels_and_none_spills(name):
    b = fused_builds()[name]
    text = device_asm(b)
    assert kernel_names(text) == set("cpecan_k_wv_%s%s" % (s, b.suffix) for s in KERNELS)
    assert "cpecan_k_wv_expect" not in text and "cpecan_k_wv_backward_em" not in text   # no ring, no expectation kernel
    for s in KERNELS:
        m = kernel_meta(text, "cpecan_k_wv_%s%s" % (s, b.suffix))
        print("%s%s: %d VGPRs, %d SGPRs, %d bytes of LDS" % (s, b.suffix, m["vgpr"], m["sgpr"], m["lds"]))
        assert m["threads"] == (256 if s == "post" else 64)
        assert m["spill"] == 0 and m["scratch"] == 0 and "scratch_" not in m["body"], "%s%s spills" % (s, b.suffix)
        assert m["vgpr"] <= 512, "%s%s uses %d VGPRs" % (s, b.suffix, m["vgpr"])
    assert kernel_meta(text, "cpecan_k_wv_post" + b.suffix)["vgpr"] <= 64   # eight waves per SIMD, as the ring builds'


@needs_hipcc
@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_the_forward_sweeps_are_the_ring_builds(name):
    """the fused build's forward sweeps are those of the build it stands in for: the same registers and static LDS"""
    b = fused_builds()[name]
    ring = dict((x.name, x) for x in builds())["h%d" % b.rows]
    for s in ("forward", "forward_sw"):
        mine = kernel_meta(device_asm(b), "cpecan_k_wv_%s%s" % (s, b.suffix))
        theirs = kernel_meta(device_asm(ring), "cpecan_k_wv_%s%s" % (s, ring.suffix))
        print("%s%s: (%d, %d, %d); %s%s: (%d, %d, %d)" % (s, b.suffix, mine["vgpr"], mine["sgpr"], mine["lds"], s,
                                                           ring.suffix, theirs["vgpr"], theirs["sgpr"], theirs["lds"]))
        assert (mine["vgpr"], mine["sgpr"], mine["lds"]) == (theirs["vgpr"], theirs["sgpr"], theirs["lds"])
    for s, r in (("backward_fx", "backward_em"), ("backward_fx_sw", "backward_em_sw")):
        mine = kernel_meta(device_asm(b), "cpecan_k_wv_%s%s" % (s, b.suffix))
        theirs = kernel_meta(device_asm(ring), "cpecan_k_wv_%s%s" % (r, ring.suffix))
        print("%s%s: %d VGPRs; %s%s: %d" % (s, b.suffix, mine["vgpr"], r, ring.suffix, theirs["vgpr"]))


@needs_hipcc
def test_at_two_cells_the_sweeps_share_a_simd():
    """a forward wave and a fused backward wave on one SIMD: 512 registers between them, allocated in blocks of 8"""
    b = fused_builds()["hf2"]
    text = device_asm(b)
    for fw, bw in (("forward", "backward_fx"), ("forward_sw", "backward_fx_sw")):
        f = kernel_meta(text, "cpecan_k_wv_%s%s" % (fw, b.suffix))["vgpr"]
        k = kernel_meta(text, "cpecan_k_wv_%s%s" % (bw, b.suffix))["vgpr"]
        print("%s%s %d + %s%s %d -> %d of 512" % (fw, b.suffix, f, bw, b.suffix, k, block8(f) + block8(k)))
        assert block8(f) + block8(k) <= 512


def test_an_object_defines_its_own_build_only():
    """as tests/test_prep_kernels_cpu.py asks of the listed builds: the object's kernels are the build's seven, every one
    with the build's suffix, none of the kernels compiled once in cpecan_kernel_prep.hip, and the build's one record"""
    from test_prep_kernels_cpu import ONCE
    if shutil.which("nm") is None:
        pytest.skip("nm not available: the symbols cannot be listed")
    for name, b in fused_builds().items():
        if not os.path.exists(b.obj):
            pytest.skip("the library's objects are not here")
        names = defined(b.obj)
        kernels = set(n for n in names if n.startswith("cpecan_k_"))
        assert kernels == set("cpecan_k_wv_%s%s" % (s, b.suffix) for s in KERNELS), name
        assert not set(ONCE) & names
        assert set(n for n in names if "_build" in n and n.startswith("cpecan_")) == {"cpecan_hdpfx_build" + b.suffix}


def test_the_library_exports_the_two_records_and_no_new_entry_point():
    lib = os.path.join(AMD, "libcpecan_hip.so")
    if not os.path.exists(lib):
        pytest.skip("library not built")
    if shutil.which("nm") is None:
        pytest.skip("nm not available: the exported symbols cannot be listed")
    names = defined(lib, "-D")
    assert set(n for n in names if n.startswith("cpecan_hdpfx_build")) == set("cpecan_hdpfx_build_hf%d" % n for n in (2, 3))
    assert not any(re.match(r"cpecan_wave_build_hf", n) or re.match(r"cpecan_wave[^_]", n) for n in names)
    header = open(os.path.join(ROOT, "include", "cpecan_hip.h")).read()
    declared = set(re.findall(r"\b(cpecan_hip_[a-z0-9_]+)\s*\(", header))
    assert set(n for n in names if n.startswith("cpecan_hip_")) == declared

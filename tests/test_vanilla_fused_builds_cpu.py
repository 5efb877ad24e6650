"""The vanilla machine's two fused builds of the wave file (vf2, vf3: the E-step summed inside the sweep back,
CPECAN_FLAG_VANILLA_FUSED_ESTEP) from the compiler's metadata.  The Makefile lists them apart from WV_BUILDS
(WV_FUSED_BUILDS, make print-fused-wave-builds, objects cpecan_kernel_wavefx_vf<n>.o: see the note there), so the table
of tests/test_sweep_build_resources.py and the object walk of tests/test_prep_kernels_cpu.py do not reach them; this
file asks of them what those two ask of a build: each object has exactly its four kernels and none of the ring path's,
defines nothing that is compiled once elsewhere, nothing spills, at two cells per lane the forward sweep and the fused
sweep back share a SIMD as the _v2 pair does (512 registers per lane, handed out in blocks of 8), and at three cells --
304 registers for the sweep back beside 264 for the forward sweep, DESIGN 4.0 -- only "no spill" is asked, as of the
strawMan _l3 fused sweeps.
The library exports the two records under a name of their own and no entry point beside those the header declares.
CPU-only: hipcc cross-compiles gfx950."""
import os
import re
import shutil

import pytest

from cpecan_load import ROOT
from sweep_builds import AMD, HIPCC, Build, builds, defined, device_asm, kernel_meta, kernel_names, make_print

needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
KERNELS = ("forward", "backward_fx", "post", "resweep_fx")
EXPECTED = {"vf2": ("-DWV_L=2", "-DWV_VANILLA", "-DWV_FUSED"), "vf3": ("-DWV_L=3", "-DWV_VANILLA", "-DWV_FUSED")}


def fused_builds():
    found = {}
    for line in make_print("print-fused-wave-builds").splitlines():
        name, obj, src, defines = line.split("\t")
        assert src == "csrc/cpecan_kernel_wave.hip"
        found[name] = Build(name, name[:-1], int(name[-1]), "_" + name, "wave", os.path.join(AMD, obj),
                            os.path.join(AMD, src), tuple(defines.split()))
    return found


def test_the_two_builds_are_listed_apart_with_their_defines():
    found = fused_builds()
    assert sorted(found) == sorted(EXPECTED)
    for name, b in found.items():
        assert b.defines == EXPECTED[name] and b.tag == "vf" and b.rows == int(name[2])
        assert b.obj.endswith("csrc/cpecan_kernel_wavefx_%s.o" % name)
    listed = set(b.name for b in builds())
    assert not listed & set(found)          # not in print-builds ...
    assert {"v2", "v3"} <= listed           # ... where the builds they stand in for are
    objects = make_print("print-objects").split()
    for name in EXPECTED:                   # the library links them
        assert "csrc/cpecan_kernel_wavefx_%s.o" % name in objects


@needs_hipcc
@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_a_build_holds_its_four_kernels_and_nothing_spills(name):
    b = fused_builds()[name]
    text = device_asm(b)
    assert kernel_names(text) == set("cpecan_k_wv_%s%s" % (s, b.suffix) for s in KERNELS)
    assert "cpecan_k_wv_expect" not in text and "backward_em" not in text
    meta = dict((s, kernel_meta(text, "cpecan_k_wv_%s%s" % (s, b.suffix))) for s in KERNELS)
    for s, m in meta.items():
        print("%s%s: %d VGPRs, %d SGPRs, %d bytes of LDS" % (s, b.suffix, m["vgpr"], m["sgpr"], m["lds"]))
        assert m["spill"] == 0 and m["scratch"] == 0 and "scratch_" not in m["body"], "%s%s spills" % (s, b.suffix)
        assert m["threads"] == (256 if s == "post" else 64)
    if b.rows == 2:
        blocks = lambda m: (m["vgpr"] + 7) // 8 * 8  # noqa: E731
        for s in ("backward_fx", "resweep_fx"):
            assert blocks(meta["forward"]) + blocks(meta[s]) <= 512, \
                "%s%s (%d registers) and the forward sweep (%d) no longer share a SIMD" % (
                    s, b.suffix, meta[s]["vgpr"], meta["forward"]["vgpr"])


@needs_hipcc
@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_the_forward_sweep_is_the_ring_builds(name):
    """the fused build's forward sweep is the one of the build it stands in for: the same registers and static LDS"""
    b = fused_builds()[name]
    ring = dict((x.name, x) for x in builds())["v%d" % b.rows]
    mine = kernel_meta(device_asm(b), "cpecan_k_wv_forward" + b.suffix)
    theirs = kernel_meta(device_asm(ring), "cpecan_k_wv_forward" + ring.suffix)
    assert (mine["vgpr"], mine["sgpr"], mine["lds"]) == (theirs["vgpr"], theirs["sgpr"], theirs["lds"])


def test_an_object_defines_its_own_build_only():
    """as tests/test_prep_kernels_cpu.py asks of the listed builds: the object's kernels are the build's four, every one
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
        assert set(n for n in names if "_build" in n and n.startswith("cpecan_")) == {"cpecan_wavefx_build" + b.suffix}


def test_the_library_exports_the_two_records_and_no_new_entry_point():
    lib = os.path.join(AMD, "libcpecan_hip.so")
    if not os.path.exists(lib):
        pytest.skip("library not built")
    for b in fused_builds().values():
        assert os.path.exists(b.obj), b.obj
    if shutil.which("nm") is None:
        pytest.skip("nm not available: the exported symbols cannot be listed")
    names = defined(lib, "-D")
    assert set(n for n in names if n.startswith("cpecan_wavefx_build")) == {"cpecan_wavefx_build_vf2",
                                                                            "cpecan_wavefx_build_vf3"}
    assert not any(re.match(r"cpecan_(systolic|wave)_build_vf", n) for n in names)
    header = open(os.path.join(ROOT, "include", "cpecan_hip.h")).read()
    declared = set(re.findall(r"\b(cpecan_hip_[a-z0-9_]+)\s*\(", header))
    assert set(n for n in names if n.startswith("cpecan_hip_")) == declared

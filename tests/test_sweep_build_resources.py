"""Every build of the two sweep files that the Makefile lists (sweep_builds.builds()) holds exactly its own kernels and
keeps the registers, the scratch and the static LDS its occupancy is designed around, from the compiler's own metadata:
the register allocator has crossed such a line silently before (an inlined helper with its own constants, a loop the
optimiser decided to clone), halving the measured throughput.  One table per kernel file, keyed by the build's tag; a
build added to the Makefile's list under a tag that has a row is held to it with no edit here, a new tag needs its row.
The library exports one record per listed build and nothing else under those names.  CPU-only: hipcc cross-compiles
gfx950."""
import os
import re
import shutil

import pytest

from cpecan_load import ROOT
from sweep_builds import AMD, HIPCC, builds, defined, device_asm, kernel_meta, kernel_names

needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
LDS_PER_CU = 160 * 1024


def of_family(family):
    return dict(argnames="build", argvalues=[b for b in builds() if b.family == family],
                ids=lambda b: b.name or "unsuffixed")


def shares_cu(waves):
    """static LDS: at the budget's occupancy a CU holds this many waves, so waves / rows workgroups (one at least)"""
    return lambda lds, rows: lds * max(1, waves // rows) <= LDS_PER_CU


FB, FBE = ("forward", "backward"), ("forward", "backward", "expect")
# tag: the kernels of a build, the VGPRs each may take -- 128: four waves per SIMD (two eight-wave workgroups share a
# CU), 168: three (512 / 3, in allocation blocks of 8), 256: two -- and the rule its static LDS keeps
WORKGROUP = {
    "r": (FBE, 128, lambda lds, rows: lds <= 64 * 1024),
    "v": (FB, 168, shares_cu(12)),   # posterior decode only: no E-step on these builds
    "ve": (FBE, 168, shares_cu(12)),  # (the vanilla and HDP track kernels are cpecan_kernel_prep.hip's)
    "h": (FB, 128, shares_cu(16)),
    "he": (FBE, 128, shares_cu(16)),
    "f": (FB, 256, shares_cu(8)),    # the expectations are summed inside the sweep back: no expectation kernel
}
# (VGPRs, static LDS bytes) of the strawMan builds' forward and backward kernels before the vanilla switch was added
STRAWMAN = {
    1: dict(forward=(112, 13984), backward=(125, 2720)),
    2: dict(forward=(114, 15152), backward=(127, 3888)),
    3: dict(forward=(112, 16320), backward=(125, 5056)),
    4: dict(forward=(114, 17488), backward=(127, 6224)),
    6: dict(forward=(111, 19824), backward=(127, 8560)),
    8: dict(forward=(111, 22160), backward=(127, 10896)),
}


@needs_hipcc
@pytest.mark.parametrize(**of_family("systolic"))
def test_workgroup_build_keeps_its_kernels_and_budget(build):
    text = device_asm(build)
    stems, vgpr_cap, lds_fits = WORKGROUP[build.tag]
    assert kernel_names(text) == set("cpecan_k_sy_%s%s" % (s, build.suffix) for s in stems)
    if "expect" not in stems:
        assert "cpecan_k_sy_expect" not in text
    for stem in stems:
        name = "cpecan_k_sy_%s%s" % (stem, build.suffix)
        m = kernel_meta(text, name)
        assert m["threads"] == 64 * build.rows
        assert m["vgpr"] <= vgpr_cap, "%s uses %d VGPRs" % (name, m["vgpr"])
        assert m["spill"] == 0 and m["scratch"] == 0 and "scratch_" not in m["body"], "%s spills to scratch" % name
        assert lds_fits(m["lds"], build.rows), "%s takes %d bytes of static LDS" % (name, m["lds"])
        if build.tag == "r" and stem in STRAWMAN[build.rows]:
            assert (m["vgpr"], m["lds"]) == STRAWMAN[build.rows][stem], name
    if build.tag == "f":  # the forward sweep is the other builds' E-step forward sweep: four waves per SIMD
        assert kernel_meta(text, "cpecan_k_sy_forward" + build.suffix)["vgpr"] <= 128


SWEEPS = ("forward", "forward_sw", "backward", "backward_sw", "backward_em", "resweep", "resweep_sw", "expect", "post")
BACK = ("backward", "resweep", "backward_em")  # (every machine's E-step sweeps back with the last)
FX = ("backward_fx", "backward_fx_sw", "resweep_fx", "resweep_fx_sw")  # the expectations summed inside the sweep back
FXV = ("backward_fx", "resweep_fx")  # ... of the vanilla machine's fused builds: no switch, and no other sweep back
# tag: the kernels of a build; per number of cells, the sweeps back that share a SIMD with the forward sweep (one
# forward and one backward wave per SIMD: the forward sweep of window w+1 beside the backward sweep of window w; a
# unified register file of 512 per lane, handed out in blocks of 8) and the ones that only must not spill; the VGPRs of
# the forward sweep where they are capped.  Four cells per lane are the documented exception (the backward sweep takes
# 306 registers: one wave per SIMD while it runs), and at three the fused sweeps back are one too (364 against 248
# beside the forward sweep; measured faster than the B-ring path all the same), as are the vanilla machine's
# (304 beside 264)
WAVE = {
    "l": (SWEEPS + ("backward_em_sw",) + FX, {2: BACK + FX, 3: BACK}, {3: FX}, None),
    "h": (SWEEPS + ("backward_em_sw",), {3: BACK}, {}, 192),  # three register pairs per slot, not ten: a light forward
    "v": (SWEEPS, {2: BACK}, {}, None),
    "vf": (("forward", "post") + FXV, {2: FXV, 3: ()}, {3: FXV}, None),  # the fused E-step and nothing else
}


@needs_hipcc
@pytest.mark.parametrize(**of_family("wave"))
def test_wave_build_keeps_its_kernels_and_budget(build):
    text = device_asm(build)
    stems, paired, unspilled, forward_cap = WAVE[build.tag]
    assert kernel_names(text) == set("cpecan_k_wv_%s%s" % (s, build.suffix) for s in stems)
    if build.rows not in paired:
        return
    meta = dict((s, kernel_meta(text, "cpecan_k_wv_%s%s" % (s, build.suffix)))
                for s in ("forward",) + paired[build.rows] + unspilled.get(build.rows, ()))
    forward = meta.pop("forward")
    assert forward["spill"] == 0 and (forward_cap is None or forward["vgpr"] <= forward_cap)
    for stem, m in meta.items():
        assert m["spill"] == 0, "%s%s spills %d VGPRs to scratch" % (stem, build.suffix, m["spill"])
        if stem in paired[build.rows]:
            assert (forward["vgpr"] + 7) // 8 * 8 + (m["vgpr"] + 7) // 8 * 8 <= 512, \
                "%s%s (%d registers) and the forward sweep (%d) no longer share a SIMD" % (
                    stem, build.suffix, m["vgpr"], forward["vgpr"])


@needs_hipcc
@pytest.mark.parametrize("name", ("vf2", "vf3"))
def test_vanilla_fused_build_spills_nowhere_and_keeps_the_ring_builds_forward_sweep(name):
    """the vanilla machine's fused builds are compiled as the vanilla builds plus -DWV_FUSED; none of their four kernels,
    the post kernel included, touches scratch; and the forward sweep is the one of the build they stand in for (_v<n>):
    the same registers and static LDS"""
    listed = dict((b.name, b) for b in builds())
    build, ring = listed[name], listed["v" + name[2]]
    assert build.defines == ("-DWV_L=" + name[2], "-DWV_VANILLA", "-DWV_FUSED")
    text = device_asm(build)
    assert "cpecan_k_wv_expect" not in text and "backward_em" not in text
    for stem in WAVE["vf"][0]:
        m = kernel_meta(text, "cpecan_k_wv_%s%s" % (stem, build.suffix))
        assert m["spill"] == 0 and m["scratch"] == 0 and "scratch_" not in m["body"], "%s%s spills" % (stem, build.suffix)
        assert m["threads"] == (256 if stem == "post" else 64)
    mine = kernel_meta(text, "cpecan_k_wv_forward" + build.suffix)
    theirs = kernel_meta(device_asm(ring), "cpecan_k_wv_forward" + ring.suffix)
    assert (mine["vgpr"], mine["sgpr"], mine["lds"]) == (theirs["vgpr"], theirs["sgpr"], theirs["lds"])


def test_library_exports_the_declared_names_and_the_listed_builds():
    """a build adds kernels and one record, no entry point: what libcpecan_hip.so exports under the cpecan_hip_ prefix is
    exactly what include/cpecan_hip.h declares, its build records are exactly the list's, and every object is there"""
    lib = os.path.join(AMD, "libcpecan_hip.so")
    if not os.path.exists(lib):
        pytest.skip("library not built")
    for b in builds():
        assert os.path.exists(b.obj), b.obj
    if shutil.which("nm") is None:
        pytest.skip("nm not available: the exported symbols cannot be listed")
    names = defined(lib, "-D")
    header = open(os.path.join(ROOT, "include", "cpecan_hip.h")).read()
    declared = set(re.findall(r"\b(cpecan_hip_[a-z0-9_]+)\s*\(", header))
    assert set(n for n in names if n.startswith("cpecan_hip_")) == declared
    assert re.search(r"#define CPECAN_FLAG_WORKGROUP_FUSED_ESTEP 2048\b", header)
    listed = set("cpecan_%s_build%s" % (b.family, b.suffix) for b in builds())
    assert set(n for n in names if re.match(r"cpecan_(systolic|wave)_build", n)) == listed
    assert {"cpecan_wave_build_vf2", "cpecan_wave_build_vf3"} <= listed
    # ... under the family's name, not one of their own as when they were off the list (cpecan_wave<something>_build_vf<n>)
    assert not any(re.match(r"cpecan_wave[^_]", n) for n in names)
    assert "cpecan_systolic_build_h4" not in names  # the HDP wave builds reach 248: no four-wave build
    assert {"cpecan_systolic_machine", "cpecan_systolic_machine_vanilla", "cpecan_systolic_machine_hdp"} <= names

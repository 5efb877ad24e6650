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


def by_name():
    return dict((b.name, b) for b in builds())


def block8(n):
    """registers are handed out in allocation blocks of 8"""
    return (n + 7) // 8 * 8


def waves_per_cu(vgprs):
    """waves a CU holds of a kernel with that many registers: four SIMDs of 512, eight waves each at the most"""
    return 4 * min(8, 512 // block8(vgprs))


def shares_cu(waves):
    """static LDS: at the budget's occupancy a CU holds this many waves, so waves / rows workgroups (one at least)"""
    return lambda lds, rows, stem=None: lds * max(1, waves // rows) <= LDS_PER_CU


def shares_cu_as(tag):
    """static LDS: the workgroups per CU that the same kernel of the <tag><rows> build gets from its own registers stay"""
    def fits(lds, rows, stem):
        ring = by_name()["%s%d" % (tag, rows)]
        vgpr = kernel_meta(device_asm(ring), "cpecan_k_sy_%s%s" % (stem, ring.suffix))["vgpr"]
        return shares_cu(max(1, waves_per_cu(vgpr) // rows) * rows)(lds, rows)
    return fits


FB, FBE = ("forward", "backward"), ("forward", "backward", "expect")
# tag: the kernels of a build, the VGPRs each may take -- 128: four waves per SIMD (two eight-wave workgroups share a
# CU), 168: three (512 / 3, in allocation blocks of 8), 256: two -- and the rule its static LDS keeps; where the sweep
# back has a line of its own, per waves per workgroup: its VGPRs and (or None) the workgroups a CU then holds exactly
WORKGROUP = {
    "r": (FBE, 128, lambda lds, rows, stem: lds <= 64 * 1024),
    "v": (FB, 168, shares_cu(12)),   # posterior decode only: no E-step on these builds
    "ve": (FBE, 168, shares_cu(12)),  # (the vanilla and HDP track kernels are cpecan_kernel_prep.hip's)
    "h": (FB, 128, shares_cu(16)),
    "he": (FBE, 128, shares_cu(16)),
    "f": (FB, 256, shares_cu(8)),    # the expectations are summed inside the sweep back: no expectation kernel
    # the vanilla machine's: the compiler lands on 144 / 141 / 145 against the 126 / 124 / 128 of the _ve sweep back (the
    # four F.gapX in flight, the two sums, their column and the record addresses); held to 128 it spills
    "vf": (FB, 256, shares_cu(12), {4: (168, None), 6: (168, None), 8: (168, None)}),
    # the HDP machine's: _hf6 is forced to three waves per SIMD (164 with the eight sums in LDS: the two workgroups per CU
    # of _he6), _hf8 takes 178 by itself (one workgroup per CU where _he8's 121 have two); DESIGN 5, round 27
    "hf": (FB, 256, shares_cu_as("he"), {6: (168, 2), 8: (256, None)}),
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
    stems, vgpr_cap, lds_fits = WORKGROUP[build.tag][:3]
    assert kernel_names(text) == set("cpecan_k_sy_%s%s" % (s, build.suffix) for s in stems)
    if "expect" not in stems:
        assert "cpecan_k_sy_expect" not in text
    for stem in stems:
        name = "cpecan_k_sy_%s%s" % (stem, build.suffix)
        m = kernel_meta(text, name)
        assert m["threads"] == 64 * build.rows
        assert m["vgpr"] <= vgpr_cap, "%s uses %d VGPRs" % (name, m["vgpr"])
        assert m["spill"] == 0 and m["scratch"] == 0 and "scratch_" not in m["body"], "%s spills to scratch" % name
        assert lds_fits(m["lds"], build.rows, stem), "%s takes %d bytes of static LDS" % (name, m["lds"])
        if build.tag == "r" and stem in STRAWMAN[build.rows]:
            assert (m["vgpr"], m["lds"]) == STRAWMAN[build.rows][stem], name
    if build.tag == "f":  # the forward sweep is the other builds' E-step forward sweep: four waves per SIMD
        assert kernel_meta(text, "cpecan_k_sy_forward" + build.suffix)["vgpr"] <= 128
    for own_line in WORKGROUP[build.tag][3:]:
        back_cap, groups = own_line[build.rows]
        back = kernel_meta(text, "cpecan_k_sy_backward" + build.suffix)["vgpr"]
        assert back <= back_cap, "backward%s uses %d VGPRs" % (build.suffix, back)
        assert groups is None or waves_per_cu(back) // build.rows == groups


SWEEPS = ("forward", "forward_sw", "backward", "backward_sw", "backward_em", "resweep", "resweep_sw", "expect", "post")
BACK = ("backward", "resweep", "backward_em")  # (every machine's E-step sweeps back with the last)
FX = ("backward_fx", "backward_fx_sw", "resweep_fx", "resweep_fx_sw")  # the expectations summed inside the sweep back
FXV = ("backward_fx", "resweep_fx")  # ... of the vanilla machine's fused builds: no switch, and no other sweep back
# tag: the kernels of a build; per number of cells, the sweeps back that share a SIMD with the forward sweep (one
# forward and one backward wave per SIMD: the forward sweep of window w+1 beside the backward sweep of window w; a
# unified register file of 512 per lane, handed out in blocks of 8; a pair names its own forward sweep) and the ones that
# only must not spill; the VGPRs of the forward sweep and of the post kernel where they are capped.  Four cells per lane
# are the documented exception (the backward sweep takes 306 registers: one wave per SIMD while it runs), and at three the
# fused sweeps back are one too (364 against 248 beside the forward sweep; measured faster than the B-ring path all the
# same), as are the vanilla machine's (304 beside 264)
WAVE = {
    "l": (SWEEPS + ("backward_em_sw",) + FX, {2: BACK + FX, 3: BACK}, {3: FX}, None, None),
    "h": (SWEEPS + ("backward_em_sw",), {3: BACK}, {}, 192, None),  # three register pairs per slot, not ten: a light forward
    "v": (SWEEPS, {2: BACK}, {}, None, None),
    "vf": (("forward", "post") + FXV, {2: FXV, 3: ()}, {3: FXV}, None, None),  # the fused E-step and nothing else
    # the HDP machine's, each sweep with and without the gap Y -> gap X term; the post kernel at eight waves per SIMD
    "hf": (("forward", "forward_sw", "post") + FX, {2: (("forward", "backward_fx"), ("forward_sw", "backward_fx_sw")),
                                                     3: (), 4: ()}, {3: ("forward_sw",) + FX, 4: ("forward_sw",) + FX},
           None, 64),
}


@needs_hipcc
@pytest.mark.parametrize(**of_family("wave"))
def test_wave_build_keeps_its_kernels_and_budget(build):
    text = device_asm(build)
    stems, paired, unspilled, forward_cap, post_cap = WAVE[build.tag]
    assert kernel_names(text) == set("cpecan_k_wv_%s%s" % (s, build.suffix) for s in stems)
    meta = lambda stem: kernel_meta(text, "cpecan_k_wv_%s%s" % (stem, build.suffix))  # noqa: E731
    assert post_cap is None or meta("post")["vgpr"] <= post_cap
    if build.rows not in paired:
        return
    pairs = [p if isinstance(p, tuple) else ("forward", p) for p in paired[build.rows]]
    forward = meta("forward")
    assert forward["spill"] == 0 and (forward_cap is None or forward["vgpr"] <= forward_cap)
    for stem in [s for pair in pairs for s in pair] + list(unspilled.get(build.rows, ())):
        assert meta(stem)["spill"] == 0, "%s%s spills %d VGPRs to scratch" % (stem, build.suffix, meta(stem)["spill"])
    for fw, back in pairs:
        f, m = meta(fw)["vgpr"], meta(back)["vgpr"]
        assert block8(f) + block8(m) <= 512, "%s%s (%d registers) and %s (%d) no longer share a SIMD" % (
            back, build.suffix, m, fw, f)


# the fused build: the ring build it stands in for (FUSED_STAND_INS of cpecan_hip.hip), with the same machine's define
FUSED = {"vf2": "v2", "vf3": "v3", "hf2": "h2", "hf3": "h3", "hf4": "h4",
         "vf4": "ve4", "vf6": "ve6", "vf8": "ve8", "hf6": "he6", "hf8": "he8"}
# _hf4 as the compiler of this tree makes it: registers (arch + acc) and static LDS per kernel
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


@needs_hipcc
@pytest.mark.parametrize("name", sorted(FUSED))
def test_fused_build_spills_nowhere_and_keeps_the_ring_builds_forward_sweep(name):
    """a fused build is compiled as the machine's other builds plus the file's FUSED define; it has no expectation kernel
    and no sweep back that parks cells for one; none of its kernels, the post kernel included, touches scratch; and every
    forward sweep is the one of the build it stands in for: the same registers and static LDS"""
    build, ring = by_name()[name], by_name()[FUSED[name]]
    sy = build.family == "systolic"
    k = "cpecan_k_%s_" % ("sy" if sy else "wv")
    machine = {"v": "VANILLA", "h": "HDP"}[name[0]]
    assert build.defines == (("-DSY_R=" + name[2], "-DSY_" + machine, "-DSY_FUSED") if sy else
                             ("-DWV_L=" + name[2], "-DWV_" + machine, "-DWV_FUSED"))
    text, ringtext = device_asm(build), device_asm(ring)
    assert k + "expect" not in text and "backward_em" not in text
    stems = (WORKGROUP if sy else WAVE)[build.tag][0]
    for stem in stems:
        m = kernel_meta(text, k + stem + build.suffix)
        print("%s%s: %d VGPRs, %d SGPRs, %d bytes of LDS" % (stem, build.suffix, m["vgpr"], m["sgpr"], m["lds"]))
        assert m["spill"] == 0 and m["scratch"] == 0 and "scratch_" not in m["body"], "%s%s spills" % (stem, build.suffix)
        assert m["threads"] == (64 * build.rows if sy else 256 if stem == "post" else 64)
        assert m["vgpr"] <= 512
        if name == "hf4":
            assert (m["vgpr"], m["lds"]) == COUNTS[stem], stem
    for stem in [s for s in stems if s.startswith("forward")]:
        mine, theirs = kernel_meta(text, k + stem + build.suffix), kernel_meta(ringtext, k + stem + ring.suffix)
        assert (mine["vgpr"], mine["sgpr"], mine["lds"]) == (theirs["vgpr"], theirs["sgpr"], theirs["lds"]), stem
    if sy and build.tag == "vf":  # the 60 bins live in LDS the E-step builds had and did not use
        back, ringback = kernel_meta(text, k + "backward" + build.suffix), kernel_meta(ringtext, k + "backward" + ring.suffix)
        assert back["lds"] == ringback["lds"]
    if name == "hf4":
        hf4_against_the_ring_build(text, ringtext)


def hf4_against_the_ring_build(text, ringtext):
    """the post kernel's LDS is _h4's; what _h4 reports for backward_em, and the forward + backward sums in allocation
    blocks of 8: the ring build's pair fits a SIMD's 512 registers on the kernels without the switch and misses them with
    it; the fused build's pair fits on neither, which is what the measurement of round 28 is read against"""
    theirs = kernel_meta(ringtext, "cpecan_k_wv_post_h4")
    assert kernel_meta(text, "cpecan_k_wv_post_hf4")["lds"] == theirs["lds"] and theirs["vgpr"] <= 64
    for s, want in RING_COUNTS.items():
        m = kernel_meta(ringtext, "cpecan_k_wv_%s_h4" % s)
        assert m["spill"] == 0 and m["scratch"] == 0
        assert (m["vgpr"], m["lds"]) == want, s
    for sw in ("", "_sw"):
        f = kernel_meta(ringtext, "cpecan_k_wv_forward%s_h4" % sw)["vgpr"]
        r = kernel_meta(ringtext, "cpecan_k_wv_backward_em%s_h4" % sw)["vgpr"]
        k = kernel_meta(text, "cpecan_k_wv_backward_fx%s_hf4" % sw)["vgpr"]
        assert (block8(f) + block8(r), block8(f) + block8(k)) == PAIRS[sw], sw
    assert PAIRS[""][0] <= 512 < PAIRS["_sw"][0] and min(PAIRS[""][1], PAIRS["_sw"][1]) > 512


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
    assert set("cpecan_%s_build_%s" % (by_name()[n].family, n) for n in FUSED) <= listed and len(FUSED) == 10
    # ... under the family's name, not one of their own as when they were off the list (cpecan_wave<something>_build_vf<n>)
    assert not any(re.match(r"cpecan_wave[^_]", n) for n in names)
    assert not any(re.match(r"cpecan_(systolic|hdpw?)fx_build", n) for n in names)  # (the names of the lists of old)
    assert "cpecan_systolic_build_h4" not in names  # the HDP wave builds reach 248: no four-wave build
    assert {"cpecan_systolic_machine", "cpecan_systolic_machine_vanilla", "cpecan_systolic_machine_hdp"} <= names

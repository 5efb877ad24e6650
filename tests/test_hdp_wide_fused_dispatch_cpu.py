"""CPECAN_FLAG_WIDE_BANDS_HDP_FUSED_ESTEP (131072) through cpecan_hip_plan_expectation_pass and cpecan_hip_plan_dispatch
(the answers of choose_dispatch in cpecan_hip.hip): no device.

Every expected value is a literal from include/cpecan_hip.h: an HDP batch of expectations that
CPECAN_FLAG_WIDE_BANDS_HDP_ESTEP (or CPECAN_WIDE_BANDS_HDP_ESTEP=1) puts on the _he6 / _he8 workgroup builds -- a widest
band of 249..376 k-mers at six waves, of 377..504 at eight, edges stepping by one, no CPECAN_FLAG_GENERAL_KERNEL -- sums
its expectations inside the sweep back (_hf6 / _hf8) when it carries the flag and keeps the ring of backward cells when
it does not.  The flag means nothing to a posterior batch, to another machine, to a band of at most 248 k-mers or past
504, to the general kernel or to a batch without the wide-bands flag of the E-step; CPECAN_FLAG_HDP_FUSED_ESTEP (65536)
keeps meaning nothing at these widths; CPECAN_EXPECT_FUSED=0 does not undo it (the fused builds have no other form of
the E-step), and cpecan_hip_plan_dispatch answers the same kernel, family, rows and widest band with and without it."""
import os
import re

import pytest

from cpecan_load import ROOT, binding
from harness import BATCH_ENV

cp = binding()

FUSED = 131072
NAME = "FLAG_WIDE_BANDS_HDP_FUSED_ESTEP"
SM, DNA, VAN, HDP, SM4, ECH = (cp.MACHINE_STRAWMAN, cp.MACHINE_DNA5, cp.MACHINE_VANILLA, cp.MACHINE_HDP,
                               cp.MACHINE_SM4, cp.MACHINE_ECHELON)
MACHINES = (SM, DNA, VAN, HDP, SM4, ECH)
POST, EXP = cp.MODE_POSTERIOR, cp.MODE_EXPECTATIONS
AUTO, GEN, SYS = cp.KERNEL_AUTO, cp.KERNEL_GENERAL, cp.KERNEL_SYSTOLIC
GENK, WIDE_HE, WIDE_VE = cp.FLAG_GENERAL_KERNEL, cp.FLAG_WIDE_BANDS_HDP_ESTEP, cp.FLAG_WIDE_BANDS_VANILLA_ESTEP
SIX = (249, 376)                          # the ground of _he6 / _hf6 ...
EIGHT = (377, 504)                        # ... and of _he8 / _hf8
SERVED = SIX + EIGHT
OUTSIDE = (1, 120, 184, 185, 248, 505)    # the wave builds', then past every build
WIDTHS = OUTSIDE[:-1] + SERVED + OUTSIDE[-1:]
# every flag a create call takes but this one, by its value in include/cpecan_hip.h
OTHER_FLAGS = dict(DEBUG_DUMP=1, UNBANDED=2, SCAN_DECODE=4, EXPECTATIONS=8, WORKGROUP_KERNELS=16, GENERAL_KERNEL=32,
                   SMALL_FOOTPRINT=64, WIDE_BANDS=128, WIDE_BANDS_HDP=256, WIDE_BANDS_HDP_ESTEP=512,
                   WIDE_BANDS_VANILLA_ESTEP=1024, WORKGROUP_FUSED_ESTEP=2048, WIDE_BANDS_FUSED_ESTEP=4096,
                   ASM_NARROW_BANDS=8192, VANILLA_FUSED_ESTEP=16384, WIDE_BANDS_VANILLA_FUSED_ESTEP=32768,
                   HDP_FUSED_ESTEP=65536)


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in BATCH_ENV:
        monkeypatch.delenv(k, raising=False)


def fused(machine=HDP, mode=EXP, kernel=AUTO, flags=FUSED | WIDE_HE, width=300, edges=True):
    return cp.plan_expectation_pass(machine, mode, kernel, flags, width, edges)


def answer(*q):
    """the four outputs of cpecan_hip_plan_dispatch, or the code and the text of the refusal"""
    try:
        return cp.plan_dispatch(*q)
    except cp.CpecanError as e:
        return (e.code, str(e))


def sweep(wave, rows, width):
    return dict(kernel=SYS, wave=wave, rows=rows, build_max_width=width)


def test_the_header_and_the_binding_name_the_flag():
    header = open(os.path.join(ROOT, "include", "cpecan_hip.h")).read()
    assert re.search(r"#define CPECAN_FLAG_WIDE_BANDS_HDP_FUSED_ESTEP %d\b" % FUSED, header)
    assert getattr(cp, NAME) == FUSED
    others = dict((k[5:], v) for k, v in vars(cp).items() if k.startswith("FLAG_") and k != NAME)
    assert others.items() >= OTHER_FLAGS.items()
    assert not any(v & FUSED for v in others.values())   # a number of its own: no other flag has the bit
    for name, value in re.findall(r"#define (CPECAN_FLAG_\w+) (\d+)\b", header):
        assert name == "CPECAN_" + NAME or not int(value) & FUSED, name


@pytest.mark.parametrize("kernel", [AUTO, GEN, SYS])  # the HDP create call has no kernel argument: any value
def test_the_flag_on_the_workgroup_estep_builds(kernel, monkeypatch):
    for by_env in (False, True):
        wide = 0 if by_env else WIDE_HE
        if by_env:
            monkeypatch.setenv("CPECAN_WIDE_BANDS_HDP_ESTEP", "1")
        for widths, rows, reach in ((SIX, 6, 376), (EIGHT, 8, 504)):
            for w in widths:
                assert fused(kernel=kernel, flags=FUSED | wide, width=w) == 1, (by_env, w)
                assert fused(kernel=kernel, flags=wide, width=w) == 0, (by_env, w)
                assert (answer(HDP, EXP, kernel, FUSED | wide, w, True) == sweep(0, rows, reach)
                        == answer(HDP, EXP, kernel, wide, w, True)), (by_env, w)
        for w in OUTSIDE:
            assert fused(kernel=kernel, flags=FUSED | wide, width=w) == 0, (by_env, w)
            assert answer(HDP, EXP, kernel, FUSED | wide, w, True) == answer(HDP, EXP, kernel, wide, w, True), (by_env, w)


def test_without_the_wide_bands_flag_of_the_estep_it_means_nothing():
    for w in WIDTHS:
        for edges in (True, False):
            assert fused(flags=FUSED, width=w, edges=edges) == 0, (w, edges)
            assert fused(flags=FUSED | cp.FLAG_WIDE_BANDS_HDP, width=w, edges=edges) == 0, (w, edges)
            assert answer(HDP, EXP, AUTO, FUSED, w, edges) == answer(HDP, EXP, AUTO, 0, w, edges), (w, edges)
    for w in SERVED:
        assert answer(HDP, EXP, AUTO, FUSED, w, True)["kernel"] == GEN, w


def test_without_the_flag_nothing_changes(monkeypatch):
    """an HDP batch of expectations on the _he builds keeps the ring, whatever CPECAN_EXPECT_FUSED says and with the wave
    builds' flag (65536) too"""
    for value in (None, "1", "0"):
        if value is not None:
            monkeypatch.setenv("CPECAN_EXPECT_FUSED", value)
        for w in WIDTHS:
            for edges in (True, False):
                assert fused(flags=WIDE_HE, width=w, edges=edges) == 0, (value, w, edges)
                if w > 184:
                    assert fused(flags=WIDE_HE | cp.FLAG_HDP_FUSED_ESTEP, width=w, edges=edges) == 0, (value, w, edges)


def test_the_ring_variable_does_not_undo_the_flag(monkeypatch):
    for value in ("0", "1"):
        monkeypatch.setenv("CPECAN_EXPECT_FUSED", value)
        for w in WIDTHS:
            assert fused(width=w) == (1 if w in SERVED else 0), (value, w)
            assert fused(flags=WIDE_HE, width=w) == 0, (value, w)
            assert answer(HDP, EXP, AUTO, FUSED | WIDE_HE, w, True) == answer(HDP, EXP, AUTO, WIDE_HE, w, True), (value, w)


def test_the_flag_means_nothing_to_the_general_kernel_or_to_edges_that_jump():
    for w in WIDTHS:
        assert fused(flags=FUSED | WIDE_HE | GENK, width=w) == 0, w
        assert answer(HDP, EXP, AUTO, FUSED | WIDE_HE | GENK, w, True)["kernel"] == GEN
        assert fused(width=w, edges=False) == 0, w               # (such a band is the general kernel's)
        assert answer(HDP, EXP, AUTO, FUSED | WIDE_HE, w, False)["kernel"] == GEN


@pytest.mark.parametrize("machine", MACHINES)
def test_the_flag_means_nothing_to_a_posterior_batch_or_another_machine(machine, monkeypatch):
    every_wide = WIDE_HE | WIDE_VE | cp.FLAG_WIDE_BANDS | cp.FLAG_WIDE_BANDS_HDP
    for mode in (POST, EXP):
        for kernel in (AUTO, GEN, SYS):
            for wide in (0, WIDE_HE, every_wide):
                for w in WIDTHS:
                    for edges in (True, False):
                        without = cp.plan_expectation_pass(machine, mode, kernel, wide, w, edges)
                        with_flag = cp.plan_expectation_pass(machine, mode, kernel, wide | FUSED, w, edges)
                        serves = machine == HDP and mode == EXP and w in SERVED and edges and wide != 0
                        assert with_flag == (1 if serves else without), (mode, kernel, wide, w, edges)
                        if machine != SM:
                            assert without == 0, (mode, kernel, wide, w, edges)
    # the strawMan machine's own fused E-step is as it was, with the bit and without
    if machine == SM:
        assert fused(machine=SM, flags=FUSED, width=100) == 1 == fused(machine=SM, flags=0, width=100)
        monkeypatch.setenv("CPECAN_EXPECT_FUSED", "0")
        assert fused(machine=SM, flags=FUSED, width=100) == 0


@pytest.mark.parametrize("name", sorted(OTHER_FLAGS))
def test_beside_every_other_flag(name):
    """the other flag does to an HDP E-step what it does alone (it moves the batch to the general kernel, refuses it or
    means nothing); where the batch stays on the six- and eight-wave E-step builds this flag fuses it, and nowhere
    else"""
    other = OTHER_FLAGS[name] | WIDE_HE
    for w in WIDTHS:
        for edges in (True, False):
            alone = answer(HDP, EXP, AUTO, other, w, edges)
            assert answer(HDP, EXP, AUTO, other | FUSED, w, edges) == alone, (w, edges)
            served = isinstance(alone, dict) and alone["kernel"] == SYS and alone["wave"] == 0 and alone["rows"] in (6, 8)
            # (the wave builds' flag fuses its own ground, two and three cells per lane, with this one or without)
            theirs = name == "HDP_FUSED_ESTEP" and (isinstance(alone, dict) and alone["kernel"] == SYS and alone["wave"] == 1
                                                     and alone["rows"] <= 3)
            assert fused(flags=other | FUSED, width=w, edges=edges) == (1 if served or theirs else 0), (w, edges)
            assert fused(flags=other, width=w, edges=edges) == (1 if theirs else 0), (w, edges)
    if name in ("UNBANDED", "DEBUG_DUMP"):   # refused as without the flag, with the same text
        assert isinstance(answer(HDP, EXP, AUTO, other | FUSED, 300, True), tuple)
    if name == "GENERAL_KERNEL":
        assert answer(HDP, EXP, AUTO, other | FUSED, 300, True)["kernel"] == GEN
    if name in ("SMALL_FOOTPRINT", "WIDE_BANDS", "HDP_FUSED_ESTEP"):   # means nothing here: the flag fuses
        assert fused(flags=other | FUSED, width=300) == 1 and fused(flags=other | FUSED, width=400) == 1


@pytest.mark.parametrize("mode", [POST, EXP])
@pytest.mark.parametrize("machine", MACHINES)
def test_the_kernel_choice_does_not_move(machine, mode, monkeypatch):
    """cpecan_hip_plan_dispatch: the same kernel, family, rows and widest band -- or the same refusal with the same
    text -- with the bit, for every machine in both modes, under both families' defaults"""
    flag_sets = (0, cp.FLAG_WORKGROUP_KERNELS, cp.FLAG_WIDE_BANDS, GENK, WIDE_VE, WIDE_HE, cp.FLAG_UNBANDED,
                 cp.FLAG_DEBUG_DUMP, cp.FLAG_WIDE_BANDS_HDP | WIDE_HE, cp.FLAG_SMALL_FOOTPRINT | WIDE_HE,
                 cp.FLAG_HDP_FUSED_ESTEP | WIDE_HE)
    for by_env in (False, True):
        if by_env:
            monkeypatch.setenv("CPECAN_KERNELS", "systolic")
        for kernel in (AUTO, GEN, SYS):
            for flags in flag_sets:
                for w in WIDTHS:
                    for edges in (True, False):
                        q = (machine, mode, kernel, flags, w, edges)
                        assert answer(machine, mode, kernel, flags | FUSED, w, edges) == answer(*q), q


def test_no_variable_of_batch_creation_sets_it(monkeypatch):
    """the C-ABI reads no variable for this flag (libcpecan_host.so has CPECAN_WIDE_BANDS_HDP_FUSED_ESTEP for its own
    batches)"""
    for k in ("CPECAN_WIDE_BANDS_HDP_FUSED_ESTEP", "CPECAN_HDP_FUSED_ESTEP", "CPECAN_EXPECT_FUSED",
              "CPECAN_EXPECT_FUSED_WORKGROUP", "CPECAN_EXPECT_FUSED_WIDE", "CPECAN_WIDE_BANDS_HDP_ESTEP"):
        monkeypatch.setenv(k, "1")
    for w in WIDTHS:
        assert fused(flags=0, width=w) == 0, w
        assert fused(flags=WIDE_HE, width=w) == 0, w
    source = open(os.path.join(ROOT, "cpecan-signal_amd", "csrc", "cpecan_hip.hip")).read()
    assert "CPECAN_WIDE_BANDS_HDP_FUSED_ESTEP" not in source
    host = open(os.path.join(ROOT, "cpecan-signal_amd", "csrc", "host", "cpecan_api.c")).read()
    assert 'getenv("CPECAN_WIDE_BANDS_HDP_FUSED_ESTEP")' in host

"""CPECAN_FLAG_HDP_FUSED_ESTEP (65536) through cpecan_hip_plan_expectation_pass and cpecan_hip_plan_dispatch (the
answers of choose_dispatch in cpecan_hip.hip): no device.

Every expected value is a literal from include/cpecan_hip.h: an HDP batch of expectations on the wave kernels at two or
three cells per lane -- a widest band of at most 120 k-mers at two, of at most 184 at three, edges stepping by one, no
CPECAN_FLAG_GENERAL_KERNEL -- sums its expectations inside the sweep back when it carries the flag and keeps the ring of
backward cells when it does not.  The flag means nothing to a posterior batch, to another machine, to an HDP E-step at
four cells per lane (185..248 k-mers: _h4 keeps its ring), on the _he6 / _he8 workgroup builds (249..504 k-mers with
CPECAN_FLAG_WIDE_BANDS_HDP_ESTEP) or on the general kernel; CPECAN_EXPECT_FUSED=0 does not undo it (the fused builds
have no other form of the E-step), and cpecan_hip_plan_dispatch answers the same kernel, family, rows and widest band
with and without it."""
import os
import re

import pytest

from cpecan_load import ROOT, binding
from harness import BATCH_ENV

cp = binding()

FUSED = 65536
SM, DNA, VAN, HDP, SM4, ECH = (cp.MACHINE_STRAWMAN, cp.MACHINE_DNA5, cp.MACHINE_VANILLA, cp.MACHINE_HDP,
                               cp.MACHINE_SM4, cp.MACHINE_ECHELON)
MACHINES = (SM, DNA, VAN, HDP, SM4, ECH)
POST, EXP = cp.MODE_POSTERIOR, cp.MODE_EXPECTATIONS
AUTO, GEN, SYS = cp.KERNEL_AUTO, cp.KERNEL_GENERAL, cp.KERNEL_SYSTOLIC
GENK, WIDE_HE, WIDE_VE = cp.FLAG_GENERAL_KERNEL, cp.FLAG_WIDE_BANDS_HDP_ESTEP, cp.FLAG_WIDE_BANDS_VANILLA_ESTEP
TWO_CELLS = (1, 56, 57, 120)             # the ground of _h2 / _hf2 ...
THREE_CELLS = (121, 184)                 # ... and of _h3 / _hf3
SERVED = TWO_CELLS + THREE_CELLS
PAST = (185, 248, 249, 504, 505)         # _h4's, then the general kernel's or with the wide-bands flag the _he builds'
WIDTHS = SERVED + PAST
# every flag a create call takes but this one, by its value in include/cpecan_hip.h
OTHER_FLAGS = dict(DEBUG_DUMP=1, UNBANDED=2, SCAN_DECODE=4, EXPECTATIONS=8, WORKGROUP_KERNELS=16, GENERAL_KERNEL=32,
                   SMALL_FOOTPRINT=64, WIDE_BANDS=128, WIDE_BANDS_HDP=256, WIDE_BANDS_HDP_ESTEP=512,
                   WIDE_BANDS_VANILLA_ESTEP=1024, WORKGROUP_FUSED_ESTEP=2048, WIDE_BANDS_FUSED_ESTEP=4096,
                   ASM_NARROW_BANDS=8192, VANILLA_FUSED_ESTEP=16384, WIDE_BANDS_VANILLA_FUSED_ESTEP=32768)


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in BATCH_ENV:
        monkeypatch.delenv(k, raising=False)


def fused(machine=HDP, mode=EXP, kernel=AUTO, flags=FUSED, width=100, edges=True):
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
    assert re.search(r"#define CPECAN_FLAG_HDP_FUSED_ESTEP %d\b" % FUSED, header)
    assert cp.FLAG_HDP_FUSED_ESTEP == FUSED
    others = dict((k[5:], v) for k, v in vars(cp).items() if k.startswith("FLAG_") and k != "FLAG_HDP_FUSED_ESTEP")
    assert others.items() >= OTHER_FLAGS.items()
    assert not any(v & FUSED for v in others.values())   # a number of its own: no other flag has the bit
    for name, value in re.findall(r"#define (CPECAN_FLAG_\w+) (\d+)\b", header):
        assert name == "CPECAN_FLAG_HDP_FUSED_ESTEP" or not int(value) & FUSED, name


@pytest.mark.parametrize("kernel", [AUTO, GEN, SYS])  # the HDP create call has no kernel argument: any value
def test_the_flag_alone_on_the_wave_builds(kernel):
    for w in TWO_CELLS:
        assert fused(kernel=kernel, width=w) == 1, w
        assert fused(kernel=kernel, flags=0, width=w) == 0, w
        assert answer(HDP, EXP, kernel, FUSED, w, True) == sweep(1, 2, 120) == answer(HDP, EXP, kernel, 0, w, True), w
    for w in THREE_CELLS:
        assert fused(kernel=kernel, width=w) == 1, w
        assert fused(kernel=kernel, flags=0, width=w) == 0, w
        assert answer(HDP, EXP, kernel, FUSED, w, True) == sweep(1, 3, 184) == answer(HDP, EXP, kernel, 0, w, True), w


def test_a_narrow_band_forced_onto_three_cells(monkeypatch):
    monkeypatch.setenv("CPECAN_SYSTOLIC_ROWS", "3")
    for w in TWO_CELLS:
        assert answer(HDP, EXP, AUTO, FUSED, w, True) == sweep(1, 3, 184) == answer(HDP, EXP, AUTO, 0, w, True), w
        assert fused(width=w) == 1, w
        assert fused(flags=0, width=w) == 0, w
    # ... and onto four: _h4 keeps its ring
    monkeypatch.setenv("CPECAN_SYSTOLIC_ROWS", "4")
    for w in SERVED:
        assert answer(HDP, EXP, AUTO, FUSED, w, True) == sweep(1, 4, 248), w
        assert fused(width=w) == 0, w


def test_without_the_flag_nothing_changes(monkeypatch):
    """an HDP batch of expectations keeps the ring whatever CPECAN_EXPECT_FUSED says"""
    for value in (None, "1", "0"):
        if value is not None:
            monkeypatch.setenv("CPECAN_EXPECT_FUSED", value)
        for w in WIDTHS:
            for edges in (True, False):
                assert fused(flags=0, width=w, edges=edges) == 0, (value, w, edges)
                assert fused(flags=WIDE_HE, width=w, edges=edges) == 0, (value, w, edges)


def test_the_ring_variable_does_not_undo_the_flag(monkeypatch):
    for value in ("0", "1"):
        monkeypatch.setenv("CPECAN_EXPECT_FUSED", value)
        for w in WIDTHS:
            assert fused(width=w) == (1 if w <= 184 else 0), (value, w)
            assert fused(flags=0, width=w) == 0, (value, w)


def test_the_flag_means_nothing_past_three_cells():
    """four cells per lane keep the ring; past 248 the general kernel"""
    for w in (185, 248):
        assert answer(HDP, EXP, AUTO, FUSED, w, True) == sweep(1, 4, 248) == answer(HDP, EXP, AUTO, 0, w, True), w
        assert fused(width=w) == 0, w
    for w in (249, 504, 505):
        assert answer(HDP, EXP, AUTO, FUSED, w, True)["kernel"] == GEN, w
        assert fused(width=w) == 0, w


def test_the_flag_means_nothing_to_the_general_kernel():
    for w in WIDTHS:
        assert fused(flags=FUSED | GENK, width=w) == 0, w
        assert answer(HDP, EXP, AUTO, FUSED | GENK, w, True)["kernel"] == GEN
        assert fused(width=w, edges=False) == 0, w               # (such a band is the general kernel's)
        assert answer(HDP, EXP, AUTO, FUSED, w, False)["kernel"] == GEN


def test_the_flag_means_nothing_to_the_workgroup_estep_builds(monkeypatch):
    for by_env in (False, True):
        wide = 0 if by_env else WIDE_HE
        if by_env:
            monkeypatch.setenv("CPECAN_WIDE_BANDS_HDP_ESTEP", "1")
        for w, rows, reach in ((249, 6, 376), (376, 6, 376), (377, 8, 504), (504, 8, 504)):
            assert answer(HDP, EXP, AUTO, FUSED | wide, w, True) == sweep(0, rows, reach), w
            assert fused(flags=FUSED | wide, width=w) == 0, w
        for w in (185, 248, 505):
            assert fused(flags=FUSED | wide, width=w) == 0, w
        # a band the two- and three-cell builds hold is left to them, and to the flag
        for w in SERVED:
            assert fused(flags=FUSED | wide, width=w) == 1, w
            assert fused(flags=wide, width=w) == 0, w


@pytest.mark.parametrize("machine", MACHINES)
def test_the_flag_means_nothing_to_a_posterior_batch_or_another_machine(machine, monkeypatch):
    for mode in (POST, EXP):
        for kernel in (AUTO, GEN, SYS):
            for w in WIDTHS:
                for edges in (True, False):
                    without = cp.plan_expectation_pass(machine, mode, kernel, 0, w, edges)
                    with_flag = cp.plan_expectation_pass(machine, mode, kernel, FUSED, w, edges)
                    serves = machine == HDP and mode == EXP and w <= 184 and edges
                    assert with_flag == (1 if serves else without), (mode, kernel, w, edges)
                    if machine != SM:
                        assert without == 0, (mode, kernel, w, edges)
    # the strawMan machine's own fused E-step is as it was, with the bit and without
    if machine == SM:
        assert fused(machine=SM, flags=FUSED, width=100) == 1 == fused(machine=SM, flags=0, width=100)
        monkeypatch.setenv("CPECAN_EXPECT_FUSED", "0")
        assert fused(machine=SM, flags=FUSED, width=100) == 0


@pytest.mark.parametrize("name", sorted(OTHER_FLAGS))
def test_beside_every_other_flag(name):
    """the other flag does to an HDP E-step what it does alone (it moves the batch to the general kernel, refuses it or
    means nothing); where the batch stays on the two- and three-cell wave builds this flag fuses it, and nowhere else"""
    other = OTHER_FLAGS[name]
    for w in WIDTHS:
        for edges in (True, False):
            alone = answer(HDP, EXP, AUTO, other, w, edges)
            assert answer(HDP, EXP, AUTO, other | FUSED, w, edges) == alone, (w, edges)
            served = isinstance(alone, dict) and alone["kernel"] == SYS and alone["wave"] == 1 and alone["rows"] <= 3
            assert fused(flags=other | FUSED, width=w, edges=edges) == (1 if served else 0), (w, edges)
            assert fused(flags=other, width=w, edges=edges) == 0, (w, edges)
    if name in ("UNBANDED", "DEBUG_DUMP"):   # refused as without the flag, with the same text
        assert isinstance(answer(HDP, EXP, AUTO, other | FUSED, 100, True), tuple)
    if name == "GENERAL_KERNEL":
        assert answer(HDP, EXP, AUTO, other | FUSED, 100, True)["kernel"] == GEN


@pytest.mark.parametrize("mode", [POST, EXP])
@pytest.mark.parametrize("machine", MACHINES)
def test_the_kernel_choice_does_not_move(machine, mode, monkeypatch):
    """cpecan_hip_plan_dispatch: the same kernel, family, rows and widest band -- or the same refusal with the same
    text -- with the bit, for every machine in both modes, under both families' defaults"""
    flag_sets = (0, cp.FLAG_WORKGROUP_KERNELS, cp.FLAG_WIDE_BANDS, GENK, WIDE_VE, cp.FLAG_UNBANDED,
                 cp.FLAG_WIDE_BANDS_HDP | cp.FLAG_WIDE_BANDS_HDP_ESTEP, cp.FLAG_SMALL_FOOTPRINT)
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
    """the C-ABI reads no variable for this flag (libcpecan_host.so has CPECAN_HDP_FUSED_ESTEP for its own batches)"""
    for k in ("CPECAN_HDP_FUSED_ESTEP", "CPECAN_EXPECT_FUSED", "CPECAN_EXPECT_FUSED_WORKGROUP",
              "CPECAN_EXPECT_FUSED_WIDE"):
        monkeypatch.setenv(k, "1")
    for w in WIDTHS:
        assert fused(flags=0, width=w) == 0, w
    source = open(os.path.join(ROOT, "cpecan-signal_amd", "csrc", "cpecan_hip.hip")).read()
    assert "CPECAN_HDP_FUSED_ESTEP" not in source
    host = open(os.path.join(ROOT, "cpecan-signal_amd", "csrc", "host", "cpecan_api.c")).read()
    assert 'getenv("CPECAN_HDP_FUSED_ESTEP")' in host

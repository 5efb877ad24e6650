"""CPECAN_FLAG_HDP_FOUR_CELLS_FUSED_ESTEP (262144) through cpecan_hip_plan_expectation_pass and
cpecan_hip_plan_dispatch (the answers of choose_dispatch in cpecan_hip.hip): no device.

Every expected value is a literal from include/cpecan_hip.h: an HDP batch of expectations on the wave kernels at four
cells per lane -- a widest band of 185..248 k-mers, or a narrower one that CPECAN_SYSTOLIC_ROWS=4 puts there, edges
stepping by one, no CPECAN_FLAG_GENERAL_KERNEL -- sums its expectations inside the sweep back (_hf4) when it carries the
flag and keeps the ring of backward cells (_h4) when it does not.  The flag means nothing to a posterior batch, to
another machine, to an HDP E-step at two or three cells per lane (where 65536 rules, and means nothing at four), on the
_he / _hf workgroup builds, past 248 k-mers or on the general kernel; CPECAN_EXPECT_FUSED=0 does not undo it, and
cpecan_hip_plan_dispatch answers the same kernel, family, rows and widest band with and without it."""
import os
import re

import pytest

from cpecan_load import ROOT, binding
from harness import BATCH_ENV

cp = binding()

FOUR = 262144
NARROW = 65536                            # CPECAN_FLAG_HDP_FUSED_ESTEP: two and three cells per lane
WIDE_FUSED = 131072                       # CPECAN_FLAG_WIDE_BANDS_HDP_FUSED_ESTEP: the _hf6 / _hf8 workgroup builds
SM, DNA, VAN, HDP, SM4, ECH = (cp.MACHINE_STRAWMAN, cp.MACHINE_DNA5, cp.MACHINE_VANILLA, cp.MACHINE_HDP,
                               cp.MACHINE_SM4, cp.MACHINE_ECHELON)
MACHINES = (SM, DNA, VAN, HDP, SM4, ECH)
POST, EXP = cp.MODE_POSTERIOR, cp.MODE_EXPECTATIONS
AUTO, GEN, SYS = cp.KERNEL_AUTO, cp.KERNEL_GENERAL, cp.KERNEL_SYSTOLIC
GENK, WIDE_HE, WIDE_VE = cp.FLAG_GENERAL_KERNEL, cp.FLAG_WIDE_BANDS_HDP_ESTEP, cp.FLAG_WIDE_BANDS_VANILLA_ESTEP
NARROWER = (1, 56, 57, 120, 121, 184)    # the ground of _h2 / _h3 by themselves
FOUR_CELLS = (185, 248)                   # ... and of _h4 / _hf4
PAST = (249, 504, 505)                    # the general kernel's, or with the wide-bands flag the _he builds'
WIDTHS = NARROWER + FOUR_CELLS + PAST
# every flag a create call takes but this one, by its value in include/cpecan_hip.h
OTHER_FLAGS = dict(DEBUG_DUMP=1, UNBANDED=2, SCAN_DECODE=4, EXPECTATIONS=8, WORKGROUP_KERNELS=16, GENERAL_KERNEL=32,
                   SMALL_FOOTPRINT=64, WIDE_BANDS=128, WIDE_BANDS_HDP=256, WIDE_BANDS_HDP_ESTEP=512,
                   WIDE_BANDS_VANILLA_ESTEP=1024, WORKGROUP_FUSED_ESTEP=2048, WIDE_BANDS_FUSED_ESTEP=4096,
                   ASM_NARROW_BANDS=8192, VANILLA_FUSED_ESTEP=16384, WIDE_BANDS_VANILLA_FUSED_ESTEP=32768,
                   HDP_FUSED_ESTEP=65536, WIDE_BANDS_HDP_FUSED_ESTEP=131072)


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in BATCH_ENV:
        monkeypatch.delenv(k, raising=False)


def fused(machine=HDP, mode=EXP, kernel=AUTO, flags=FOUR, width=200, edges=True):
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
    assert re.search(r"#define CPECAN_FLAG_HDP_FOUR_CELLS_FUSED_ESTEP %d\b" % FOUR, header)
    assert cp.FLAG_HDP_FOUR_CELLS_FUSED_ESTEP == FOUR
    others = dict((k[5:], v) for k, v in vars(cp).items()
                  if k.startswith("FLAG_") and k != "FLAG_HDP_FOUR_CELLS_FUSED_ESTEP")
    assert others.items() >= OTHER_FLAGS.items()
    assert not any(v & FOUR for v in others.values())   # a number of its own: no other flag has the bit
    for name, value in re.findall(r"#define (CPECAN_FLAG_\w+) (\d+)\b", header):
        assert name == "CPECAN_FLAG_HDP_FOUR_CELLS_FUSED_ESTEP" or not int(value) & FOUR, name


@pytest.mark.parametrize("kernel", [AUTO, GEN, SYS])  # the HDP create call has no kernel argument: any value
def test_the_flag_alone_at_four_cells(kernel):
    for w in FOUR_CELLS:
        assert fused(kernel=kernel, width=w) == 1, w
        assert fused(kernel=kernel, flags=0, width=w) == 0, w
        assert fused(kernel=kernel, flags=NARROW, width=w) == 0, w      # 65536 keeps meaning nothing on _h4
        assert fused(kernel=kernel, flags=NARROW | FOUR, width=w) == 1, w
        assert answer(HDP, EXP, kernel, FOUR, w, True) == sweep(1, 4, 248) == answer(HDP, EXP, kernel, 0, w, True), w


def test_a_narrower_band_forced_onto_four_cells(monkeypatch):
    monkeypatch.setenv("CPECAN_SYSTOLIC_ROWS", "4")
    for w in NARROWER + FOUR_CELLS:
        assert answer(HDP, EXP, AUTO, FOUR, w, True) == sweep(1, 4, 248) == answer(HDP, EXP, AUTO, 0, w, True), w
        assert fused(width=w) == 1, w
        assert fused(flags=0, width=w) == 0, w
        assert fused(flags=NARROW, width=w) == 0, w                     # ... one forced there included
        assert fused(flags=NARROW | FOUR, width=w) == 1, w


def test_two_and_three_cells_are_the_other_flags(monkeypatch):
    """by themselves bands up to 184 k-mers land on _h2 / _h3: this flag alone leaves them the ring, both flags fuse"""
    for w, rows, reach in ((1, 2, 120), (56, 2, 120), (57, 2, 120), (120, 2, 120), (121, 3, 184), (184, 3, 184)):
        assert answer(HDP, EXP, AUTO, FOUR, w, True) == sweep(1, rows, reach) == answer(HDP, EXP, AUTO, 0, w, True), w
        assert fused(width=w) == 0, w
        assert fused(flags=NARROW, width=w) == 1, w
        assert fused(flags=NARROW | FOUR, width=w) == 1, w
    monkeypatch.setenv("CPECAN_SYSTOLIC_ROWS", "3")
    for w in (1, 56, 57, 120):
        assert answer(HDP, EXP, AUTO, FOUR, w, True) == sweep(1, 3, 184), w
        assert fused(width=w) == 0, w
        assert fused(flags=NARROW | FOUR, width=w) == 1, w


def test_without_the_flag_nothing_changes(monkeypatch):
    """an HDP batch of expectations keeps the ring whatever CPECAN_EXPECT_FUSED says"""
    for value in (None, "1", "0"):
        if value is not None:
            monkeypatch.setenv("CPECAN_EXPECT_FUSED", value)
        for rows in (None, "4"):
            if rows is not None:
                monkeypatch.setenv("CPECAN_SYSTOLIC_ROWS", rows)
            for w in WIDTHS:
                for edges in (True, False):
                    assert fused(flags=0, width=w, edges=edges) == 0, (value, rows, w, edges)
                    assert fused(flags=WIDE_HE, width=w, edges=edges) == 0, (value, rows, w, edges)
        monkeypatch.delenv("CPECAN_SYSTOLIC_ROWS")


def test_the_ring_variable_does_not_undo_the_flag(monkeypatch):
    for value in ("0", "1"):
        monkeypatch.setenv("CPECAN_EXPECT_FUSED", value)
        for w in WIDTHS:
            assert fused(width=w) == (1 if 185 <= w <= 248 else 0), (value, w)
            assert fused(flags=0, width=w) == 0, (value, w)
        monkeypatch.setenv("CPECAN_SYSTOLIC_ROWS", "4")
        for w in NARROWER + FOUR_CELLS:
            assert fused(width=w) == 1, (value, w)
            assert fused(flags=0, width=w) == 0, (value, w)
        monkeypatch.delenv("CPECAN_SYSTOLIC_ROWS")


def test_the_flag_means_nothing_past_four_cells(monkeypatch):
    """past 248 k-mers the general kernel, or with the wide-bands flag of the E-step (or its variable) the _he builds and,
    under their own flag, the _hf6 / _hf8 builds: with and without that flag and that variable this one changes nothing"""
    for w in PAST:
        assert answer(HDP, EXP, AUTO, FOUR, w, True)["kernel"] == GEN, w
        assert fused(width=w) == 0, w
    for by_env in (False, True):
        wide = 0 if by_env else WIDE_HE
        if by_env:
            monkeypatch.setenv("CPECAN_WIDE_BANDS_HDP_ESTEP", "1")
        for w, rows, reach in ((249, 6, 376), (376, 6, 376), (377, 8, 504), (504, 8, 504)):
            assert answer(HDP, EXP, AUTO, FOUR | wide, w, True) == sweep(0, rows, reach), w
            assert fused(flags=FOUR | wide, width=w) == 0, w
            assert fused(flags=FOUR | wide | WIDE_FUSED, width=w) == 1 == fused(flags=wide | WIDE_FUSED, width=w), w
        assert fused(flags=FOUR | wide, width=505) == 0
        assert fused(flags=FOUR | wide | WIDE_FUSED, width=505) == 0
        assert answer(HDP, EXP, AUTO, FOUR | wide, 505, True)["kernel"] == GEN
        # a band the four-cell build holds is left to it, and to the flag
        for w in FOUR_CELLS:
            assert answer(HDP, EXP, AUTO, FOUR | wide, w, True) == sweep(1, 4, 248), w
            assert fused(flags=FOUR | wide, width=w) == 1, w
            assert fused(flags=wide, width=w) == 0, w
            assert fused(flags=wide | WIDE_FUSED, width=w) == 0, w


def test_the_flag_means_nothing_to_the_general_kernel(monkeypatch):
    for rows in (None, "4"):
        if rows is not None:
            monkeypatch.setenv("CPECAN_SYSTOLIC_ROWS", rows)
        for w in WIDTHS:
            assert fused(flags=FOUR | GENK, width=w) == 0, w
            assert answer(HDP, EXP, AUTO, FOUR | GENK, w, True)["kernel"] == GEN
            assert fused(width=w, edges=False) == 0, w               # (such a band is the general kernel's)
            assert answer(HDP, EXP, AUTO, FOUR, w, False)["kernel"] == GEN


@pytest.mark.parametrize("machine", MACHINES)
def test_the_flag_means_nothing_to_a_posterior_batch_or_another_machine(machine, monkeypatch):
    for rows in (None, "4"):
        if rows is not None:
            monkeypatch.setenv("CPECAN_SYSTOLIC_ROWS", rows)
        for mode in (POST, EXP):
            for kernel in (AUTO, GEN, SYS):
                for w in WIDTHS:
                    for edges in (True, False):
                        without = cp.plan_expectation_pass(machine, mode, kernel, 0, w, edges)
                        with_flag = cp.plan_expectation_pass(machine, mode, kernel, FOUR, w, edges)
                        four = w <= 248 if rows else 185 <= w <= 248
                        serves = machine == HDP and mode == EXP and four and edges
                        assert with_flag == (1 if serves else without), (rows, mode, kernel, w, edges)
                        if machine != SM:
                            assert without == 0, (rows, mode, kernel, w, edges)
    monkeypatch.delenv("CPECAN_SYSTOLIC_ROWS")
    # the strawMan machine's own fused E-step is as it was, with the bit and without
    if machine == SM:
        assert fused(machine=SM, flags=FOUR, width=200) == 1 == fused(machine=SM, flags=0, width=200)
        monkeypatch.setenv("CPECAN_EXPECT_FUSED", "0")
        assert fused(machine=SM, flags=FOUR, width=200) == 0


@pytest.mark.parametrize("name", sorted(OTHER_FLAGS))
def test_beside_every_other_flag(name):
    """the other flag does to an HDP E-step what it does alone (it moves the batch to the general kernel, refuses it,
    fuses it on its own builds or means nothing); where the batch stays on the four-cell wave build this flag fuses it,
    and nowhere else"""
    other = OTHER_FLAGS[name]
    for w in WIDTHS:
        for edges in (True, False):
            alone = answer(HDP, EXP, AUTO, other, w, edges)
            assert answer(HDP, EXP, AUTO, other | FOUR, w, edges) == alone, (w, edges)
            served = isinstance(alone, dict) and alone["kernel"] == SYS and alone["wave"] == 1 and alone["rows"] == 4
            by_other = fused(flags=other, width=w, edges=edges)
            assert fused(flags=other | FOUR, width=w, edges=edges) == (1 if served else by_other), (w, edges)
            if name not in ("HDP_FUSED_ESTEP", "WIDE_BANDS_HDP_FUSED_ESTEP"):
                assert by_other == 0, (w, edges)
    if name in ("UNBANDED", "DEBUG_DUMP"):   # refused as without the flag, with the same text
        assert isinstance(answer(HDP, EXP, AUTO, other | FOUR, 200, True), tuple)
    if name == "GENERAL_KERNEL":
        assert answer(HDP, EXP, AUTO, other | FOUR, 200, True)["kernel"] == GEN
    if name == "HDP_FUSED_ESTEP":            # both flags: fused at two, three and four cells
        for w in NARROWER + FOUR_CELLS:
            assert fused(flags=other | FOUR, width=w) == 1, w
            assert fused(flags=other, width=w) == (1 if w <= 184 else 0), w


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
        for rows in (None, "4"):
            if rows is not None:
                monkeypatch.setenv("CPECAN_SYSTOLIC_ROWS", rows)
            for kernel in (AUTO, GEN, SYS):
                for flags in flag_sets:
                    for w in WIDTHS:
                        for edges in (True, False):
                            q = (machine, mode, kernel, flags, w, edges)
                            assert answer(machine, mode, kernel, flags | FOUR, w, edges) == answer(*q), (rows, q)
        monkeypatch.delenv("CPECAN_SYSTOLIC_ROWS")


def test_no_variable_of_batch_creation_sets_it(monkeypatch):
    """the C-ABI reads no variable for this flag (libcpecan_host.so has CPECAN_HDP_FOUR_CELLS_FUSED_ESTEP for its own
    batches)"""
    for k in ("CPECAN_HDP_FOUR_CELLS_FUSED_ESTEP", "CPECAN_HDP_FUSED_ESTEP", "CPECAN_WIDE_BANDS_HDP_FUSED_ESTEP",
              "CPECAN_EXPECT_FUSED", "CPECAN_EXPECT_FUSED_WORKGROUP", "CPECAN_EXPECT_FUSED_WIDE"):
        monkeypatch.setenv(k, "1")
    for rows in (None, "4"):
        if rows is not None:
            monkeypatch.setenv("CPECAN_SYSTOLIC_ROWS", rows)
        for w in WIDTHS:
            assert fused(flags=0, width=w) == 0, w
    source = open(os.path.join(ROOT, "cpecan-signal_amd", "csrc", "cpecan_hip.hip")).read()
    assert "CPECAN_HDP_FOUR_CELLS_FUSED_ESTEP" not in source
    host = open(os.path.join(ROOT, "cpecan-signal_amd", "csrc", "host", "cpecan_api.c")).read()
    assert 'getenv("CPECAN_HDP_FOUR_CELLS_FUSED_ESTEP")' in host

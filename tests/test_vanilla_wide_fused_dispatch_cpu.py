"""CPECAN_FLAG_WIDE_BANDS_VANILLA_FUSED_ESTEP (32768) through cpecan_hip_plan_expectation_pass and
cpecan_hip_plan_dispatch (the answers of choose_dispatch in cpecan_hip.hip): no device.

Every expected value is a literal from include/cpecan_hip.h: a vanilla batch of expectations that
CPECAN_FLAG_WIDE_BANDS_VANILLA_ESTEP (1024, or CPECAN_WIDE_BANDS_VANILLA_ESTEP=1) puts on the _ve workgroup builds -- a
widest band of 185..248 k-mers on four waves, 249..376 on six, 377..504 on eight, edges stepping by one, no
CPECAN_FLAG_GENERAL_KERNEL -- sums its expectations inside the sweep back when it carries the flag (_vf4 / _vf6 / _vf8) and
keeps the ring of backward cells when it does not.  The flag means nothing to a posterior batch, to another machine, to a
band of at most 184 k-mers (the wave builds, where 16384 rules) or past 504, to the general kernel and to a batch without
the wide-bands flag of the E-step; CPECAN_EXPECT_FUSED=0 does not undo it (the fused builds have no other form of the
E-step), and cpecan_hip_plan_dispatch answers the same kernel, family, rows and widest band with and without it."""
import os
import re

import pytest

from cpecan_load import ROOT, binding
from harness import BATCH_ENV
from test_vanilla_fused_dispatch_cpu import MACHINES, WIDTHS, answer, sweep
from test_vanilla_fused_dispatch_cpu import OTHER_FLAGS as OLDER_FLAGS

cp = binding()

WIDE_FUSED = 32768
WAVE_FUSED = 16384
SM, VAN = cp.MACHINE_STRAWMAN, cp.MACHINE_VANILLA
POST, EXP = cp.MODE_POSTERIOR, cp.MODE_EXPECTATIONS
AUTO, GEN, SYS = cp.KERNEL_AUTO, cp.KERNEL_GENERAL, cp.KERNEL_SYSTOLIC
GENK, WIDE_VE = cp.FLAG_GENERAL_KERNEL, cp.FLAG_WIDE_BANDS_VANILLA_ESTEP
# (width, waves per workgroup, the build's widest band) on the ground of the _ve / _vf builds, and widths off it
GROUND = ((185, 4, 248), (248, 4, 248), (249, 6, 376), (376, 6, 376), (377, 8, 504), (504, 8, 504))
OFF = (1, 56, 120, 121, 184, 505)
# every flag a create call takes but this one, by its value in include/cpecan_hip.h
OTHER_FLAGS = dict(OLDER_FLAGS, VANILLA_FUSED_ESTEP=WAVE_FUSED)


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in BATCH_ENV:
        monkeypatch.delenv(k, raising=False)


def fused(machine=VAN, mode=EXP, kernel=AUTO, flags=WIDE_FUSED | WIDE_VE, width=300, edges=True):
    return cp.plan_expectation_pass(machine, mode, kernel, flags, width, edges)


def test_the_header_and_the_binding_name_the_flag():
    header = open(os.path.join(ROOT, "include", "cpecan_hip.h")).read()
    assert re.search(r"#define CPECAN_FLAG_WIDE_BANDS_VANILLA_FUSED_ESTEP %d\b" % WIDE_FUSED, header)
    assert cp.FLAG_WIDE_BANDS_VANILLA_FUSED_ESTEP == WIDE_FUSED
    others = dict((k[5:], v) for k, v in vars(cp).items()
                  if k.startswith("FLAG_") and k != "FLAG_WIDE_BANDS_VANILLA_FUSED_ESTEP")
    assert others.items() >= OTHER_FLAGS.items()
    assert not any(v & WIDE_FUSED for v in others.values())   # a number of its own: no other flag has the bit
    assert set(int(v) for v in re.findall(r"#define CPECAN_FLAG_\w+ (\d+)", header)) == set(others.values()) | {WIDE_FUSED}


@pytest.mark.parametrize("kernel", [AUTO, GEN, SYS])  # the vanilla create call has no kernel argument: any value
@pytest.mark.parametrize("by_env", [False, True], ids=["flag", "variable"])
def test_fused_on_the_ground_of_the_ve_builds(kernel, by_env, monkeypatch):
    wide = 0 if by_env else WIDE_VE
    if by_env:
        monkeypatch.setenv("CPECAN_WIDE_BANDS_VANILLA_ESTEP", "1")
    for w, rows, reach in GROUND:
        assert fused(kernel=kernel, flags=WIDE_FUSED | wide, width=w) == 1, w
        assert fused(kernel=kernel, flags=wide, width=w) == 0, w
        assert answer(VAN, EXP, kernel, WIDE_FUSED | wide, w, True) == sweep(0, rows, reach) \
            == answer(VAN, EXP, kernel, wide, w, True), w
    for w in OFF:
        assert fused(kernel=kernel, flags=WIDE_FUSED | wide, width=w) == 0, w
        assert answer(VAN, EXP, kernel, WIDE_FUSED | wide, w, True) == answer(VAN, EXP, kernel, wide, w, True), w
    assert answer(VAN, EXP, kernel, WIDE_FUSED | wide, 184, True) == sweep(1, 3, 184)
    assert answer(VAN, EXP, kernel, WIDE_FUSED | wide, 505, True)["kernel"] == GEN


def test_the_flag_alone_answers_nothing(monkeypatch):
    """without the wide-bands flag of the E-step the batch is the wave builds' or the general kernel's, whatever
    CPECAN_EXPECT_FUSED says"""
    for value in (None, "1", "0"):
        if value is not None:
            monkeypatch.setenv("CPECAN_EXPECT_FUSED", value)
        for w in WIDTHS + (247, 300, 377, 450):
            for edges in (True, False):
                assert fused(flags=WIDE_FUSED, width=w, edges=edges) == 0, (value, w, edges)
                assert answer(VAN, EXP, AUTO, WIDE_FUSED, w, edges) == answer(VAN, EXP, AUTO, 0, w, edges), (value, w, edges)
                assert fused(flags=0, width=w, edges=edges) == 0, (value, w, edges)
                assert fused(flags=WIDE_VE, width=w, edges=edges) == 0, (value, w, edges)


def test_both_fused_flags_on_both_sides_of_184():
    both = WAVE_FUSED | WIDE_FUSED | WIDE_VE
    for w in (1, 120, 121, 184) + tuple(g[0] for g in GROUND):
        assert fused(flags=both, width=w) == 1, w
    assert fused(flags=both, width=505) == 0
    assert answer(VAN, EXP, AUTO, both, 184, True) == sweep(1, 3, 184)
    assert answer(VAN, EXP, AUTO, both, 185, True) == sweep(0, 4, 248)
    # each flag on its own side only
    assert fused(flags=WAVE_FUSED | WIDE_VE, width=185) == 0 and fused(flags=WIDE_FUSED | WIDE_VE, width=184) == 0


def test_the_ring_variable_does_not_undo_the_flag(monkeypatch):
    for value in ("0", "1"):
        monkeypatch.setenv("CPECAN_EXPECT_FUSED", value)
        for w, _, _ in GROUND:
            assert fused(width=w) == 1, (value, w)
            assert fused(flags=WIDE_VE, width=w) == 0, (value, w)


def test_the_flag_means_nothing_to_the_general_kernel():
    for w in WIDTHS:
        assert fused(flags=WIDE_FUSED | WIDE_VE | GENK, width=w) == 0, w
        assert answer(VAN, EXP, AUTO, WIDE_FUSED | WIDE_VE | GENK, w, True)["kernel"] == GEN
        assert fused(width=w, edges=False) == 0, w               # (such a band is the general kernel's)
        assert answer(VAN, EXP, AUTO, WIDE_FUSED | WIDE_VE, w, False)["kernel"] == GEN


@pytest.mark.parametrize("machine", MACHINES)
def test_the_flag_means_nothing_to_a_posterior_batch_or_another_machine(machine, monkeypatch):
    """over the grid of test_vanilla_fused_dispatch_cpu.py: widths x edges x kernel, both modes, the flag alone and
    beside the wide-bands flag of the vanilla E-step"""
    for mode in (POST, EXP):
        for kernel in (AUTO, GEN, SYS):
            for w in WIDTHS:
                for edges in (True, False):
                    for base in (0, WIDE_VE):
                        without = cp.plan_expectation_pass(machine, mode, kernel, base, w, edges)
                        with_flag = cp.plan_expectation_pass(machine, mode, kernel, base | WIDE_FUSED, w, edges)
                        serves = machine == VAN and mode == EXP and base == WIDE_VE and 185 <= w <= 504 and edges
                        assert with_flag == (1 if serves else without), (mode, kernel, w, edges, base)
                        assert answer(machine, mode, kernel, base | WIDE_FUSED, w, edges) \
                            == answer(machine, mode, kernel, base, w, edges), (mode, kernel, w, edges, base)
                        if machine != SM:
                            assert without == 0, (mode, kernel, w, edges, base)
    # the strawMan machine's own fused E-step is as it was, with the bit and without
    if machine == SM:
        assert fused(machine=SM, flags=WIDE_FUSED, width=100) == 1 == fused(machine=SM, flags=0, width=100)
        monkeypatch.setenv("CPECAN_EXPECT_FUSED", "0")
        assert fused(machine=SM, flags=WIDE_FUSED, width=100) == 0


@pytest.mark.parametrize("name", sorted(OTHER_FLAGS))
def test_beside_every_other_flag(name):
    """the other flag does to a vanilla E-step what it does alone (it moves the batch to the general kernel or to the
    _ve builds, refuses it or means nothing); where the batch lands on the _ve builds this flag fuses it, and nowhere
    else -- 16384 still fuses the wave builds beside it"""
    other = OTHER_FLAGS[name]
    for base in (0, WIDE_VE):
        for w in WIDTHS:
            for edges in (True, False):
                alone = answer(VAN, EXP, AUTO, other | base, w, edges)
                assert answer(VAN, EXP, AUTO, other | base | WIDE_FUSED, w, edges) == alone, (w, edges, base)
                on_ve = isinstance(alone, dict) and alone["kernel"] == SYS and alone["wave"] == 0
                before = fused(flags=other | base, width=w, edges=edges)
                assert fused(flags=other | base | WIDE_FUSED, width=w, edges=edges) == (1 if on_ve else before), (w, edges, base)
                on_wave = isinstance(alone, dict) and alone["kernel"] == SYS and alone["wave"] == 1
                assert before == (1 if on_wave and name == "VANILLA_FUSED_ESTEP" else 0), (w, edges, base)
    if name in ("UNBANDED", "DEBUG_DUMP"):   # refused as without the flag, with the same text
        assert isinstance(answer(VAN, EXP, AUTO, other | WIDE_VE | WIDE_FUSED, 300, True), tuple)
    if name == "GENERAL_KERNEL":
        assert answer(VAN, EXP, AUTO, other | WIDE_VE | WIDE_FUSED, 300, True)["kernel"] == GEN
    if name == "WIDE_BANDS_VANILLA_ESTEP":
        assert fused(flags=other | WIDE_FUSED, width=300) == 1


@pytest.mark.parametrize("mode", [POST, EXP])
@pytest.mark.parametrize("machine", MACHINES)
def test_the_kernel_choice_does_not_move(machine, mode, monkeypatch):
    """cpecan_hip_plan_dispatch: the same kernel, family, rows and widest band -- or the same refusal with the same
    text -- with the bit, for every machine in both modes, under both families' defaults"""
    flag_sets = (0, cp.FLAG_WORKGROUP_KERNELS, cp.FLAG_WIDE_BANDS, GENK, WIDE_VE, cp.FLAG_UNBANDED, WAVE_FUSED | WIDE_VE,
                 cp.FLAG_WIDE_BANDS_HDP | cp.FLAG_WIDE_BANDS_HDP_ESTEP, cp.FLAG_SMALL_FOOTPRINT)
    for by_env in (False, True):
        if by_env:
            monkeypatch.setenv("CPECAN_KERNELS", "systolic")
        for kernel in (AUTO, GEN, SYS):
            for flags in flag_sets:
                for w in WIDTHS:
                    for edges in (True, False):
                        q = (machine, mode, kernel, flags, w, edges)
                        assert answer(machine, mode, kernel, flags | WIDE_FUSED, w, edges) == answer(*q), q


def test_no_variable_of_batch_creation_sets_it(monkeypatch):
    """the C-ABI reads no variable for this flag (libcpecan_host.so has CPECAN_WIDE_BANDS_VANILLA_FUSED_ESTEP for its own
    batches)"""
    for k in ("CPECAN_WIDE_BANDS_VANILLA_FUSED_ESTEP", "CPECAN_VANILLA_FUSED_ESTEP", "CPECAN_EXPECT_FUSED_WORKGROUP",
              "CPECAN_EXPECT_FUSED_WIDE"):
        monkeypatch.setenv(k, "1")
    for w in WIDTHS:
        assert fused(flags=0, width=w) == 0, w
        assert fused(flags=WIDE_VE, width=w) == 0, w
    source = open(os.path.join(ROOT, "cpecan-signal_amd", "csrc", "cpecan_hip.hip")).read()
    assert "CPECAN_WIDE_BANDS_VANILLA_FUSED_ESTEP" not in source
    host = open(os.path.join(ROOT, "cpecan-signal_amd", "csrc", "host", "cpecan_api.c")).read()
    assert 'getenv("CPECAN_WIDE_BANDS_VANILLA_FUSED_ESTEP")' in host

"""Which batches the assembly sweeps take, through cpecan_hip_plan_assembly_sweeps (the answer of choose_dispatch in
cpecan_hip.hip, no device): CPECAN_FLAG_ASM_NARROW_BANDS (8192) or CPECAN_ASM_NARROW=1 puts a strawMan posterior batch of
the wave kernels with a widest band of at most 120 k-mers on the two-cell sweeps; bands of 121..158 k-mers run the
three-cell ones as before; everything else runs what it runs without the flag, and cpecan_hip_plan_dispatch never moves."""
import re

import pytest

from cpecan_load import binding
from harness import BATCH_ENV

cp = binding()

NARROW = 8192
LIMIT = 120        # ASM2_MAX_WIDTH: the whole ground of the two-cell build
S, P, E = cp.MACHINE_STRAWMAN, cp.MODE_POSTERIOR, cp.MODE_EXPECTATIONS
OTHER_MACHINES = (cp.MACHINE_DNA5, cp.MACHINE_VANILLA, cp.MACHINE_HDP, cp.MACHINE_SM4, cp.MACHINE_ECHELON)
WIDTHS = (0, 1, 56, 57, 72, 102, LIMIT, LIMIT + 1, 140, 158, 159, 184, 185, 248, 249, 504, 505)


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in BATCH_ENV:
        monkeypatch.delenv(k, raising=False)


def cells(flags, width, machine=S, mode=P, kernel=cp.KERNEL_AUTO, edges=True):
    return cp.plan_assembly_sweeps(machine, mode, kernel, flags, width, edges)


def test_the_header_the_binding_and_the_generated_limit_agree():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "cpecan_hip.h")).read()
    assert re.search(r"#define CPECAN_FLAG_ASM_NARROW_BANDS %d\b" % NARROW, header)
    assert cp.FLAG_ASM_NARROW_BANDS == NARROW
    others = [v for k, v in vars(cp).items() if k.startswith("FLAG_") and k != "FLAG_ASM_NARROW_BANDS"]
    assert len(others) >= 13 and not any(v & NARROW for v in others)
    gen = open(os.path.join(root, "cpecan-signal_amd", "csrc", "cpecan_asm_gen.h")).read()
    assert "#define ASM2_MAX_WIDTH %d\n" % LIMIT in gen and "#define ASM_MAX_WIDTH 158\n" in gen
    assert LIMIT >= 103   # (an expansion of 50 around anchors every 50 columns: bands of 101-102 k-mers)


@pytest.mark.parametrize("by", ["flag", "variable"])
def test_the_flag_and_the_variable_each_give_two_cells_up_to_the_limit(by, monkeypatch):
    flags = NARROW if by == "flag" else 0
    if by == "variable":
        monkeypatch.setenv("CPECAN_ASM_NARROW", "1")
    for kernel in (cp.KERNEL_AUTO, cp.KERNEL_SYSTOLIC):
        for w in (1, 72, 102, LIMIT):
            assert cells(flags, w, kernel=kernel) == 2, w
            assert cells(flags | cp.FLAG_SMALL_FOOTPRINT, w, kernel=kernel) == 2, w
        for w in range(LIMIT + 1, 121):       # (just past the limit, while the two-cell build still holds the band)
            assert cells(flags, w, kernel=kernel) == 0, w
        for w in (121, 140, 158):
            assert cells(flags, w, kernel=kernel) == 3, w
        for w in (159, 184, 185, 248):
            assert cells(flags, w, kernel=kernel) == 0, w
    assert cells(flags, 72, kernel=cp.KERNEL_GENERAL) == 0
    assert cells(flags, 72, edges=False) == 0            # (such a band is the general kernel's)


def test_any_other_value_of_the_variable_is_no_request(monkeypatch):
    for value in ("0", "2", ""):
        monkeypatch.setenv("CPECAN_ASM_NARROW", value)
        assert [cells(0, w) for w in (1, 72, LIMIT, 121)] == [0, 0, 0, 3], value


def test_without_the_flag_todays_answers(monkeypatch):
    for w in WIDTHS:
        assert cells(0, w) == (3 if 121 <= w <= 158 else 0), w
        assert cells(cp.FLAG_SMALL_FOOTPRINT, w) == (3 if 121 <= w <= 158 else 0), w


@pytest.mark.parametrize("by", ["flag", "variable"])
def test_everything_the_flag_means_nothing_to(by, monkeypatch):
    flags = NARROW if by == "flag" else 0
    if by == "variable":
        monkeypatch.setenv("CPECAN_ASM_NARROW", "1")
    for w in WIDTHS:
        for machine in OTHER_MACHINES:
            for mode in (P, E):
                assert cells(flags, w, machine=machine, mode=mode) == 0, (machine, mode, w)
        assert cells(flags, w, mode=E) == 0, w                                    # a strawMan batch of expectations
        assert cells(flags | cp.FLAG_WORKGROUP_KERNELS, w) == 0, w                # the workgroup family, by flag ...
        assert cells(flags | cp.FLAG_WIDE_BANDS, w) == cells(flags, w), w
    monkeypatch.setenv("CPECAN_KERNELS", "systolic")                              # ... and by the environment
    assert [cells(flags, w) for w in WIDTHS] == [0] * len(WIDTHS)
    monkeypatch.delenv("CPECAN_KERNELS")
    monkeypatch.setenv("CPECAN_ASM", "0")                                         # every batch on the compiled kernels
    assert [cells(flags, w) for w in WIDTHS] == [0] * len(WIDTHS)
    monkeypatch.setenv("CPECAN_ASM", "1")   # (the forward sweep alone, a test aid of the three-cell sweeps: not at two)
    assert [cells(flags, w) for w in (72, LIMIT, 121)] == [0, 0, 3]


def test_the_kernel_choice_does_not_move(monkeypatch):
    """cpecan_hip_plan_dispatch: the same kernel, family, build and widest band -- or the same refusal -- with the bit"""
    def answer(*q):
        try:
            return cp.plan_dispatch(*q)
        except cp.CpecanError as err:
            return (err.code, str(err))

    for by_env in (False, True):
        if by_env:
            monkeypatch.setenv("CPECAN_ASM_NARROW", "1")
        for machine in (S,) + OTHER_MACHINES:
            for mode in (P, E):
                for kernel in (cp.KERNEL_AUTO, cp.KERNEL_GENERAL, cp.KERNEL_SYSTOLIC):
                    for flags in (0, cp.FLAG_WORKGROUP_KERNELS, cp.FLAG_WIDE_BANDS, cp.FLAG_GENERAL_KERNEL, cp.FLAG_SMALL_FOOTPRINT):
                        for w in WIDTHS:
                            for edges in (True, False):
                                q = (machine, mode, kernel, flags, w, edges)
                                assert answer(*q[:3], flags | NARROW, w, edges) == answer(*q), q


def test_a_refused_combination_answers_zero():
    assert cp.plan_assembly_sweeps(S, P, cp.KERNEL_SYSTOLIC, NARROW | cp.FLAG_UNBANDED, 72, True) == 0
    assert cp.plan_assembly_sweeps(17, P, cp.KERNEL_AUTO, NARROW, 72, True) == 0

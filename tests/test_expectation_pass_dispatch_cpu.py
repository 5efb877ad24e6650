"""The form of the E-step as batch creation chooses it (Dispatch::fused, choose_dispatch in cpecan_hip.hip) through
cpecan_hip_plan_expectation_pass, against the rules include/cpecan_hip.h states for cpecan_hip_batch_expectation_pass:
1 for a strawMan batch of expectations on the wave kernels (unless CPECAN_EXPECT_FUSED=0) and, with the flag or the
variable of their range, on the workgroup kernels' fused builds (which have no other form); 0 for everything else, and
0 with the refusal's text for what creation refuses.  With it: the list of variables the tests of the choice clear
(harness.BATCH_ENV) against the source, and the functions behind read_batch_env that read no environment.  No device."""
import os
import re

import pytest

from cpecan_load import ROOT, binding
from harness import BATCH_ENV

cp = binding()

S = cp.MACHINE_STRAWMAN
POST, EXPECT = cp.MODE_POSTERIOR, cp.MODE_EXPECTATIONS
AUTO, GENERAL, SYSTOLIC = cp.KERNEL_AUTO, cp.KERNEL_GENERAL, cp.KERNEL_SYSTOLIC
WG, WIDE = cp.FLAG_WORKGROUP_KERNELS, cp.FLAG_WIDE_BANDS
FUSED_WG, FUSED_WIDE = cp.FLAG_WORKGROUP_FUSED_ESTEP, cp.FLAG_WIDE_BANDS_FUSED_ESTEP
# both sides of the widest band of every build: one to four waves or cells (56, 120, 184, 248), six and eight waves
NARROW_WIDTHS = (1, 56, 57, 120, 121, 184, 185, 248)   # the wave family's, and _r1 .. _r4's
WIDE_WIDTHS = (249, 376, 377, 504)                     # _r6 and _r8's
PAST = 505
SOURCE = os.path.join(ROOT, "cpecan-signal_amd", "csrc", "cpecan_hip.hip")


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in BATCH_ENV:
        monkeypatch.delenv(k, raising=False)


def fused(machine=S, mode=EXPECT, kernel=AUTO, flags=0, width=100, edges=True):
    return cp.plan_expectation_pass(machine, mode, kernel, flags, width, edges)


def rows(flags, width, kernel=AUTO):
    """(wave, rows) of the build cpecan_hip_plan_dispatch names: the test's inputs are of the class they were chosen for"""
    d = cp.plan_dispatch(S, EXPECT, kernel, flags, width, True)
    return d["wave"], d["rows"]


def last_error():
    return cp.lib().cpecan_hip_last_error().decode()


@pytest.mark.parametrize("kernel", [AUTO, SYSTOLIC])
@pytest.mark.parametrize("width", NARROW_WIDTHS)
def test_wave_family_sums_inside_the_sweep_back(width, kernel, monkeypatch):
    assert rows(0, width, kernel)[0] == 1
    assert fused(kernel=kernel, width=width) == 1
    # neither fused flag of the workgroup kernels, nor the wide-bands flag, means anything here
    for flags in (FUSED_WG, FUSED_WIDE, WIDE, WIDE | FUSED_WIDE):
        assert fused(kernel=kernel, flags=flags, width=width) == 1, flags
    monkeypatch.setenv("CPECAN_EXPECT_FUSED", "0")
    assert fused(kernel=kernel, width=width) == 0
    monkeypatch.setenv("CPECAN_EXPECT_FUSED", "1")
    assert fused(kernel=kernel, width=width) == 1


@pytest.mark.parametrize("family", ["by-flag", "by-variable"])
@pytest.mark.parametrize("width", NARROW_WIDTHS)
def test_workgroup_builds_of_one_to_four_waves(width, family, monkeypatch):
    flags = WG if family == "by-flag" else 0
    if family == "by-variable":
        monkeypatch.setenv("CPECAN_KERNELS", "systolic")
    assert rows(flags, width) == (0, 1 + (width > 56) + (width > 120) + (width > 184))
    assert fused(flags=flags, width=width) == 0
    assert fused(flags=flags | FUSED_WIDE, width=width) == 0       # the other range's flag
    assert fused(flags=flags | WIDE | FUSED_WIDE, width=width) == 0
    assert fused(flags=flags | FUSED_WG, width=width) == 1
    assert rows(flags | FUSED_WG, width) == rows(flags, width)
    monkeypatch.setenv("CPECAN_EXPECT_FUSED_WIDE", "1")
    assert fused(flags=flags, width=width) == 0
    monkeypatch.delenv("CPECAN_EXPECT_FUSED_WIDE")
    monkeypatch.setenv("CPECAN_EXPECT_FUSED_WORKGROUP", "1")
    assert fused(flags=flags, width=width) == 1
    monkeypatch.setenv("CPECAN_EXPECT_FUSED_WORKGROUP", "0")
    assert fused(flags=flags, width=width) == 0
    # the fused builds have no other form of the E-step
    monkeypatch.setenv("CPECAN_EXPECT_FUSED", "0")
    assert fused(flags=flags | FUSED_WG, width=width) == 1
    assert fused(flags=flags, width=width) == 0


@pytest.mark.parametrize("family", [0, WG], ids=["wave-default", "workgroup-default"])
@pytest.mark.parametrize("width", WIDE_WIDTHS)
def test_workgroup_builds_of_six_and_eight_waves(width, family, monkeypatch):
    flags = WIDE | family
    assert rows(flags, width) == (0, 6 if width <= 376 else 8)
    assert fused(flags=flags, width=width) == 0
    assert fused(flags=flags | FUSED_WG, width=width) == 0         # the other range's flag
    assert fused(flags=flags | FUSED_WIDE, width=width) == 1
    assert rows(flags | FUSED_WIDE, width) == rows(flags, width)
    # without the wide-bands flag there is no such build to stand in for: the general kernel
    assert fused(flags=family | FUSED_WIDE, width=width) == 0
    monkeypatch.setenv("CPECAN_EXPECT_FUSED_WORKGROUP", "1")
    assert fused(flags=flags, width=width) == 0
    monkeypatch.delenv("CPECAN_EXPECT_FUSED_WORKGROUP")
    monkeypatch.setenv("CPECAN_EXPECT_FUSED_WIDE", "1")
    assert fused(flags=flags, width=width) == 1
    assert fused(flags=family, width=width) == 0
    monkeypatch.setenv("CPECAN_EXPECT_FUSED", "0")
    assert fused(flags=flags, width=width) == 1
    monkeypatch.delenv("CPECAN_EXPECT_FUSED_WIDE")
    assert fused(flags=flags | FUSED_WIDE, width=width) == 1
    assert fused(flags=flags, width=width) == 0


def test_wide_bands_by_variable(monkeypatch):
    monkeypatch.setenv("CPECAN_WIDE_BANDS", "1")
    for width in WIDE_WIDTHS:
        assert fused(width=width) == 0 and fused(flags=FUSED_WIDE, width=width) == 1, width


ALL_FLAGS = (0, WG, WIDE, FUSED_WG, FUSED_WIDE, WG | FUSED_WG, WIDE | FUSED_WIDE, WG | WIDE | FUSED_WG | FUSED_WIDE)


def test_posterior_batches_have_no_expectation_pass(monkeypatch):
    for by_env in (False, True):
        if by_env:
            monkeypatch.setenv("CPECAN_EXPECT_FUSED_WORKGROUP", "1")
            monkeypatch.setenv("CPECAN_EXPECT_FUSED_WIDE", "1")
        for kernel in (AUTO, GENERAL, SYSTOLIC):
            for flags in ALL_FLAGS:
                for width in NARROW_WIDTHS + WIDE_WIDTHS + (PAST,):
                    assert fused(mode=POST, kernel=kernel, flags=flags, width=width) == 0, (kernel, flags, width)


@pytest.mark.parametrize("machine", [cp.MACHINE_DNA5, cp.MACHINE_VANILLA, cp.MACHINE_HDP, cp.MACHINE_SM4, cp.MACHINE_ECHELON])
def test_every_other_machine(machine, monkeypatch):
    own = cp.FLAG_WIDE_BANDS_HDP | cp.FLAG_WIDE_BANDS_HDP_ESTEP | cp.FLAG_WIDE_BANDS_VANILLA_ESTEP
    for by_env in (False, True):
        if by_env:
            monkeypatch.setenv("CPECAN_EXPECT_FUSED_WORKGROUP", "1")
            monkeypatch.setenv("CPECAN_EXPECT_FUSED_WIDE", "1")
        for mode in (POST, EXPECT):
            for flags in ALL_FLAGS + (own, own | WIDE | FUSED_WG | FUSED_WIDE):
                for width in NARROW_WIDTHS + WIDE_WIDTHS + (PAST,):
                    assert fused(machine, mode, AUTO, flags, width) == 0, (mode, flags, width)


def test_general_kernel_and_past_the_widest_build():
    for flags in ALL_FLAGS:
        for width in NARROW_WIDTHS + WIDE_WIDTHS + (PAST,):
            assert fused(kernel=GENERAL, flags=flags, width=width) == 0, (flags, width)
            assert fused(flags=flags | cp.FLAG_DEBUG_DUMP, width=width) == 0, (flags, width)   # (dumps: the general kernel)
            assert fused(flags=flags, width=width, edges=False) == 0, (flags, width)          # (ragged edges: the same)
        assert fused(flags=flags, width=PAST) == 0, flags
        assert cp.plan_dispatch(S, EXPECT, AUTO, flags, PAST, True)["kernel"] == GENERAL
    assert fused(width=249) == 0 and fused(flags=WG, width=249) == 0


REFUSED = [
    (S, EXPECT, SYSTOLIC, WIDE | FUSED_WIDE, PAST, True),       # no build is that wide
    (S, EXPECT, SYSTOLIC, FUSED_WG | WG, 249, True),
    (S, EXPECT, SYSTOLIC, 0, 100, False),                      # edges that jump
    (S, EXPECT, SYSTOLIC, cp.FLAG_DEBUG_DUMP, 100, True),
    (S, EXPECT, AUTO, cp.FLAG_UNBANDED, 100, True),
    (S, 7, AUTO, 0, 100, True),                                # no such mode
    (cp.MACHINE_SM4, EXPECT, AUTO, 0, 100, True),
    (cp.MACHINE_ECHELON, EXPECT, AUTO, FUSED_WG, 100, True),
    (cp.MACHINE_VANILLA, EXPECT, AUTO, cp.FLAG_UNBANDED, 100, True),
    (cp.MACHINE_HDP, POST, AUTO, cp.FLAG_DEBUG_DUMP, 100, True),
    (17, EXPECT, AUTO, 0, 100, True),
    (S, EXPECT, AUTO, 0, -1, True),
]


@pytest.mark.parametrize("q", REFUSED, ids=lambda q: "-".join(str(int(v)) for v in q))
def test_a_refused_combination_gives_0_and_the_refusal(q):
    with pytest.raises(cp.CpecanError) as ei:
        cp.plan_dispatch(*q)
    assert fused(S, EXPECT, AUTO, 0, 100) == 1                  # (an answer in between: the text below is this call's)
    assert fused(*q) == 0
    assert last_error() and str(ei.value).endswith(last_error()), (str(ei.value), last_error())


# ---------------------------------------- the source behind the plan calls ----------------------------------------
def body(name):
    """the text of the function `name` of cpecan_hip.hip, from its (static) definition to its closing brace"""
    text = open(SOURCE).read()
    m = re.search(r"^static [^\n;]*\b%s\(" % name, text, re.M)
    assert m, name
    return text[m.start():text.index("\n}\n", m.start())]


def test_the_cleared_variables_are_the_ones_batch_creation_reads():
    read = re.findall(r'getenv\("(CPECAN_[A-Z0-9_]+)"\)', body("read_batch_env"))
    assert len(set(BATCH_ENV)) == len(BATCH_ENV)
    assert set(read) == set(BATCH_ENV), set(read) ^ set(BATCH_ENV)


@pytest.mark.parametrize("name", ["choose_dispatch", "build_asm_plan", "build_bands", "plan_bands", "new_batch",
                                  "sweep_storage"])
def test_the_choice_and_the_storage_read_no_environment(name):
    assert "getenv" not in body(name), name

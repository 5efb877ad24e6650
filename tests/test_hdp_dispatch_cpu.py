"""The kernel choice of an HDP batch with CPECAN_FLAG_WIDE_BANDS_HDP / CPECAN_WIDE_BANDS_HDP=1 (choose_dispatch in
cpecan_hip.hip) through cpecan_hip_plan_dispatch: no device.

Every expected value is a literal from include/cpecan_hip.h, not read from the tables under test: the HDP wave builds
take bands up to 120, 184 and 248 k-mers (2, 3, 4 cells per lane); with the flag a posterior batch whose widest band is
249..376 k-mers runs on the six-wave HDP build of the workgroup family, one of 377..504 on the eight-wave build; past
504, on edges that step by more than one k-mer, un-banded, with CPECAN_FLAG_GENERAL_KERNEL and for the E-step the batch
stays on the general kernel.  The flag means nothing to the other machines, and CPECAN_FLAG_WIDE_BANDS nothing to this
one (tests/test_dispatch_cpu.py)."""
import pytest

from cpecan_load import binding
from harness import BATCH_ENV

cp = binding()

SM, DNA, VAN, HDP, SM4, ECH = (cp.MACHINE_STRAWMAN, cp.MACHINE_DNA5, cp.MACHINE_VANILLA, cp.MACHINE_HDP,
                               cp.MACHINE_SM4, cp.MACHINE_ECHELON)
POST, EXP = cp.MODE_POSTERIOR, cp.MODE_EXPECTATIONS
AUTO, GEN, SYS = cp.KERNEL_AUTO, cp.KERNEL_GENERAL, cp.KERNEL_SYSTOLIC
UNB, GENK, WIDE = cp.FLAG_UNBANDED, cp.FLAG_GENERAL_KERNEL, cp.FLAG_WIDE_BANDS
GENERAL = dict(kernel=GEN, wave=0, rows=0, build_max_width=0)


def sweep(wave, rows, width):
    return dict(kernel=SYS, wave=wave, rows=rows, build_max_width=width)


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in BATCH_ENV:
        monkeypatch.delenv(k, raising=False)


def plan(machine, mode=POST, kernel=AUTO, flags=0, width=100, edges=True):
    return cp.plan_dispatch(machine, mode, kernel, flags, width, edges)


def test_the_flag_is_256():
    assert cp.FLAG_WIDE_BANDS_HDP == 256


@pytest.mark.parametrize("by_env", [False, True])
@pytest.mark.parametrize("kernel", [AUTO, GEN, SYS])  # the HDP create call has no kernel argument: whatever is passed
def test_hdp_wide_builds(by_env, kernel, monkeypatch):
    flags = 0
    if by_env:
        monkeypatch.setenv("CPECAN_WIDE_BANDS_HDP", "1")
    else:
        flags = 256
    assert plan(HDP, POST, kernel, flags, 249) == sweep(0, 6, 376)
    assert plan(HDP, POST, kernel, flags, 376) == sweep(0, 6, 376)
    assert plan(HDP, POST, kernel, flags, 377) == sweep(0, 8, 504)
    assert plan(HDP, POST, kernel, flags, 504) == sweep(0, 8, 504)
    # a band the wave builds hold is left to them
    assert plan(HDP, POST, kernel, flags, 248) == sweep(1, 4, 248)
    assert plan(HDP, POST, kernel, flags, 184) == sweep(1, 3, 184)
    assert plan(HDP, POST, kernel, flags, 100) == sweep(1, 2, 120)
    assert plan(HDP, POST, kernel, flags, 505) == GENERAL


@pytest.mark.parametrize("by_env", [False, True])
def test_what_stays_on_the_general_kernel(by_env, monkeypatch):
    flags = 0
    if by_env:
        monkeypatch.setenv("CPECAN_WIDE_BANDS_HDP", "1")
    else:
        flags = 256
    for w in (249, 300, 376, 377, 504):
        assert plan(HDP, POST, AUTO, flags, w, edges=False) == GENERAL
        assert plan(HDP, POST, AUTO, flags | UNB, w) == GENERAL
        assert plan(HDP, POST, AUTO, flags | GENK, w) == GENERAL
        assert plan(HDP, EXP, AUTO, flags, w) == GENERAL  # the E-step ignores the flag
    # ... and the E-step within the wave builds' reach is theirs, as without the flag
    assert plan(HDP, EXP, AUTO, flags, 248) == sweep(1, 4, 248)
    assert plan(HDP, POST, AUTO, flags | GENK, 100) == GENERAL


def test_without_the_flag_and_with_the_other_flag():
    for flags in (0, WIDE):
        assert plan(HDP, POST, AUTO, flags, 249) == GENERAL
        assert plan(HDP, POST, AUTO, flags, 504) == GENERAL
        assert plan(HDP, POST, AUTO, flags, 248) == sweep(1, 4, 248)


@pytest.mark.parametrize("by_env", [False, True])
def test_the_flag_means_nothing_to_the_other_machines(by_env, monkeypatch):
    flags = 0
    if by_env:
        monkeypatch.setenv("CPECAN_WIDE_BANDS_HDP", "1")
    else:
        flags = 256
    for mode in (POST, EXP):
        assert plan(SM, mode, AUTO, flags, 300) == GENERAL
        assert plan(VAN, mode, AUTO, flags, 300) == GENERAL
    assert plan(DNA, POST, AUTO, flags, 300) == GENERAL
    assert plan(SM4, POST, AUTO, flags, 300) == GENERAL
    assert plan(ECH, POST, AUTO, flags, 300) == GENERAL
    # their own flag still serves them, with this one beside it
    assert plan(SM, POST, AUTO, flags | WIDE, 300) == sweep(0, 6, 376)
    assert plan(VAN, POST, AUTO, flags | WIDE, 300) == sweep(0, 6, 376)
    with pytest.raises(cp.CpecanError) as ei:
        plan(SM, POST, SYS, flags, 300)
    assert "band is 300 cells wide (systolic kernel: at most 248," in str(ei.value)


def test_environment_values(monkeypatch):
    monkeypatch.setenv("CPECAN_WIDE_BANDS_HDP", "0")
    assert plan(HDP, POST, AUTO, 0, 300) == GENERAL
    monkeypatch.setenv("CPECAN_WIDE_BANDS_HDP", "1")
    assert plan(HDP, POST, AUTO, 0, 300) == sweep(0, 6, 376)
    monkeypatch.delenv("CPECAN_WIDE_BANDS_HDP")
    monkeypatch.setenv("CPECAN_WIDE_BANDS", "1")  # the other machines' variable
    assert plan(HDP, POST, AUTO, 0, 300) == GENERAL

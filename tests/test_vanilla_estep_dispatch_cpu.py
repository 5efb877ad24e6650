"""The kernel choice of a vanilla E-step with CPECAN_FLAG_WIDE_BANDS_VANILLA_ESTEP / CPECAN_WIDE_BANDS_VANILLA_ESTEP=1
(choose_dispatch in cpecan_hip.hip) through cpecan_hip_plan_dispatch: no device.

Every expected value is a literal from include/cpecan_hip.h, not read from the tables under test: the vanilla wave
builds take bands up to 120 and 184 k-mers (2, 3 cells per lane); with the flag a vanilla batch of expectations whose
widest band is 185..248 k-mers runs on the four-wave E-step build of the workgroup family, one of 249..376 on the
six-wave build, one of 377..504 on the eight-wave build; past 504, on edges that step by more than one k-mer and with
CPECAN_FLAG_GENERAL_KERNEL it stays on the general kernel, and un-banded it is refused as without the flag.  The flag
means nothing to a vanilla posterior batch or to the other machines, and the three older wide-band flags nothing to a
vanilla E-step."""
import pytest

from cpecan_load import binding
from harness import BATCH_ENV

cp = binding()

SM, DNA, VAN, HDP, SM4, ECH = (cp.MACHINE_STRAWMAN, cp.MACHINE_DNA5, cp.MACHINE_VANILLA, cp.MACHINE_HDP,
                               cp.MACHINE_SM4, cp.MACHINE_ECHELON)
POST, EXP = cp.MODE_POSTERIOR, cp.MODE_EXPECTATIONS
AUTO, GEN, SYS = cp.KERNEL_AUTO, cp.KERNEL_GENERAL, cp.KERNEL_SYSTOLIC
UNB, GENK, WIDE, WIDE_HDP, WIDE_HDP_E = cp.FLAG_UNBANDED, cp.FLAG_GENERAL_KERNEL, 128, 256, 512
GENERAL = dict(kernel=GEN, wave=0, rows=0, build_max_width=0)
VARIABLE = "CPECAN_WIDE_BANDS_VANILLA_ESTEP"
OLDER_VARIABLES = ("CPECAN_WIDE_BANDS", "CPECAN_WIDE_BANDS_HDP", "CPECAN_WIDE_BANDS_HDP_ESTEP")


def sweep(wave, rows, width):
    return dict(kernel=SYS, wave=wave, rows=rows, build_max_width=width)


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in BATCH_ENV:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(params=[False, True], ids=["by-flag", "by-variable"])
def flag(request, monkeypatch):
    """the flag's value for the create call: 1024, or 0 with the variable set in its place"""
    if request.param:
        monkeypatch.setenv(VARIABLE, "1")
        return 0
    return 1024


def plan(machine, mode=POST, kernel=AUTO, flags=0, width=100, edges=True):
    return cp.plan_dispatch(machine, mode, kernel, flags, width, edges)


def test_the_flag_is_1024():
    assert cp.FLAG_WIDE_BANDS_VANILLA_ESTEP == 1024


@pytest.mark.parametrize("kernel", [AUTO, GEN, SYS])  # the vanilla create call has no kernel argument: any value
def test_vanilla_estep_builds(flag, kernel):
    assert plan(VAN, EXP, kernel, flag, 185) == sweep(0, 4, 248)
    assert plan(VAN, EXP, kernel, flag, 248) == sweep(0, 4, 248)
    assert plan(VAN, EXP, kernel, flag, 249) == sweep(0, 6, 376)
    assert plan(VAN, EXP, kernel, flag, 376) == sweep(0, 6, 376)
    assert plan(VAN, EXP, kernel, flag, 377) == sweep(0, 8, 504)
    assert plan(VAN, EXP, kernel, flag, 504) == sweep(0, 8, 504)
    # a band the wave builds hold is left to them
    assert plan(VAN, EXP, kernel, flag, 184) == sweep(1, 3, 184)
    assert plan(VAN, EXP, kernel, flag, 121) == sweep(1, 3, 184)
    assert plan(VAN, EXP, kernel, flag, 100) == sweep(1, 2, 120)
    assert plan(VAN, EXP, kernel, flag, 505) == GENERAL


def test_what_stays_on_the_general_kernel(flag):
    for w in (185, 248, 249, 300, 376, 377, 504):
        assert plan(VAN, EXP, AUTO, flag, w, edges=False) == GENERAL
        assert plan(VAN, EXP, AUTO, flag | GENK, w) == GENERAL
    assert plan(VAN, EXP, AUTO, flag | GENK, 100) == GENERAL


def test_unbanded_estep_is_refused_as_without_the_flag(flag):
    for flags in (UNB, flag | UNB):
        for w in (100, 200, 300):
            with pytest.raises(cp.CpecanError) as ei:
                plan(VAN, EXP, AUTO, flags, w)
            assert "expectations run over the banded matrix only" in str(ei.value)


def test_the_flag_means_nothing_to_a_posterior_batch(flag):
    for w in (200, 300, 400):
        assert plan(VAN, POST, AUTO, flag, w) == GENERAL
    assert plan(VAN, POST, AUTO, flag, 184) == sweep(1, 3, 184)
    # ... whose own flag still serves it, with this one beside it
    assert plan(VAN, POST, AUTO, flag | WIDE, 200) == sweep(0, 4, 248)
    assert plan(VAN, POST, AUTO, flag | WIDE, 300) == sweep(0, 6, 376)
    assert plan(VAN, POST, AUTO, flag | WIDE, 400) == sweep(0, 8, 504)


def test_the_older_flags_mean_nothing_to_an_estep(monkeypatch):
    older = (0, WIDE, WIDE_HDP, WIDE_HDP_E, WIDE | WIDE_HDP, WIDE | WIDE_HDP_E, WIDE | WIDE_HDP | WIDE_HDP_E)
    for flags in older:
        for w in (200, 300, 400):
            assert plan(VAN, EXP, AUTO, flags, w) == GENERAL
        assert plan(VAN, EXP, AUTO, flags, 184) == sweep(1, 3, 184)
        # ... and take nothing from the new one beside them
        assert plan(VAN, EXP, AUTO, flags | 1024, 200) == sweep(0, 4, 248)
        assert plan(VAN, EXP, AUTO, flags | 1024, 300) == sweep(0, 6, 376)
        assert plan(VAN, EXP, AUTO, flags | 1024, 400) == sweep(0, 8, 504)
    # nor do their variables
    for k in OLDER_VARIABLES:
        monkeypatch.setenv(k, "1")
    for w in (200, 300, 400):
        assert plan(VAN, EXP, AUTO, 0, w) == GENERAL
    assert plan(VAN, EXP, AUTO, 1024, 300) == sweep(0, 6, 376)


def test_the_flag_means_nothing_to_the_other_machines(flag):
    for mode in (POST, EXP):
        assert plan(SM, mode, AUTO, flag, 300) == GENERAL
        assert plan(HDP, mode, AUTO, flag, 300) == GENERAL
        assert plan(DNA, mode, AUTO, flag, 300) == GENERAL
        # their own flag still serves them, with this one beside it
        assert plan(SM, mode, AUTO, flag | WIDE, 300) == sweep(0, 6, 376)
    assert plan(HDP, POST, AUTO, flag | WIDE_HDP, 300) == sweep(0, 6, 376)
    assert plan(HDP, EXP, AUTO, flag | WIDE_HDP_E, 300) == sweep(0, 6, 376)
    assert plan(HDP, EXP, AUTO, flag | WIDE_HDP, 300) == GENERAL
    assert plan(SM4, POST, AUTO, flag, 300) == GENERAL
    assert plan(ECH, POST, AUTO, flag, 300) == GENERAL
    with pytest.raises(cp.CpecanError) as ei:
        plan(SM, EXP, SYS, flag, 300)
    assert "band is 300 cells wide (systolic kernel: at most 248," in str(ei.value)
    for machine in (SM4, ECH):
        with pytest.raises(cp.CpecanError) as ei:
            plan(machine, EXP, AUTO, flag, 300)
        assert "posterior decode only" in str(ei.value)


def test_environment_values(monkeypatch):
    monkeypatch.setenv(VARIABLE, "0")
    assert plan(VAN, EXP, AUTO, 0, 300) == GENERAL
    monkeypatch.setenv(VARIABLE, "1")
    assert plan(VAN, EXP, AUTO, 0, 200) == sweep(0, 4, 248)
    assert plan(VAN, EXP, AUTO, 0, 300) == sweep(0, 6, 376)
    assert plan(VAN, EXP, AUTO, 0, 400) == sweep(0, 8, 504)
    assert plan(VAN, POST, AUTO, 0, 300) == GENERAL
    assert plan(HDP, EXP, AUTO, 0, 300) == GENERAL
    monkeypatch.delenv(VARIABLE)
    monkeypatch.setenv("CPECAN_WIDE_BANDS", "1")  # the posterior decode's variable
    assert plan(VAN, EXP, AUTO, 0, 300) == GENERAL
    assert plan(VAN, POST, AUTO, 0, 300) == sweep(0, 6, 376)

"""The kernel choice of an HDP E-step with CPECAN_FLAG_WIDE_BANDS_HDP_ESTEP / CPECAN_WIDE_BANDS_HDP_ESTEP=1
(choose_dispatch in cpecan_hip.hip) through cpecan_hip_plan_dispatch: no device.

Every expected value is a literal from include/cpecan_hip.h, not read from the tables under test: the HDP wave builds
take bands up to 120, 184 and 248 k-mers (2, 3, 4 cells per lane); with the flag an HDP batch of expectations whose
widest band is 249..376 k-mers runs on the six-wave E-step build of the workgroup family, one of 377..504 on the
eight-wave build; past 504, on edges that step by more than one k-mer and with CPECAN_FLAG_GENERAL_KERNEL it stays on
the general kernel, and un-banded it is refused as without the flag.  The flag means nothing to an HDP posterior batch
or to the other machines, and the two older wide-band flags nothing to an HDP E-step."""
import pytest

from cpecan_load import binding
from harness import BATCH_ENV

cp = binding()

SM, DNA, VAN, HDP, SM4, ECH = (cp.MACHINE_STRAWMAN, cp.MACHINE_DNA5, cp.MACHINE_VANILLA, cp.MACHINE_HDP,
                               cp.MACHINE_SM4, cp.MACHINE_ECHELON)
POST, EXP = cp.MODE_POSTERIOR, cp.MODE_EXPECTATIONS
AUTO, GEN, SYS = cp.KERNEL_AUTO, cp.KERNEL_GENERAL, cp.KERNEL_SYSTOLIC
UNB, GENK, WIDE, WIDE_HDP = cp.FLAG_UNBANDED, cp.FLAG_GENERAL_KERNEL, 128, 256
GENERAL = dict(kernel=GEN, wave=0, rows=0, build_max_width=0)
VARIABLE = "CPECAN_WIDE_BANDS_HDP_ESTEP"


def sweep(wave, rows, width):
    return dict(kernel=SYS, wave=wave, rows=rows, build_max_width=width)


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in BATCH_ENV:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(params=[False, True], ids=["by-flag", "by-variable"])
def flag(request, monkeypatch):
    """the flag's value for the create call: 512, or 0 with the variable set in its place"""
    if request.param:
        monkeypatch.setenv(VARIABLE, "1")
        return 0
    return 512


def plan(machine, mode=POST, kernel=AUTO, flags=0, width=100, edges=True):
    return cp.plan_dispatch(machine, mode, kernel, flags, width, edges)


def test_the_flag_is_512():
    assert cp.FLAG_WIDE_BANDS_HDP_ESTEP == 512


@pytest.mark.parametrize("kernel", [AUTO, GEN, SYS])  # the HDP create call has no kernel argument: whatever is passed
def test_hdp_estep_builds(flag, kernel):
    assert plan(HDP, EXP, kernel, flag, 249) == sweep(0, 6, 376)
    assert plan(HDP, EXP, kernel, flag, 376) == sweep(0, 6, 376)
    assert plan(HDP, EXP, kernel, flag, 377) == sweep(0, 8, 504)
    assert plan(HDP, EXP, kernel, flag, 504) == sweep(0, 8, 504)
    # a band the wave builds hold is left to them
    assert plan(HDP, EXP, kernel, flag, 248) == sweep(1, 4, 248)
    assert plan(HDP, EXP, kernel, flag, 184) == sweep(1, 3, 184)
    assert plan(HDP, EXP, kernel, flag, 100) == sweep(1, 2, 120)
    assert plan(HDP, EXP, kernel, flag, 505) == GENERAL


def test_what_stays_on_the_general_kernel(flag):
    for w in (249, 300, 376, 377, 504):
        assert plan(HDP, EXP, AUTO, flag, w, edges=False) == GENERAL
        assert plan(HDP, EXP, AUTO, flag | GENK, w) == GENERAL
    assert plan(HDP, EXP, AUTO, flag | GENK, 100) == GENERAL


def test_unbanded_estep_is_refused_as_without_the_flag(flag):
    for flags in (UNB, flag | UNB):
        for w in (100, 300):
            with pytest.raises(cp.CpecanError) as ei:
                plan(HDP, EXP, AUTO, flags, w)
            assert "expectations run over the banded matrix only" in str(ei.value)


def test_the_flag_means_nothing_to_a_posterior_batch(flag):
    assert plan(HDP, POST, AUTO, flag, 300) == GENERAL
    assert plan(HDP, POST, AUTO, flag, 248) == sweep(1, 4, 248)
    # ... whose own flag still serves it, with this one beside it
    assert plan(HDP, POST, AUTO, flag | WIDE_HDP, 300) == sweep(0, 6, 376)
    assert plan(HDP, POST, AUTO, flag | WIDE_HDP, 400) == sweep(0, 8, 504)


def test_the_older_flags_mean_nothing_to_an_estep(flag, monkeypatch):
    for flags in (0, WIDE, WIDE_HDP, WIDE | WIDE_HDP):
        assert plan(HDP, EXP, AUTO, flags, 300) == (GENERAL if flag == 512 else sweep(0, 6, 376))
    # (with the variable every E-step has the flag; without it, by the flag alone:)
    monkeypatch.delenv(VARIABLE, raising=False)
    assert plan(HDP, EXP, AUTO, WIDE_HDP, 300) == GENERAL
    assert plan(HDP, EXP, AUTO, WIDE, 300) == GENERAL
    assert plan(HDP, EXP, AUTO, WIDE_HDP | 512, 300) == sweep(0, 6, 376)
    assert plan(HDP, EXP, AUTO, WIDE_HDP | 512, 400) == sweep(0, 8, 504)


def test_the_flag_means_nothing_to_the_other_machines(flag):
    for mode in (POST, EXP):
        assert plan(SM, mode, AUTO, flag, 300) == GENERAL
        assert plan(VAN, mode, AUTO, flag, 300) == GENERAL
        assert plan(DNA, mode, AUTO, flag, 300) == GENERAL
        # their own flag still serves them, with this one beside it
        assert plan(SM, mode, AUTO, flag | WIDE, 300) == sweep(0, 6, 376)
    assert plan(SM4, POST, AUTO, flag, 300) == GENERAL
    assert plan(ECH, POST, AUTO, flag, 300) == GENERAL
    assert plan(VAN, POST, AUTO, flag | WIDE, 300) == sweep(0, 6, 376)
    assert plan(VAN, EXP, AUTO, flag | WIDE, 300) == GENERAL
    with pytest.raises(cp.CpecanError) as ei:
        plan(SM, EXP, SYS, flag, 300)
    assert "band is 300 cells wide (systolic kernel: at most 248," in str(ei.value)
    for machine in (SM4, ECH):
        with pytest.raises(cp.CpecanError) as ei:
            plan(machine, EXP, AUTO, flag, 300)
        assert "posterior decode only" in str(ei.value)


def test_environment_values(monkeypatch):
    monkeypatch.setenv(VARIABLE, "0")
    assert plan(HDP, EXP, AUTO, 0, 300) == GENERAL
    monkeypatch.setenv(VARIABLE, "1")
    assert plan(HDP, EXP, AUTO, 0, 300) == sweep(0, 6, 376)
    assert plan(HDP, POST, AUTO, 0, 300) == GENERAL
    monkeypatch.delenv(VARIABLE)
    monkeypatch.setenv("CPECAN_WIDE_BANDS", "1")      # the other machines' variable
    monkeypatch.setenv("CPECAN_WIDE_BANDS_HDP", "1")  # the posterior decode's
    assert plan(HDP, EXP, AUTO, 0, 300) == GENERAL
    assert plan(HDP, POST, AUTO, 0, 300) == sweep(0, 6, 376)

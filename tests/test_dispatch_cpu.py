"""The kernel choice of batch creation (choose_dispatch in cpecan_hip.hip) through cpecan_hip_plan_dispatch: no device.

Every expected value below is a literal from include/cpecan_hip.h and the commit messages that introduced the builds, not
read from the tables under test:
  - workgroup family (CPECAN_FLAG_WORKGROUP_KERNELS, CPECAN_KERNELS=systolic): 1, 2, 3, 4 waves for bands up to 56, 120,
    184, 248 k-mers; wave family (the default): 2, 3, 4 cells per lane up to 120, 184, 248 (the HDP machine too; the
    vanilla machine's ends at 3 cells, 184);
  - CPECAN_FLAG_WIDE_BANDS / CPECAN_WIDE_BANDS=1: 6 and 8 waves up to 376 and 504 for the strawMan machine (both modes),
    4, 6, 8 waves for 185..248, ..376, ..504 for the vanilla machine's posterior decode only;
  - AUTO falls to the general kernel past the widest reachable build or on edges that step by more than one;
    CPECAN_KERNEL_SYSTOLIC refuses there and names the limit; cell dumps and un-banded batches only on the general kernel;
  - the 5-state machine's wave kernels take bands up to 192 cells.
"""
import pytest

from cpecan_load import binding
from harness import BATCH_ENV

cp = binding()

SM, DNA, VAN, HDP, SM4, ECH = (cp.MACHINE_STRAWMAN, cp.MACHINE_DNA5, cp.MACHINE_VANILLA, cp.MACHINE_HDP,
                               cp.MACHINE_SM4, cp.MACHINE_ECHELON)
POST, EXP = cp.MODE_POSTERIOR, cp.MODE_EXPECTATIONS
AUTO, GEN, SYS = cp.KERNEL_AUTO, cp.KERNEL_GENERAL, cp.KERNEL_SYSTOLIC
WG, WIDE, DUMP, UNB, GENK = (cp.FLAG_WORKGROUP_KERNELS, cp.FLAG_WIDE_BANDS, cp.FLAG_DEBUG_DUMP, cp.FLAG_UNBANDED,
                             cp.FLAG_GENERAL_KERNEL)
GENERAL = dict(kernel=GEN, wave=0, rows=0, build_max_width=0)


def sweep(wave, rows, width):
    return dict(kernel=SYS, wave=wave, rows=rows, build_max_width=width)


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in BATCH_ENV:
        monkeypatch.delenv(k, raising=False)


def plan(machine, mode=POST, kernel=AUTO, flags=0, width=100, edges=True):
    return cp.plan_dispatch(machine, mode, kernel, flags, width, edges)


def refused(text, *a, **k):
    with pytest.raises(cp.CpecanError) as ei:
        plan(*a, **k)
    assert ei.value.code == cp.EINVAL
    assert text in str(ei.value), str(ei.value)


# (first width, last width, rows, widest band of the build): both sides of every class boundary
WORKGROUP = [(1, 56, 1, 56), (57, 120, 2, 120), (121, 184, 3, 184), (185, 248, 4, 248)]
WAVE = [(1, 120, 2, 120), (121, 184, 3, 184), (185, 248, 4, 248)]
WAVE_VANILLA = [(1, 120, 2, 120), (121, 184, 3, 184)]
WIDE_STRAWMAN = [(249, 376, 6, 376), (377, 504, 8, 504)]
WIDE_VANILLA = [(185, 248, 4, 248), (249, 376, 6, 376), (377, 504, 8, 504)]


@pytest.mark.parametrize("mode", [POST, EXP])
@pytest.mark.parametrize("kernel", [AUTO, SYS])
def test_strawman_families_by_band_width(mode, kernel, monkeypatch):
    for lo, hi, rows, width in WAVE:
        for w in (lo, hi):
            assert plan(SM, mode, kernel, 0, w) == sweep(1, rows, width)
    for lo, hi, rows, width in WORKGROUP:
        for w in (lo, hi):
            assert plan(SM, mode, kernel, WG, w) == sweep(0, rows, width)
    monkeypatch.setenv("CPECAN_KERNELS", "systolic")
    for lo, hi, rows, width in WORKGROUP:
        for w in (lo, hi):
            assert plan(SM, mode, kernel, 0, w) == sweep(0, rows, width)


@pytest.mark.parametrize("mode", [POST, EXP])
@pytest.mark.parametrize("flags", [0, WG])
def test_strawman_past_the_widest_build(mode, flags):
    assert plan(SM, mode, AUTO, flags, 249) == GENERAL
    assert plan(SM, mode, GEN, flags, 249) == GENERAL
    refused("band is 249 cells wide (systolic kernel: at most 248,", SM, mode, SYS, flags, 249)
    # ragged edges: whatever the width
    assert plan(SM, mode, AUTO, flags, 100, edges=False) == GENERAL
    refused("band is 100 cells wide (systolic kernel: at most 248,", SM, mode, SYS, flags, 100, edges=False)


def test_general_kernel_on_request():
    for machine in (SM, DNA, VAN, HDP, SM4, ECH):
        flags = GENK if machine in (VAN, HDP, DNA) else 0
        assert plan(machine, POST, GEN, flags, 50) == GENERAL


@pytest.mark.parametrize("mode", [POST, EXP])
@pytest.mark.parametrize("kernel", [AUTO, SYS])
@pytest.mark.parametrize("family_flag", [0, WG])
@pytest.mark.parametrize("by_env", [False, True])
def test_strawman_wide_builds(mode, kernel, family_flag, by_env, monkeypatch):
    flags = family_flag
    if by_env:
        monkeypatch.setenv("CPECAN_WIDE_BANDS", "1")
    else:
        flags |= WIDE
    for lo, hi, rows, width in WIDE_STRAWMAN:
        for w in (lo, hi):
            assert plan(SM, mode, kernel, flags, w) == sweep(0, rows, width)
    # a band the family holds is left to it
    assert plan(SM, mode, kernel, flags, 248) == sweep(0 if family_flag else 1, 4, 248)
    assert plan(SM, mode, kernel, flags, 120) == sweep(0 if family_flag else 1, 2, 120)
    if kernel == AUTO:
        assert plan(SM, mode, kernel, flags, 505) == GENERAL
        assert plan(SM, mode, kernel, flags, 300, edges=False) == GENERAL
    else:
        refused("band is 505 cells wide (systolic kernel: at most 504,", SM, mode, kernel, flags, 505)
        refused("(systolic kernel: at most 504,", SM, mode, kernel, flags, 300, edges=False)


def test_wide_bands_environment_values(monkeypatch):
    monkeypatch.setenv("CPECAN_WIDE_BANDS", "0")
    assert plan(SM, POST, AUTO, 0, 300) == GENERAL
    monkeypatch.setenv("CPECAN_WIDE_BANDS", "1")
    assert plan(SM, POST, AUTO, 0, 300) == sweep(0, 6, 376)
    # the flag means nothing to the other machines
    assert plan(HDP, POST, AUTO, 0, 300) == GENERAL
    assert plan(DNA, POST, AUTO, 0, 300) == GENERAL
    assert plan(SM4, POST, AUTO, 0, 300) == GENERAL
    assert plan(ECH, POST, AUTO, 0, 300) == GENERAL


@pytest.mark.parametrize("mode", [POST, EXP])
def test_systolic_rows_environment(mode, monkeypatch):
    monkeypatch.setenv("CPECAN_SYSTOLIC_ROWS", "3")
    assert plan(SM, mode, AUTO, WG, 50) == sweep(0, 3, 184)
    assert plan(SM, mode, AUTO, 0, 50) == sweep(1, 3, 184)
    assert plan(SM, mode, AUTO, WG, 200) == sweep(0, 4, 248)  # at least N
    assert plan(SM, mode, AUTO, WG | WIDE, 300) == sweep(0, 6, 376)  # the wide builds are not part of the walk
    monkeypatch.setenv("CPECAN_SYSTOLIC_ROWS", "4")
    assert plan(SM, mode, AUTO, WG, 50) == sweep(0, 4, 248)
    assert plan(HDP, mode, AUTO, 0, 50) == sweep(1, 4, 248)
    assert plan(VAN, mode, AUTO, 0, 50) == sweep(1, 3, 184)  # (the vanilla wave family ends at three cells per lane)
    monkeypatch.setenv("CPECAN_SYSTOLIC_ROWS", "9")  # clamped
    assert plan(SM, mode, AUTO, WG, 50) == sweep(0, 4, 248)
    monkeypatch.setenv("CPECAN_SYSTOLIC_ROWS", "0")
    assert plan(SM, mode, AUTO, WG, 50) == sweep(0, 1, 56)


@pytest.mark.parametrize("mode", [POST, EXP])
@pytest.mark.parametrize("kernel", [AUTO, GEN, SYS])  # these machines have no kernel argument: whatever is passed
def test_hdp_and_vanilla_wave_builds(mode, kernel, monkeypatch):
    for env in (None, "systolic"):  # CPECAN_KERNELS and CPECAN_FLAG_WORKGROUP_KERNELS are the strawMan machine's
        if env:
            monkeypatch.setenv("CPECAN_KERNELS", env)
        for flags in (0, WG):
            for lo, hi, rows, width in WAVE:
                for w in (lo, hi):
                    assert plan(HDP, mode, kernel, flags, w) == sweep(1, rows, width)
            for lo, hi, rows, width in WAVE_VANILLA:
                for w in (lo, hi):
                    assert plan(VAN, mode, kernel, flags, w) == sweep(1, rows, width)
            assert plan(HDP, mode, kernel, flags, 249) == GENERAL
            assert plan(HDP, mode, kernel, flags | WIDE, 249) == GENERAL
            assert plan(VAN, mode, kernel, flags, 185) == GENERAL
            assert plan(HDP, mode, kernel, flags, 100, edges=False) == GENERAL
            assert plan(VAN, mode, kernel, flags, 100, edges=False) == GENERAL
            assert plan(HDP, mode, kernel, flags | GENK, 100) == GENERAL
            assert plan(VAN, mode, kernel, flags | GENK, 100) == GENERAL


@pytest.mark.parametrize("by_env", [False, True])
def test_vanilla_wide_builds_posterior_only(by_env, monkeypatch):
    flags = 0
    if by_env:
        monkeypatch.setenv("CPECAN_WIDE_BANDS", "1")
    else:
        flags = WIDE
    for lo, hi, rows, width in WIDE_VANILLA:
        for w in (lo, hi):
            assert plan(VAN, POST, AUTO, flags, w) == sweep(0, rows, width)
            assert plan(VAN, EXP, AUTO, flags, w) == GENERAL  # a vanilla E-step ignores the flag
            assert plan(VAN, POST, AUTO, flags | GENK, w) == GENERAL
            assert plan(VAN, POST, AUTO, flags | UNB, w) == GENERAL
            assert plan(VAN, POST, AUTO, flags, w, edges=False) == GENERAL
    assert plan(VAN, POST, AUTO, flags, 184) == sweep(1, 3, 184)
    assert plan(VAN, EXP, AUTO, flags, 184) == sweep(1, 3, 184)
    assert plan(VAN, POST, AUTO, flags, 505) == GENERAL


def test_cell_dumps_and_unbanded_only_on_the_general_kernel():
    assert plan(SM, POST, AUTO, DUMP, 100) == GENERAL
    assert plan(SM, POST, GEN, DUMP, 100) == GENERAL
    assert plan(SM, EXP, AUTO, DUMP, 100) == GENERAL
    refused("cell dumps are only available from the general kernel", SM, POST, SYS, DUMP, 100)
    refused("cell dumps are only available from the general kernel", SM, POST, SYS, DUMP | WIDE, 300)
    assert plan(SM, POST, AUTO, UNB, 100) == GENERAL
    assert plan(SM, POST, GEN, UNB, 100) == GENERAL
    refused("un-banded alignment: posterior mode on the general kernel only", SM, POST, SYS, UNB, 100)
    for kernel in (AUTO, GEN, SYS):
        refused("un-banded alignment: posterior mode on the general kernel only", SM, EXP, kernel, UNB, 100)
    for machine in (DNA, VAN, HDP, SM4, ECH):
        assert plan(machine, POST, AUTO, UNB, 100) == GENERAL
    for machine in (DNA, VAN, HDP):
        refused("expectations run over the banded matrix only", machine, EXP, AUTO, UNB, 100)
    for machine, who in ((DNA, "DNA batches: no cell dumps"), (VAN, "vanilla batches: no cell dumps"),
                         (HDP, "HDP batches: no cell dumps"),
                         (SM4, "4-state batches: posterior decode only, no cell dumps"),
                         (ECH, "echelon batches: posterior decode only, no cell dumps")):
        refused(who, machine, POST, AUTO, DUMP, 100)


def test_machines_without_an_estep():
    refused("4-state batches: posterior decode only, no cell dumps", SM4, EXP, AUTO, 0, 100)
    refused("echelon batches: posterior decode only, no cell dumps", ECH, EXP, AUTO, 0, 100)
    for w in (10, 100, 600):
        for edges in (True, False):
            assert plan(SM4, POST, AUTO, 0, w, edges) == GENERAL
            assert plan(ECH, POST, AUTO, 0, w, edges) == GENERAL


@pytest.mark.parametrize("mode", [POST, EXP])
def test_five_state_wave_path(mode):
    on = dict(GENERAL, wave=1)  # batch_info reports the general kernel, batch_kernel_family the wave path
    for w in (1, 64, 65, 128, 129, 192):
        assert plan(DNA, mode, AUTO, 0, w) == on
        assert plan(DNA, mode, AUTO, 0, w, edges=False) == on  # (the 5-state kernels read the band as intervals)
        assert plan(DNA, mode, AUTO, GENK, w) == GENERAL
    assert plan(DNA, mode, AUTO, 0, 193) == GENERAL
    assert plan(DNA, POST, AUTO, UNB, 100) == GENERAL


def test_bad_arguments():
    refused("unknown machine 6", 6)
    refused("unknown machine -1", -1)
    refused("unknown mode 2", SM, 2)

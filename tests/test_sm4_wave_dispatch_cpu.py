"""CPECAN_FLAG_SM4_WAVE (524288) through cpecan_hip_plan_dispatch (the answers of choose_dispatch in cpecan_hip.hip):
no device.

A banded 4-state posterior batch that carries the flag and whose widest band is at most 128 cells runs on the
one-wave-per-alignment kernels of cpecan_kernel_wave4.hip, reported as a DNA batch on the 5-state wave kernels is:
kernel GENERAL, wave 1, rows 0.  Past 128 cells, un-banded or with CPECAN_FLAG_GENERAL_KERNEL it is the general kernel
as without the flag; expectations and cell dumps are refused with the texts they always had; the flag means nothing to
another machine; the C-ABI reads no variable for it (libcpecan_host.so has CPECAN_SM4_WAVE for its own batches)."""
import os
import re

import pytest

from cpecan_load import ROOT, binding
from harness import BATCH_ENV

cp = binding()

WAVE4 = 524288
SM, DNA, VAN, HDP, SM4, ECH = (cp.MACHINE_STRAWMAN, cp.MACHINE_DNA5, cp.MACHINE_VANILLA, cp.MACHINE_HDP,
                               cp.MACHINE_SM4, cp.MACHINE_ECHELON)
POST, EXP = cp.MODE_POSTERIOR, cp.MODE_EXPECTATIONS
AUTO, GEN, SYS = cp.KERNEL_AUTO, cp.KERNEL_GENERAL, cp.KERNEL_SYSTOLIC
GENERAL = dict(kernel=GEN, wave=0, rows=0, build_max_width=0)
WAVE = dict(GENERAL, wave=1)
REFUSAL = "4-state batches: posterior decode only, no cell dumps"


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in BATCH_ENV + ("CPECAN_SM4_WAVE",):
        monkeypatch.delenv(k, raising=False)


def answer(*q):
    """the four outputs of cpecan_hip_plan_dispatch, or the code and the text of the refusal"""
    try:
        return cp.plan_dispatch(*q)
    except cp.CpecanError as e:
        return (e.code, str(e))


def test_the_header_and_the_binding_name_the_flag():
    header = open(os.path.join(ROOT, "include", "cpecan_hip.h")).read()
    assert re.search(r"#define CPECAN_FLAG_SM4_WAVE %d\b" % WAVE4, header)
    assert cp.FLAG_SM4_WAVE == WAVE4
    for name, value in re.findall(r"#define (CPECAN_FLAG_\w+) (\d+)\b", header):
        assert name == "CPECAN_FLAG_SM4_WAVE" or not int(value) & WAVE4, name   # the next free bit, nobody else's
    assert max(int(v) for _, v in re.findall(r"#define (CPECAN_FLAG_\w+) (\d+)\b", header)) == WAVE4


@pytest.mark.parametrize("edges", [True, False])
@pytest.mark.parametrize("kernel", [AUTO, GEN])
def test_kernel_choice_under_the_flag(kernel, edges):
    for w in (1, 64, 65, 128):
        assert answer(SM4, POST, kernel, WAVE4, w, edges) == WAVE, w
        assert answer(SM4, POST, kernel, 0, w, edges) == GENERAL, w
    for w in (129, 300):
        assert answer(SM4, POST, kernel, WAVE4, w, edges) == GENERAL, w


def test_flag_combinations():
    for w in (1, 64, 65, 128, 129, 300):
        for edges in (True, False):
            assert answer(SM4, POST, AUTO, WAVE4 | cp.FLAG_UNBANDED, w, edges) == GENERAL, w
            assert answer(SM4, POST, AUTO, WAVE4 | cp.FLAG_GENERAL_KERNEL, w, edges) == GENERAL, w
            for flags in (WAVE4 | cp.FLAG_DEBUG_DUMP, WAVE4 | cp.FLAG_DEBUG_DUMP | cp.FLAG_UNBANDED):
                code, text = answer(SM4, POST, AUTO, flags, w, edges)
                assert REFUSAL in text and (code, text) == answer(SM4, POST, AUTO, flags & ~WAVE4, w, edges)
            code, text = answer(SM4, EXP, AUTO, WAVE4, w, edges)
            assert REFUSAL in text and (code, text) == answer(SM4, EXP, AUTO, 0, w, edges)
    # flags that mean nothing to this machine keep meaning nothing beside the flag
    for other in (cp.FLAG_SCAN_DECODE, cp.FLAG_WORKGROUP_KERNELS, cp.FLAG_SMALL_FOOTPRINT, cp.FLAG_WIDE_BANDS,
                  cp.FLAG_ASM_NARROW_BANDS):
        assert answer(SM4, POST, AUTO, WAVE4 | other, 100, True) == WAVE
        assert answer(SM4, POST, AUTO, WAVE4 | other, 129, True) == GENERAL


@pytest.mark.parametrize("mode", [POST, EXP])
@pytest.mark.parametrize("machine", [SM, DNA, VAN, HDP, ECH])
def test_other_machines_ignore_the_flag(machine, mode, monkeypatch):
    flag_sets = (0, cp.FLAG_WORKGROUP_KERNELS, cp.FLAG_WIDE_BANDS, cp.FLAG_GENERAL_KERNEL, cp.FLAG_UNBANDED,
                 cp.FLAG_WIDE_BANDS_HDP | cp.FLAG_WIDE_BANDS_HDP_ESTEP, cp.FLAG_WIDE_BANDS_VANILLA_ESTEP)
    for by_env in (False, True):
        if by_env:
            monkeypatch.setenv("CPECAN_KERNELS", "systolic")
        for kernel in (AUTO, GEN, SYS):
            for flags in flag_sets:
                for w in (50, 100, 200, 300):
                    for edges in (True, False):
                        q = (machine, mode, kernel, flags, w, edges)
                        assert answer(machine, mode, kernel, flags | WAVE4, w, edges) == answer(*q), q
                        for fn in (cp.plan_expectation_pass, cp.plan_assembly_sweeps):
                            assert fn(machine, mode, kernel, flags | WAVE4, w, edges) == fn(*q), q


def test_no_variable_of_batch_creation_sets_it(monkeypatch):
    monkeypatch.setenv("CPECAN_SM4_WAVE", "1")
    for w in (1, 64, 65, 128, 129, 300):
        assert answer(SM4, POST, AUTO, 0, w, True) == GENERAL, w
        assert answer(SM4, POST, AUTO, WAVE4, w, True) == (WAVE if w <= 128 else GENERAL), w
    monkeypatch.setenv("CPECAN_SM4_WAVE", "0")
    assert answer(SM4, POST, AUTO, WAVE4, 100, True) == WAVE
    for name in ("cpecan_hip.hip", "cpecan_run.hip", "cpecan_readback.hip"):
        assert "CPECAN_SM4_WAVE" not in open(os.path.join(ROOT, "cpecan-signal_amd", "csrc", name)).read(), name
    host = open(os.path.join(ROOT, "cpecan-signal_amd", "csrc", "host", "cpecan_api.c")).read()
    assert 'getenv("CPECAN_SM4_WAVE")' in host

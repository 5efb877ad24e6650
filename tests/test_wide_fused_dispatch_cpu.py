"""CPECAN_FLAG_WIDE_BANDS_FUSED_ESTEP (4096) does not take part in the kernel choice: for every machine, both modes, the
three kernel requests and a band in the range of every build, cpecan_hip_plan_dispatch answers with the bit set what it
answers without it -- the same kernel, family, rows and widest band, or the same refusal with the same text -- and so it
does with CPECAN_EXPECT_FUSED_WIDE=1 in the environment.  (What the bit does change, the form of the E-step of a strawMan
batch on the six- and eight-wave builds, is batch creation's: tests/test_wide_fused_expectations_gpu.py.)  No device."""
import pytest

from cpecan_load import binding
from harness import BATCH_ENV
from test_workgroup_fused_dispatch_cpu import FLAGS, MACHINES, WIDTHS, answer

cp = binding()

WIDE_FUSED = 4096
MODES = (cp.MODE_POSTERIOR, cp.MODE_EXPECTATIONS)
KERNELS = (cp.KERNEL_AUTO, cp.KERNEL_GENERAL, cp.KERNEL_SYSTOLIC)


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in BATCH_ENV:
        monkeypatch.delenv(k, raising=False)


def queries(machine, mode):
    return [(machine, mode, kernel, flags, width, edges) for kernel in KERNELS for flags in FLAGS for width in WIDTHS
            for edges in (True, False)]


def test_the_binding_names_the_flag():
    assert cp.FLAG_WIDE_BANDS_FUSED_ESTEP == WIDE_FUSED
    # a number of its own: no other flag of the binding has the bit
    others = [v for k, v in vars(cp).items() if k.startswith("FLAG_") and k != "FLAG_WIDE_BANDS_FUSED_ESTEP"]
    assert len(others) >= 12 and not any(v & WIDE_FUSED for v in others)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("machine", MACHINES)
def test_the_flag_does_not_move_the_kernel_choice(machine, mode, monkeypatch):
    seen = set()
    for by_env in (False, True):
        if by_env:
            monkeypatch.setenv("CPECAN_KERNELS", "systolic")
        for q in queries(machine, mode):
            without = answer(*q)
            assert answer(*q[:3], q[3] | WIDE_FUSED, *q[4:]) == without, q
            assert answer(*q[:3], q[3] | WIDE_FUSED | cp.FLAG_WORKGROUP_FUSED_ESTEP, *q[4:]) == without, q
            if isinstance(without, dict):
                seen.add((without["kernel"], without["wave"], without["rows"]))
    if machine == cp.MACHINE_STRAWMAN:  # the comparison went through every build of the workgroup family
        assert {(cp.KERNEL_SYSTOLIC, 0, r) for r in (1, 2, 3, 4, 6, 8)} <= seen, seen


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("machine", MACHINES)
def test_the_variable_does_not_move_it_either(machine, mode, monkeypatch):
    for by_env in (False, True):
        if by_env:
            monkeypatch.setenv("CPECAN_KERNELS", "systolic")
        monkeypatch.delenv("CPECAN_EXPECT_FUSED_WIDE", raising=False)
        ref = [answer(*q) for q in queries(machine, mode)]
        for value in ("1", "0"):
            monkeypatch.setenv("CPECAN_EXPECT_FUSED_WIDE", value)
            assert [answer(*q) for q in queries(machine, mode)] == ref, value
            assert [answer(*q[:3], q[3] | WIDE_FUSED, *q[4:]) for q in queries(machine, mode)] == ref, value


def test_the_variable_beside_the_wide_bands_variable(monkeypatch):
    """CPECAN_WIDE_BANDS=1 is what sends a flagless strawMan batch to the six- and eight-wave builds; the fused variable
    beside it leaves that choice alone"""
    monkeypatch.setenv("CPECAN_WIDE_BANDS", "1")
    ref = [answer(*q) for q in queries(cp.MACHINE_STRAWMAN, cp.MODE_EXPECTATIONS)]
    assert any(isinstance(a, dict) and a["rows"] in (6, 8) for a in ref)
    monkeypatch.setenv("CPECAN_EXPECT_FUSED_WIDE", "1")
    assert [answer(*q) for q in queries(cp.MACHINE_STRAWMAN, cp.MODE_EXPECTATIONS)] == ref

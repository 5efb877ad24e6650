"""CPECAN_FLAG_WORKGROUP_FUSED_ESTEP (2048) does not take part in the kernel choice: for every machine, both modes and a
band in the range of every build, cpecan_hip_plan_dispatch answers with the bit set what it answers without it -- the same
kernel, family, rows and widest band, or the same refusal with the same text.  (What the bit does change, the form of the
E-step of a strawMan batch on the workgroup kernels, is batch creation's: tests/test_workgroup_fused_expectations_gpu.py.)
No device."""
import pytest

from cpecan_load import binding
from harness import BATCH_ENV

cp = binding()

FUSED = 2048
MACHINES = (cp.MACHINE_STRAWMAN, cp.MACHINE_DNA5, cp.MACHINE_VANILLA, cp.MACHINE_HDP, cp.MACHINE_SM4, cp.MACHINE_ECHELON)
# a band inside every build's range and on both sides of every boundary: the four workgroup builds (56, 120, 184, 248),
# the wide ones (376, 504), past them
WIDTHS = (1, 30, 56, 57, 100, 120, 121, 184, 185, 200, 248, 249, 300, 376, 377, 504, 505)
FLAGS = (0, cp.FLAG_WORKGROUP_KERNELS, cp.FLAG_WIDE_BANDS, cp.FLAG_WORKGROUP_KERNELS | cp.FLAG_WIDE_BANDS,
         cp.FLAG_GENERAL_KERNEL, cp.FLAG_WIDE_BANDS_HDP | cp.FLAG_WIDE_BANDS_HDP_ESTEP | cp.FLAG_WIDE_BANDS_VANILLA_ESTEP,
         cp.FLAG_UNBANDED)


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in BATCH_ENV:
        monkeypatch.delenv(k, raising=False)


def answer(*a):
    """the four outputs, or the code and the text of the refusal"""
    try:
        return cp.plan_dispatch(*a)
    except cp.CpecanError as e:
        return (e.code, str(e))


def test_the_binding_names_the_flag():
    assert cp.FLAG_WORKGROUP_FUSED_ESTEP == FUSED


@pytest.mark.parametrize("mode", [cp.MODE_POSTERIOR, cp.MODE_EXPECTATIONS])
@pytest.mark.parametrize("machine", MACHINES)
def test_the_flag_does_not_move_the_kernel_choice(machine, mode, monkeypatch):
    seen = set()
    for by_env in (False, True):
        if by_env:
            monkeypatch.setenv("CPECAN_KERNELS", "systolic")
        for kernel in (cp.KERNEL_AUTO, cp.KERNEL_GENERAL, cp.KERNEL_SYSTOLIC):
            for flags in FLAGS:
                for width in WIDTHS:
                    for edges in (True, False):
                        without = answer(machine, mode, kernel, flags, width, edges)
                        assert answer(machine, mode, kernel, flags | FUSED, width, edges) == without, \
                            (kernel, flags, width, edges)
                        if isinstance(without, dict):
                            seen.add((without["kernel"], without["wave"], without["rows"]))
    if machine == cp.MACHINE_STRAWMAN:  # the comparison went through every build of the workgroup family
        assert {(cp.KERNEL_SYSTOLIC, 0, r) for r in (1, 2, 3, 4, 6, 8)} <= seen, seen


def test_the_variable_does_not_move_it_either(monkeypatch):
    ref = [answer(cp.MACHINE_STRAWMAN, cp.MODE_EXPECTATIONS, cp.KERNEL_AUTO, f, w, True) for f in FLAGS for w in WIDTHS]
    monkeypatch.setenv("CPECAN_EXPECT_FUSED_WORKGROUP", "1")
    assert [answer(cp.MACHINE_STRAWMAN, cp.MODE_EXPECTATIONS, cp.KERNEL_AUTO, f, w, True)
            for f in FLAGS for w in WIDTHS] == ref

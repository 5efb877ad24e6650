"""The six- and eight-wave fused builds (f6, f8: the strawMan E-step summed inside the sweep back at bands of 249..504
k-mers) are on the Makefile's list with the defines they are meant to be compiled with, so that
tests/test_sweep_build_resources.py holds them to the "f" row of its table (forward and backward only, at most 256 VGPRs,
nothing spilled or in scratch, the LDS rule) with no edit there; what the sweep back of each is designed around beyond that
row -- three waves per SIMD at six waves per workgroup, whatever the allocation lands on at eight -- is asserted here from
the compiler's metadata.
CPU-only: hipcc cross-compiles gfx950."""
import os

import pytest

from sweep_builds import HIPCC, builds, device_asm, kernel_meta

needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
WIDE_FUSED = {"f6": ("-DSY_R=6", "-DSY_FUSED"), "f8": ("-DSY_R=8", "-DSY_FUSED")}


def by_name():
    return dict((b.name, b) for b in builds())


def test_the_list_has_the_two_builds_with_their_defines():
    listed = by_name()
    for name, defines in WIDE_FUSED.items():
        assert name in listed, sorted(listed)
        b = listed[name]
        assert b.defines == defines and b.family == "systolic" and b.tag == "f" and b.rows == int(name[1])
        assert b.suffix == "_" + name and b.obj.endswith("csrc/cpecan_kernel_systolic_%s.o" % name)
    # the ring builds of as many waves, which the fused ones stand in for, and the narrower fused builds are still there
    assert {"r6", "r8", "f1", "f2", "f3", "f4"} <= set(listed)
    assert len(builds()) >= 30  # (with the unsuffixed four-wave build)


@needs_hipcc
def test_the_six_wave_sweep_back_shares_a_cu():
    """f6 keeps its eight transition sums in LDS and is held to three waves per SIMD (168 VGPRs: 512 / 3 in allocation
    blocks of 8), so that two six-wave workgroups share a CU as on r6 -- measured faster than the 179 registers the compiler
    takes by itself; nothing may go to scratch for it, and two workgroups' LDS must fit the CU"""
    back = kernel_meta(device_asm(by_name()["f6"]), "cpecan_k_sy_backward_f6")
    assert back["vgpr"] <= 168 and back["spill"] == 0 and back["scratch"] == 0, back["vgpr"]
    assert "scratch_" not in back["body"] and 2 * back["lds"] <= 160 * 1024


@needs_hipcc
def test_no_occupancy_is_forced_on_the_eight_wave_sweep_back():
    """at eight waves only 128 registers would bring a second workgroup to the CU, and forcing them spills: f8 is what
    the compiler makes of it, its sums in registers"""
    back = kernel_meta(device_asm(by_name()["f8"]), "cpecan_k_sy_backward_f8")
    assert 128 < back["vgpr"] <= 256 and back["spill"] == 0 and back["scratch"] == 0, back["vgpr"]
    assert back["lds"] < 16 * 1024  # (no sums in LDS)

"""The hand-scheduled assembly sweeps at two cells per lane (csrc/asm/gen_sweeps.py under CPECAN_ASM_L=2 ->
csrc/asm/cpecan_sweeps_gfx950_l2.s: cpecan_k_asm_forward_l2 / cpecan_k_asm_backward_l2, bands up to 120 k-mers), no GPU:

* on the instruction emulator (gcn_emu.py) every forward cell, every backward cell and every refresh equals the oracle's,
  window by window -- in a child process, asm_l2_child.py, because asm_harness imports the generator, and with it the
  cells per lane, once per process;
* the generator reproduces both tracked assembly files;
* each kernel stays inside the registers it declares, and the two declare few enough to share a SIMD.
"""
import os
import re
import subprocess
import sys
import tempfile

import pytest

import asm_l2_child

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASM = os.path.join(ROOT, "cpecan-signal_amd", "csrc", "asm")
L2_S = os.path.join(ASM, "cpecan_sweeps_gfx950_l2.s")


def _env(**extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("CPECAN_ASM")}
    env.update(extra)
    return env


@pytest.mark.parametrize("case", range(len(asm_l2_child.CASES)),
                         ids=["e%d-every%d-band%s" % (c[5], min(c[3], 999), c[6]) for c in asm_l2_child.CASES])
def test_two_cell_sweeps_on_the_emulator_equal_the_oracle(case):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "asm_l2_child.py"), str(case)], env=_env(CPECAN_ASM_L="2"),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "case ok" in r.stdout


def test_the_cases_cover_the_widths_of_the_default_expansions_and_the_limit():
    widths = [c[6] for c in asm_l2_child.CASES]
    assert 71 in widths and 101 in widths and 120 in widths


def _generate(out, **extra):
    subprocess.check_call([sys.executable, os.path.join(ASM, "gen_sweeps.py"), out], env=_env(**extra), stderr=subprocess.DEVNULL)
    return open(out).read()


def test_generator_reproduces_both_tracked_files():
    with tempfile.TemporaryDirectory() as d:
        assert _generate(os.path.join(d, "l2.s"), CPECAN_ASM_L="2") == open(L2_S).read()
        assert _generate(os.path.join(d, "l3.s")) == open(os.path.join(ASM, "cpecan_sweeps_gfx950.s")).read()
        assert _generate(os.path.join(d, "l3b.s"), CPECAN_ASM_L="3") == open(os.path.join(ASM, "cpecan_sweeps_gfx950.s")).read()


def _metadata(text):
    """{kernel: dict(vgprs, sgprs, lds)} from the .amdgpu_metadata block"""
    out = {}
    for block in text.split("  - .agpr_count:")[1:]:
        get = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))  # noqa: E731
        out[re.search(r"\.name:\s+(\S+)", block).group(1)] = dict(vgprs=get("vgpr_count"), sgprs=get("sgpr_count"),
                                                                  lds=get("group_segment_fixed_size"))
    return out


def test_two_cell_kernels_stay_inside_their_registers_and_share_a_simd():
    text = open(L2_S).read()
    meta = _metadata(text)
    assert sorted(meta) == ["cpecan_k_asm_backward_l2", "cpecan_k_asm_forward_l2"]
    bodies = {}
    for name in meta:
        body = text.split("\n%s:\n" % name)[1].split(".Lend_%s:" % name)[0]
        bodies[name] = body.split("\t.section\t.rodata")[0]
    for name, m in meta.items():
        code = bodies[name]
        top_v = max([int(x) for x in re.findall(r"\bv(\d+)\b", code)] + [int(b) for _, b in re.findall(r"\bv\[(\d+):(\d+)\]", code)])
        top_s = max([int(x) for x in re.findall(r"\bs(\d+)\b", code)] + [int(b) for _, b in re.findall(r"\bs\[(\d+):(\d+)\]", code)])
        assert top_v < m["vgprs"] <= 256 and m["vgprs"] % 8 == 0, (name, top_v, m)
        assert top_s < m["sgprs"] <= 102, (name, top_s, m)      # (s0..s101 are all a wave can name; vcc is allocated on top)
        # the kernel descriptor allocates what the metadata reports
        kd = text.split(".amdhsa_kernel %s\n" % name)[1].split(".end_amdhsa_kernel")[0]
        assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", kd).group(1)) == m["vgprs"]
        assert int(re.search(r"\.amdhsa_accum_offset (\d+)", kd).group(1)) == m["vgprs"]
        assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", kd).group(1)) == m["lds"]
    f, b = meta["cpecan_k_asm_forward_l2"], meta["cpecan_k_asm_backward_l2"]
    # a SIMD's file is 512 registers a lane: a forward and a backward wave of one window fit side by side
    assert (f["vgprs"] + 7) // 8 * 8 + (b["vgprs"] + 7) // 8 * 8 <= 512
    assert (f["vgprs"], b["vgprs"]) == (184, 168)
    # LDS: the events' ring and the rows of k-mers of the forward kernel, the gap-X rows and the refresh's cells of the backward one
    assert (f["lds"], b["lds"]) == (19008, 3584)
    header = open(os.path.join(ROOT, "cpecan-signal_amd", "csrc", "cpecan_asm_gen.h")).read()
    assert "#define ASM2_LDS_F_BYTES %d\n" % f["lds"] in header and "#define ASM2_LDS_B_BYTES %d\n" % b["lds"] in header
    assert "#define ASM2_MAX_WIDTH 120\n" in header and "#define ASM2_ROW_BYTES 5120\n" in header

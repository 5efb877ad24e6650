"""The fused-expectation sweeps back (cpecan_k_wv_backward_fx*, cpecan_k_wv_resweep_fx*) from the compiler's own
metadata: they exist, keep nothing in scratch, and at two cells per lane share a SIMD with the forward sweep (512
registers, handed out in blocks of 8).  At three cells per lane they do not (364 registers against 248 beside the
forward sweep; measured faster than the B-ring path all the same): there only the no-spill check applies.
CPU-only: hipcc cross-compiles gfx950."""
import os
import re
import shutil
import subprocess

import pytest

from cpecan_load import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("cells", [2, 3])
def test_fused_sweeps_back_exist_and_do_not_spill(tmp_path, cells):
    src = os.path.join(ROOT, "cpecan-signal_amd", "csrc", "cpecan_kernel_wave.hip")
    out = str(tmp_path / "wv.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                           "-fno-fast-math", "-Wno-unused-function", "-DWV_L=%d" % cells,
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.dirname(src), "-S",
                           "--cuda-device-only", "-o", out, src], stderr=subprocess.DEVNULL)
    text = open(out).read()
    sfx = "_l%d" % cells

    def meta(name):
        m = text[text.index(".name:           " + name + "\n"):]
        return int(re.search(r"\.vgpr_count:\s+(\d+)", m).group(1)), \
            int(re.search(r"\.vgpr_spill_count:\s+(\d+)", m).group(1))

    fwd = (meta("cpecan_k_wv_forward" + sfx)[0] + 7) // 8 * 8
    for name in ("cpecan_k_wv_backward_fx", "cpecan_k_wv_backward_fx_sw", "cpecan_k_wv_resweep_fx",
                 "cpecan_k_wv_resweep_fx_sw"):
        vgpr, spill = meta(name + sfx)
        assert spill == 0, "%s spills %d VGPRs to scratch" % (name + sfx, spill)
        if cells == 2:
            assert fwd + (vgpr + 7) // 8 * 8 <= 512, "%s (%d) and the forward sweep (%d) no longer share a SIMD" % (
                name + sfx, vgpr, fwd)

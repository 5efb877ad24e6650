"""The echelon general kernel (cpecan_kernel_generale.hip) from the compiler's own metadata, as
test_kernel_resources.py checks the other five: nothing in scratch, at most 168 VGPRs (three waves per SIMD, as the
HDP and strawMan general kernels) and no static LDS beyond the driver's shared total.  CPU-only: hipcc cross-compiles
gfx950."""
import os
import re
import shutil
import subprocess

import pytest

from cpecan_load import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_echelon_kernel_keeps_three_waves_per_simd(tmp_path):
    src = os.path.join(ROOT, "cpecan-signal_amd", "csrc", "cpecan_kernel_generale.hip")
    out = str(tmp_path / "g.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                           "-fno-fast-math", "-Wno-unused-function", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.dirname(src), "-S", "--cuda-device-only", "-o", out, src],
                          stderr=subprocess.DEVNULL)
    text = open(out).read()
    kernel = "cpecan_k_generale"
    meta = next(m for m in text[text.index("amdhsa.kernels:"):].split("\n  - .agpr_count")
                if ".name:           %s\n" % kernel in m)
    vgpr = int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1))
    spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", meta).group(1))
    lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", meta).group(1))
    scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta).group(1))
    body = text[text.index("\n" + kernel + ":"):]
    body = body[:body.index("s_endpgm")]
    assert vgpr <= 168, "%s uses %d VGPRs (at most 168)" % (kernel, vgpr)
    assert lds <= 8, "%s takes %d bytes of static LDS (at most 8)" % (kernel, lds)
    assert spill == 0 and scratch == 0 and "scratch_" not in body, "%s spills to scratch" % kernel

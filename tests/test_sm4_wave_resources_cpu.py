"""The 4-state machine's one-wave-per-alignment kernels (cpecan_kernel_wave4.hip) keep the project's rule for wave
kernels: two waves per SIMD, that is at most 256 of a SIMD's 512 registers, and nothing in scratch -- from the compiler's
own metadata, as tests/test_kernel_resources.py takes it for the 5-state kernels.  CPU-only: hipcc cross-compiles
gfx950."""
import os
import re
import shutil
import subprocess

import pytest

from cpecan_load import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = ("cpecan_k_wave4_l1", "cpecan_k_wave4_l2")


@pytest.fixture(scope="module")
def device_asm(tmp_path_factory):
    src = os.path.join(ROOT, "cpecan-signal_amd", "csrc", "cpecan_kernel_wave4.hip")
    out = str(tmp_path_factory.mktemp("wave4") / "w4.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                           "-fno-fast-math", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.dirname(src), "-S",
                           "--cuda-device-only", "-o", out, src], stderr=subprocess.DEVNULL)
    return open(out).read()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("name", KERNELS)
def test_wave4_kernels_fit_two_waves_per_simd(device_asm, name):
    text = device_asm
    meta = next(m for m in text[text.index("amdhsa.kernels:"):].split("\n  - .agpr_count")
                if ".name:           %s\n" % name in m)
    vgpr = int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1))
    spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", meta).group(1))
    scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta).group(1))
    body = text[text.index("\n" + name + ":"):]
    body = body[:body.index("s_endpgm")]
    print("%s: %d VGPRs, %d spilled, %d bytes of scratch" % (name, vgpr, spill, scratch))
    assert vgpr <= 256, "%s uses %d VGPRs: fewer than two waves per SIMD" % (name, vgpr)
    assert spill == 0 and scratch == 0 and "scratch_" not in body, "%s spills to scratch" % name


def test_the_object_is_one_of_the_plain_sources():
    """cpecan_kernel_wave4.o is listed among HIP_SRC and is no build of the two sweep files (no _<tag><n> suffix)"""
    amd = os.path.join(ROOT, "cpecan-signal_amd")
    objects = subprocess.check_output(["make", "-s", "-C", amd, "print-objects"], text=True).split()
    assert "csrc/cpecan_kernel_wave4.o" in objects
    builds = subprocess.check_output(["make", "-s", "-C", amd, "print-builds"], text=True)
    assert "wave4" not in builds

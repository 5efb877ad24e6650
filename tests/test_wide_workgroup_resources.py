"""The six- and eight-wave builds of the workgroup-per-alignment kernels (CPECAN_FLAG_WIDE_BANDS: bands of 249..376 and
377..504 k-mers) keep the family's budget: at most 128 VGPRs and nothing in scratch.  An eight-wave workgroup puts two
waves on every SIMD; at 128 registers or fewer two such workgroups share a CU.  CPU-only: hipcc cross-compiles gfx950."""
import os
import re
import shutil
import subprocess

import pytest

from cpecan_load import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("rows", [6, 8])
def test_wide_builds_keep_the_register_budget(tmp_path, rows):
    src = os.path.join(ROOT, "cpecan-signal_amd", "csrc", "cpecan_kernel_systolic.hip")
    out = str(tmp_path / "sy.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                           "-fno-fast-math", "-Wno-unused-function", "-DSY_R=%d" % rows,
                           "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.dirname(src), "-S", "--cuda-device-only", "-o", out, src],
                          stderr=subprocess.DEVNULL)
    text = open(out).read()
    kernels = text[text.index("amdhsa.kernels:"):].split("\n  - .agpr_count")
    for stem in ("cpecan_k_sy_forward", "cpecan_k_sy_backward", "cpecan_k_sy_expect"):
        name = "%s_r%d" % (stem, rows)
        meta = [m for m in kernels if ".name:           %s\n" % name in m]
        assert len(meta) == 1, "%s is not in the %d-wave build" % (name, rows)
        vgpr = int(re.search(r"\.vgpr_count:\s+(\d+)", meta[0]).group(1))
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", meta[0]).group(1))
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", meta[0]).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta[0]).group(1))
        threads = int(re.search(r"\.max_flat_workgroup_size:\s+(\d+)", meta[0]).group(1))
        body = text[text.index("\n" + name + ":"):]
        body = body[:body.index("s_endpgm")]
        assert threads == 64 * rows
        assert vgpr <= 128, "%s uses %d VGPRs" % (name, vgpr)
        assert spill == 0 and scratch == 0 and "scratch_" not in body, "%s spills to scratch" % name
        assert lds <= 64 * 1024, "%s takes %d bytes of static LDS" % (name, lds)


def test_library_exports_only_the_declared_names():
    """the wide builds add kernels and two build records, no entry point: what libcpecan_hip.so exports under the
    cpecan_hip_ prefix is still exactly what include/cpecan_hip.h declares, and the records of the two builds are there"""
    lib = os.path.join(ROOT, "cpecan-signal_amd", "libcpecan_hip.so")
    if not os.path.exists(lib) or shutil.which("nm") is None:
        pytest.skip("library not built, or no nm")
    names = set(l.split()[-1] for l in subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True).splitlines())
    header = open(os.path.join(ROOT, "include", "cpecan_hip.h")).read()
    declared = set(re.findall(r"\b(cpecan_hip_[a-z0-9_]+)\s*\(", header))
    assert set(n for n in names if n.startswith("cpecan_hip_")) == declared
    assert {"cpecan_systolic_build_r6", "cpecan_systolic_build_r8"} <= names

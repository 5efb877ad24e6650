"""CPECAN_SM4_WAVE=1 through libcpecan_host.so: every 4-state posterior batch of the host library then carries
CPECAN_FLAG_SM4_WAVE.  The stream classes narrow reads on the wave kernels and wide ones on the general kernel, in
chunks of their own, and every read's pairs are those of the call on that read alone in a process without the variable;
the driver (vanillaAlign --fourState) writes the same bytes with the variable as without.  The library reads the
variable, so each run is a process of its own (tests/sm4_wave_host_child.py)."""
import json
import os
import subprocess
import sys

import pytest

import stream_api as sa
from test_vanilla_align_cli_gpu import EXE, _guide, _npread_with_forward_complement

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def env_with(value):
    env = {k: v for k, v in os.environ.items() if k != "CPECAN_SM4_WAVE"}
    if value is not None:
        env["CPECAN_SM4_WAVE"] = value
    return env


def child(tmp_path, how, value):
    path = str(tmp_path / ("%s_%s.json" % (how, value)))
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(HERE, "sm4_wave_host_child.py"), path,
                        how], env=env_with(value), capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.load(open(path))


def test_the_stream_classes_narrow_reads_on_the_wave_kernel(tmp_path):
    off = child(tmp_path, "both", None)
    on = child(tmp_path, "stream", "1")
    assert all(len(r) > 0 for r in off["alone"])
    assert on["reads"] == off["alone"] == off["reads"]
    # one class per chunk: the narrow reads on the wave kernel (reported as the 5-state wave kernels are: general,
    # wave 1, rows 0), the wide ones on the general kernel
    kinds = sorted((c["kernel"], c["wave"], c["rows"], c["maxWidth"] <= 128, c["nReads"]) for c in on["chunks"])
    assert kinds == [(sa.KERNEL_GENERAL, 0, 0, False, 3), (sa.KERNEL_GENERAL, 1, 0, True, 3)], on["chunks"]
    # without the variable the stream is what it was: one class, the general kernel
    assert all((c["kernel"], c["wave"], c["rows"]) == (sa.KERNEL_GENERAL, 0, 0) for c in off["chunks"]), off["chunks"]
    assert sum(c["nReads"] for c in off["chunks"]) == 6


def test_the_driver_writes_the_same_bytes(golden_dir, zymo_read, template_model, tmp_path):
    """vanillaAlign --fourState -x 50 on the shipped read (bands of about 100 cells: two cells per lane)"""
    _, _, cigar = _guide(zymo_read, template_model)
    npread, _ = _npread_with_forward_complement(golden_dir, zymo_read, tmp_path)
    written = {}
    for value in (None, "1"):
        tsv = str(tmp_path / ("out_%s.tsv" % value))
        cmd = [EXE, "--fourState", "-T", os.path.join(golden_dir, "template_median68pA.model"), "-C",
               os.path.join(golden_dir, "complement_median68pA_pop2.model"), "-q", npread, "-r",
               os.path.join(golden_dir, "ZymoRef.txt"), "-u", tsv, "-L", "zymo_read", "-x", "50"]
        r = subprocess.run(cmd, input=cigar, env=env_with(value), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "SUCCESS" in r.stderr, r.stderr[-2000:]
        written[value] = (open(tsv, "rb").read(), r.stdout)
    assert written["1"] == written[None] and written[None][0].count(b"\n") > 300

"""What of the streamed E-step needs no device: the new names are exported, declared and bound; a C program compiles
against the two headers alone; and the class the stream gives an E-step read (expectations_request, through the
cpecan_stream_expectations_class hook) is what cpecan_hip_plan_dispatch answers for that width in
CPECAN_MODE_EXPECTATIONS under the flags the machine's create call passes -- the environment's fused-E-step switches
among them."""
import ctypes as C
import os
import re
import subprocess

import pytest

import host_api as h
import stream_estep_api as se
from cpecan_load import ROOT, binding
from harness import BATCH_ENV

cp = binding()
LIBDIR = os.path.join(ROOT, "cpecan-signal_amd")
# the switches the host library's create calls turn into flags (csrc/host/cpecan_api.c), per machine
SWITCHES = {
    "strawman": {},
    "dna5": {},
    "vanilla": {"CPECAN_VANILLA_FUSED_ESTEP": cp.FLAG_VANILLA_FUSED_ESTEP,
                "CPECAN_WIDE_BANDS_VANILLA_FUSED_ESTEP": cp.FLAG_WIDE_BANDS_VANILLA_FUSED_ESTEP},
    "hdp": {"CPECAN_HDP_FUSED_ESTEP": cp.FLAG_HDP_FUSED_ESTEP,
            "CPECAN_WIDE_BANDS_HDP_FUSED_ESTEP": cp.FLAG_WIDE_BANDS_HDP_FUSED_ESTEP,
            "CPECAN_HDP_FOUR_CELLS_FUSED_ESTEP": cp.FLAG_HDP_FOUR_CELLS_FUSED_ESTEP},
}
BASE = {"strawman": (cp.KERNEL_AUTO, cp.FLAG_SMALL_FOOTPRINT), "dna5": (cp.KERNEL_GENERAL, 0),
        "vanilla": (cp.KERNEL_AUTO, 0), "hdp": (cp.KERNEL_AUTO, 0)}
# either side of every width at which a machine's E-step changes kernels (64/128/192 cells of the 5-state machine; 120,
# 184, 248, 376, 504 k-mers of the signal machines), and far past the last
WIDTHS = [1, 50, 64, 65, 120, 121, 128, 129, 184, 185, 192, 193, 248, 249, 376, 377, 504, 505, 900]


def test_the_new_names_are_declared_exported_and_bound():
    api = open(os.path.join(ROOT, "include", "cpecan_api.h")).read()
    hip = open(os.path.join(ROOT, "include", "cpecan_hip.h")).read()
    host = C.CDLL(h.LIB_PATH)
    for name in se.ESTEP_EXPORTS:
        assert re.search(r"\b%s\s*\(" % name, api) and hasattr(host, name), name
    assert re.search(r"typedef void \(\*cpecan_stream_done_fn\)\(void \*arg, int64_t tag, bool refused\);", api)
    name = "cpecan_hip_batch_sum_expectations"
    assert re.search(r"\bint %s\(cpecan_batch \*batch, double \*out\);" % name, hip)
    assert name in cp.EXPORTS and hasattr(C.CDLL(cp.LIB_PATH), name) and hasattr(cp.Batch, "sum_expectations")
    assert list(getattr(cp.lib(), name).argtypes) == [C.c_void_p, C.c_void_p]


def test_a_c_program_compiles_against_the_headers_alone(tmp_path):
    exe = str(tmp_path / "stream_estep_api_test")
    subprocess.run(["gcc", "-O1", "-std=gnu99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "stream_estep_api_test.c"), "-o", exe, "-L" + LIBDIR,
                    "-lcpecan_host", "-lcpecan_hip", "-Wl,-rpath," + LIBDIR, "-lm", "-lpthread"], check=True)
    env = {k: v for k, v in os.environ.items() if k not in BATCH_ENV}
    r = subprocess.run([exe, "100"], capture_output=True, text=True, timeout=120, env=env)
    d = cp.plan_dispatch(cp.MACHINE_STRAWMAN, cp.MODE_EXPECTATIONS, cp.KERNEL_AUTO, cp.FLAG_SMALL_FOOTPRINT, 100)
    assert r.returncode == 0 and r.stdout.split() == ["ok", str(d["kernel"]), str(d["wave"]), str(d["rows"])], r


def _subsets(names):
    out = [()]
    for n in names:
        out += [s + (n,) for s in out]
    return out


@pytest.mark.parametrize("kind", ["strawman", "dna5", "vanilla", "hdp"])
def test_the_streams_class_is_the_plan_under_the_create_calls_flags(kind, monkeypatch):
    for name in BATCH_ENV + tuple(n for sw in SWITCHES.values() for n in sw):
        monkeypatch.delenv(name, raising=False)
    machine = se.MACHINE_OF[kind]
    kernel, base = BASE[kind]
    # the switches that send a wide band's E-step to the workgroup kernels at all (read by the C-ABI itself)
    wide = {"vanilla": "CPECAN_WIDE_BANDS_VANILLA_ESTEP", "hdp": "CPECAN_WIDE_BANDS_HDP_ESTEP"}.get(kind)
    seen = set()
    for wide_on in ([False, True] if wide else [False]):
        if wide_on:
            monkeypatch.setenv(wide, "1")
        for on in _subsets(sorted(SWITCHES[kind])):
            for name in SWITCHES[kind]:
                monkeypatch.setenv(name, "1" if name in on else "0")
            flags = base
            for name in on:
                flags |= SWITCHES[kind][name]
            for w in WIDTHS:
                for step in (True, False):
                    d = cp.plan_dispatch(machine, cp.MODE_EXPECTATIONS, kernel, flags, w, step)
                    assert se.expectations_class(machine, w, step) == (d["kernel"], d["wave"], d["rows"]), (on, w, step)
                    seen.add((d["kernel"], d["wave"], d["rows"]))
    assert len(seen) >= (2 if kind == "dna5" else 3), seen  # (the widths do cross the machine's thresholds)


@pytest.mark.parametrize("kind", ["sm4", "echelon"])
def test_a_machine_without_an_e_step_has_no_class(kind):
    k, w, r = C.c_int32(), C.c_int32(), C.c_int32()
    rc = se.lib().cpecan_stream_expectations_class(se.MACHINE_OF[kind], 100, 1, C.byref(k), C.byref(w), C.byref(r))
    assert rc == cp.EINVAL

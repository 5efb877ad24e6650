"""Time of the model-table create calls on two builds of the library, alternating, for the record in DESIGN.md section 5.

For every library given (name=path of a libcpecan_hip.so), --repeats times after one warm-up round, the tables cleared
before every call:
  the four threaded creates at --models models (default 1024) and 16 threads -- cpecan_hip_models_create,
  _models_create_scaled, _modelsv_create, _modelsv_create_scaled -- as the library's own CPECAN_TIMING "TOTAL" line;
  the four creates of a handful of models, --few (default 8) in one call onto a table that already holds as many --
  cpecan_hip_models4_create, _models5_create, _modelse_create, _modelsh_create -- by the wall clock around the call.
Prints min, median and max per call and library.
Run on the GPU box: python tests/tools/bench_model_tables.py parent=PATH branch=PATH [--models N] [--few N]"""
import argparse
import ctypes as C
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
os.environ["CPECAN_TIMING"] = "1"
import pyoracle as o  # noqa: E402  (model construction only)
import synth  # noqa: E402
import test_vanilla_gpu as tv  # noqa: E402
from harness import cp  # noqa: E402

THREADS = 16


class Stderr:
    """the process's stderr in a file while a call runs: the library's timing lines"""

    def __enter__(self):
        sys.stderr.flush()
        self.saved, self.tmp = os.dup(2), tempfile.TemporaryFile()
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode()
        self.tmp.close()


def context_on(path):
    """a binding Context whose calls go to the library at `path` (the binding's argument types)"""
    L = C.CDLL(path)
    L.cpecan_hip_last_error.restype = C.c_char_p
    for name in cp.EXPORTS:
        if getattr(cp.lib(), name).argtypes is not None:
            getattr(L, name).argtypes = getattr(cp.lib(), name).argtypes
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="+", help="name=path of a libcpecan_hip.so")
    ap.add_argument("--models", type=int, default=1024)
    ap.add_argument("--few", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    print("box: %s, %s" % (os.uname().nodename, torch.cuda.get_device_name(0)), flush=True)
    n, few = a.models, a.few
    match, gap_x, gap_y = synth.synthetic_pore_model()
    skip = np.concatenate([tv.skip_bins(0), tv.skip_bins(0)])
    vm = o.VanillaModel(match, skip, gap_y)
    rng = np.random.default_rng(1)
    S = np.column_stack([rng.uniform(0.95, 1.05, n), rng.uniform(-5, 5, n), rng.uniform(0.9, 1.1, n),
                         rng.uniform(0.9, 1.2, n), rng.uniform(0.9, 1.2, n)])
    sm3 = [(cp.NANOPORE_TRANSITIONS, match, gap_x, gap_y)] * n
    van = [(vm.scalars, match, skip, gap_y)] * n
    m4 = o.Sm4Model(match, gap_y)
    m5 = o.Sm5Model()
    nhdp = o.load_nhdp(os.path.join(ROOT, "tests", "golden", "testTemplate.nhdp"))
    calls = [  # (label, the library's lap name or None for the wall clock, call(ctx))
        ("models_create", "models_create", lambda c: c.models_create(sm3, threads=THREADS)),
        ("models_create_scaled", "models_create_scaled", lambda c: c.models_create_scaled(sm3[0], S, threads=THREADS)),
        ("modelsv_create", "modelsv_create", lambda c: c.modelsv_create(van, threads=THREADS)),
        ("modelsv_create_scaled", "modelsv_create_scaled", lambda c: c.modelsv_create_scaled(van[0], S, threads=THREADS)),
        ("models4_create x%d" % few, None, lambda c: c.models4_create([(m4.transitions, match, m4.gap_x, gap_y)] * few)),
        ("models5_create x%d" % few, None, lambda c: c.models5_create([(list(m5.c.t), m5.match, m5.gx, m5.gy)] * few)),
        ("modelse_create x%d" % few, None, lambda c: c.modelse_create([((0.1, 0.1), match, skip, gap_y)] * few)),
        ("modelsh_create x%d" % few, None, lambda c: c.modelsh_create(
            [(cp.NANOPORE_TRANSITIONS, nhdp["alphabet"], nhdp["grid"], nhdp["y"], nhdp["slope"], nhdp["kmer_row"])] * few)),
    ]
    libs = []
    for spec in a.libs:
        name, path = spec.split("=", 1)
        L = context_on(path)
        h = C.c_void_p()
        assert L.cpecan_hip_ctx_create(0, C.byref(h)) == 0
        libs.append((name, L, h))
    times = {(label, name): [] for label, _, _ in calls for name, _, _ in libs}
    real_lib = cp.lib
    for rep in range(a.repeats + 1):  # the first round warms up (code objects, pinned memory, the allocator's cache)
        for label, lap, call in calls:
            for name, L, h in libs:
                cp.lib = lambda L=L: L
                ctx = cp.Context.__new__(cp.Context)  # the binding's methods on this library's handle
                ctx.h = h
                ctx.models_clear()
                if lap is None:
                    call(ctx)  # the table the timed call grows
                with Stderr() as err:
                    t0 = time.perf_counter()
                    call(ctx)
                    t1 = time.perf_counter()
                ms = (t1 - t0) * 1e3
                if lap is not None:
                    ms = float(re.search(r"\] %s: TOTAL ([0-9.]+) ms" % lap, err.text).group(1))
                if rep:
                    times[(label, name)].append(ms)
                ctx.models_clear()
                ctx.h = None
    cp.lib = real_lib
    print("%d models at %d threads (the library's TOTAL lap); %d models onto %d (wall clock); ms, %d repeats" % (
        n, THREADS, few, few, a.repeats))
    for label, _, _ in calls:
        for name, _, _ in libs:
            t = times[(label, name)]
            print("%-24s %-8s min %8.2f  median %8.2f  max %8.2f" % (label, name, min(t), float(np.median(t)), max(t)))
    for _, L, h in libs:
        L.cpecan_hip_ctx_destroy(h)


if __name__ == "__main__":
    main()

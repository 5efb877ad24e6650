"""Set-up and per-iteration cost of the vanilla machine's per-read models, for the record in DESIGN.md section 5.

For N reads of one strand (default 1024), in alternation and as medians of --repeats runs (default 5), threads = 16:
  (i)   the host-scaled route: two tables per read copied and scaled on the host as emissions_signal_scaleModel does
        (the checker's C restatement), then cpecan_hip_modelsv_create -- on --parent-lib, the library of the commit
        this one is compared with, and on this tree's library;
  (ii)  cpecan_hip_modelsv_create_scaled on this tree's library;
  (iii) one E-step iteration (bins in, 61 sums out) of em.PersistentVanillaEStep against one with the context cleared,
        the tables scaled and uploaded again and the batch created again (on --parent-lib and on this tree's library),
        on the shape of tools/bench_machines.py: 2000 k-mers x 4000 events, band 100.
Run on the GPU box: python tests/tools/bench_vanilla_models.py [--parent-lib PATH] [--reads N] [--estep-reads N]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import pyoracle as o  # noqa: E402  (model construction and the host's scaleModel only)
import synth  # noqa: E402
import test_vanilla_gpu as tv  # noqa: E402
from cpecan_load import em  # noqa: E402
from harness import band_params, cp  # noqa: E402

THREADS = 16
FUDGE = (float(np.float32(0.17)), float(np.float32(0.55)))


class Raw:
    """the calls of the host-scaled route on a library given by its path (the parent commit's has no binding of its
    own in this tree); argument types are the binding's"""
    NAMES = ("cpecan_hip_ctx_create", "cpecan_hip_ctx_destroy", "cpecan_hip_models_clear", "cpecan_hip_modelsv_create",
             "cpecan_hip_batch_create_vanilla", "cpecan_hip_batch_run", "cpecan_hip_batch_sync",
             "cpecan_hip_batch_expectations_device_ptr", "cpecan_hip_batch_destroy")

    def __init__(self, path):
        self.L = C.CDLL(path)
        self.L.cpecan_hip_last_error.restype = C.c_char_p
        for name in self.NAMES:
            getattr(self.L, name).argtypes = getattr(cp.lib(), name).argtypes
        self.ctx = C.c_void_p()
        self.ok(self.L.cpecan_hip_ctx_create(0, C.byref(self.ctx)))

    def ok(self, rc):
        if rc != 0:
            raise RuntimeError("%d: %s" % (rc, self.L.cpecan_hip_last_error().decode()))

    def models_clear(self):
        self.ok(self.L.cpecan_hip_models_clear(self.ctx))

    def modelsv_create(self, scalars, tables, skip, threads):
        """tables: per read (match, gap_y)"""
        descs = (cp.VanillaModelDesc * len(tables))()
        for d, (match, gap_y) in zip(descs, tables):
            d.m_to_y_not_x, d.e_to_e, d.end_match_prob, d.end_from_x_prob, d.end_from_y_prob = [float(v) for v in scalars]
            d.match_probs, d.skip_probs, d.gap_y_probs = match.ctypes.data, skip.ctypes.data, gap_y.ctypes.data
        ids = np.zeros(len(tables), np.int32)
        self.ok(self.L.cpecan_hip_modelsv_create(self.ctx, C.cast(descs, C.c_void_p), len(tables), threads,
                                                 ids.ctypes.data))
        return ids

    def e_step(self, items, batch, bp, dev):
        """batch created, run, the 61 sums of its models added on the device, batch destroyed"""
        import torch
        xb = np.frombuffer(bytes(batch["x_chars"]), np.uint8)
        ev = np.ascontiguousarray(batch["events"], dtype=np.float64).reshape(-1)
        an = np.ascontiguousarray(batch["anchors"], dtype=np.int64).reshape(-1, 2)
        h = C.c_void_p()
        self.ok(self.L.cpecan_hip_batch_create_vanilla(self.ctx, items.ctypes.data, items.shape[0], xb.ctypes.data,
                                                       xb.size, ev.ctypes.data, ev.size // 3, an.ctypes.data, an.shape[0],
                                                       C.byref(bp), cp.FLAG_EXPECTATIONS, C.byref(h)))
        try:
            self.ok(self.L.cpecan_hip_batch_run(h))
            self.ok(self.L.cpecan_hip_batch_sync(h))
            p, n = C.c_void_p(), C.c_int64()
            self.ok(self.L.cpecan_hip_batch_expectations_device_ptr(h, C.byref(p), C.byref(n)))
            total = torch.as_tensor(em()._DeviceDoubles(p.value, n.value), device=dev).view(-1, 61).sum(0).cpu().numpy()
        finally:
            self.L.cpecan_hip_batch_destroy(h)
        return total

    def close(self):
        self.L.cpecan_hip_ctx_destroy(self.ctx)


def host_scaled_tables(match, gap_y, scalings):
    """what a caller of the host-scaled route does per read: its own copy of the two tables, the match table scaled"""
    out = []
    for sc in scalings:
        m = match.copy()
        o.lib().orc_scale_model(m.ctypes.data_as(C.c_void_p), *[float(v) for v in sc])
        out.append((m, gap_y.copy()))
    return out


def median_ms(samples):
    return float(np.median(samples)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libcpecan_hip.so of the commit to compare with")
    ap.add_argument("--reads", type=int, default=1024)
    ap.add_argument("--estep-reads", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    print("box: %s, %s" % (os.uname().nodename, torch.cuda.get_device_name(0)), flush=True)
    libs = [("this tree", Raw(cp.LIB_PATH))]
    if a.parent_lib:
        libs.insert(0, ("parent", Raw(a.parent_lib)))
    match, _, gap_y = synth.synthetic_pore_model()
    skip = np.concatenate([tv.skip_bins(0), tv.skip_bins(0)])
    base = o.VanillaModel(match, skip, gap_y, *FUDGE)
    rng = np.random.default_rng(1)
    n = a.reads
    S = np.column_stack([rng.uniform(0.95, 1.05, n), rng.uniform(-5, 5, n), rng.uniform(0.9, 1.1, n),
                         rng.uniform(0.9, 1.2, n), rng.uniform(0.9, 1.2, n)])
    ctx = cp.Context(0)

    # (i) against (ii): set-up of n models
    t_scale, t_create, t_scaled = [], {name: [] for name, _ in libs}, []
    for rep in range(a.repeats + 1):  # the first round warms up (code objects, pinned memory, the allocator's cache)
        for name, raw in libs:
            raw.models_clear()
            t0 = time.perf_counter()
            tables = host_scaled_tables(match, gap_y, S)
            t1 = time.perf_counter()
            raw.modelsv_create(base.scalars, tables, skip, THREADS)
            t2 = time.perf_counter()
            del tables
            if rep:
                t_scale.append(t1 - t0)
                t_create[name].append(t2 - t1)
        ctx.models_clear()
        t0 = time.perf_counter()
        ctx.modelsv_create_scaled((base.scalars, match, skip, gap_y), S, threads=THREADS)
        t1 = time.perf_counter()
        if rep:
            t_scaled.append(t1 - t0)
    hs = median_ms(t_scale)
    print("models: %d reads, threads %d, medians of %d" % (n, THREADS, a.repeats))
    for name, _ in libs:
        mc = median_ms(t_create[name])
        print("(i)  %-9s host scaling %.1f ms + modelsv_create %.1f ms = %.1f ms" % (name, hs, mc, hs + mc))
    ms = median_ms(t_scaled)
    print("(ii) this tree modelsv_create_scaled %.1f ms" % ms, flush=True)
    for raw in [r for _, r in libs]:
        raw.models_clear()
    ctx.models_clear()

    # (iii) one E-step iteration: persistent against rebuilt
    n = a.estep_reads
    batch = synth.make_batch(5, n, 2000, 4000, anchor_every=50)
    bp = band_params(0.01, 1000, 40, 100)
    S = batch["scalings"]
    bins = [np.concatenate([tv.skip_bins(k), tv.skip_bins(k + 1)]) for k in range(a.repeats + 1)]
    step = em().PersistentVanillaEStep(cp, [ctx], batch, bp, range(n), [(base.scalars, match, skip, gap_y)], [0] * n)
    items = np.zeros(n, cp.ITEM_DTYPE)
    for i, it in enumerate(batch["items"]):
        items[i] = (it["x_offset"], it["lX"], it["y_offset"], it["lY"], it["anchor_offset"], it["n_anchors"], i, 1, 1, 0)
    t_pers, t_reb, worst = [], {name: [] for name, _ in libs}, 0.0
    for rep in range(a.repeats + 1):
        t0 = time.perf_counter()
        got = step(bins[rep])
        t1 = time.perf_counter()
        if rep:
            t_pers.append(t1 - t0)
        for name, raw in libs:
            t0 = time.perf_counter()
            raw.models_clear()
            raw.modelsv_create(base.scalars, host_scaled_tables(match, gap_y, S), bins[rep], THREADS)
            want = raw.e_step(items, batch, bp, dev)
            t1 = time.perf_counter()
            if rep:
                t_reb[name].append(t1 - t0)
            worst = max(worst, float(np.max(np.abs(got - want) / np.abs(want))))
    print("E-step iteration: %d reads of 2000 k-mers x 4000 events, band 100 (%s), medians of %d" % (
        n, step.batches[0][1].info().get("family", "general"), a.repeats))
    print("(iii) persistent (set_skip_probs + run + sums) %.1f ms" % median_ms(t_pers))
    for name, _ in libs:
        print("(iii) rebuilt on %-9s (clear + host scaling + modelsv_create + batch + run + sums) %.1f ms" % (
            name, median_ms(t_reb[name])))
    print("largest relative difference of the 61 sums, persistent against rebuilt: %.3g" % worst, flush=True)
    step.close()
    ctx.close()
    for _, raw in libs:
        raw.close()


if __name__ == "__main__":
    main()

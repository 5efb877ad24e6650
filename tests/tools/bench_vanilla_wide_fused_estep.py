"""The vanilla machine's E-step on the workgroup-per-alignment kernels with its expectations summed inside the sweep back
(CPECAN_FLAG_WIDE_BANDS_VANILLA_FUSED_ESTEP beside CPECAN_FLAG_WIDE_BANDS_VANILLA_ESTEP: the _vf4 / _vf6 / _vf8 builds)
against the _ve builds' path through the ring of backward cells and cpecan_k_sy_expect -- what a batch with the wide-bands
flag alone runs -- for the paragraph in DESIGN.md.  The batches are bench_vanilla_wide_estep.py's: vanilla reads of 2 000
k-mers x 4 000 events, a scaled model per read, a widest band of 235 (four waves), 324 (six) and 454 k-mers (eight).
  stage [reads [ring]]   one process, one device: per band a batch with the wide-bands flag and one with both flags, run
                      in turn (ring, fused, ring, fused, ...), medians of five wall times of run() + sync() after a
                      warm-up, cells from the batch's own per-read counts.  With `ring`, and with a library that does not
                      know the flag (the parent commit's, through CPECAN_HIP_LIB), the ring batch alone.
  ab PARENT_LIB [reads]   three processes in turn, three times each, another one first each time: `stage reads ring` with
                      CPECAN_HIP_LIB=PARENT_LIB,
                      the same with this tree's library (the un-flagged figure of this tree beside the parent's, like
                      for like: one batch alive), and `stage reads` with this tree's library; medians of the processes'
                      medians.
Run on the GPU box: python tests/tools/bench_vanilla_wide_fused_estep.py stage|ab ..."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "tools"), os.path.join(ROOT, "oracle")]

PROCESSES = 3
RING = 1024    # CPECAN_FLAG_WIDE_BANDS_VANILLA_ESTEP
FLAG = 32768   # CPECAN_FLAG_WIDE_BANDS_VANILLA_FUSED_ESTEP


def stage(n, ring_only=False):
    import pyoracle as o  # (model construction only)
    import synth
    from bench_vanilla_wide import CONFIGS, REPS  # (the same batches)
    from harness import band_params, cp, make_items
    from test_vanilla_gpu import skip_bins
    ctx = cp.Context(0)
    out = {}
    for label, every, e in CONFIGS:
        batch = synth.make_batch(5, n, 2000, 4000, anchor_every=every)
        bp = band_params(0.01, 1000, 40, e)
        models = [o.VanillaModel(m, skip_bins(i % 8), gy, 0.17 if i % 2 == 0 else 0.14, 0.55 if i % 2 == 0 else 0.49)
                  for i, (m, _, gy) in enumerate(batch["models"])]
        ctx.models_clear()
        ctx.modelsv_create([(m.scalars, m.match, m.skip, m.gap_y) for m in models])
        del models
        items = make_items(batch, (1, 1))
        knows = cp.plan_expectation_pass(cp.MACHINE_VANILLA, cp.MODE_EXPECTATIONS, cp.KERNEL_AUTO, RING | FLAG, 300) == 1
        forms = (("ring", RING), ("fused", RING | FLAG)) if knows and not ring_only else (("ring", RING),)
        bs = [cp.Batch(ctx, items, batch["x_chars"], batch["events"], batch["anchors"], bp,
                       flags=cp.FLAG_EXPECTATIONS | f, vanilla=True) for _, f in forms]
        times = [[] for _ in bs]
        for b in bs:  # warm-up
            b.run(); b.sync()
        for _ in range(REPS):
            for k, b in enumerate(bs):  # ring, fused, ring, fused, ...
                t0 = time.perf_counter(); b.run(); b.sync(); times[k].append(time.perf_counter() - t0)
        for k, ((form, _), b) in enumerate(zip(forms, bs)):
            info = b.info()
            assert info["family"] == "workgroup" and info["fused_expectations"] == k, info
            cells = int(b.counts()[2].sum())
            med = statistics.median(times[k])
            out["%s %s" % (label, form)] = med * 1e3
            print("%s E-step %s: %d reads, widest band %d, %s kernel (%d waves), %d cells, runs (ms) %s, median %.1f ms, "
                  "spread %.1f ms, %.2f Gcells/s" % (
                      label, form, b.n, info["max_band_width"], info["kernel"], info["waves_per_workgroup"], cells,
                      " ".join("%.1f" % (t * 1e3) for t in times[k]), med * 1e3,
                      (max(times[k]) - min(times[k])) * 1e3, cells / med / 1e9), flush=True)
        if len(bs) == 2:
            print("%s E-step: ring / fused = %.3fx" % (label, statistics.median(times[0]) / statistics.median(times[1])),
                  flush=True)
        for b in bs:
            b.close()
    ctx.close()
    print("medians " + json.dumps(out), flush=True)


def ab(parent_lib, n):
    sides = ("parent", "branch alone", "branch")
    runs = dict((s, []) for s in sides)
    for k in range(PROCESSES):
        for side in sides[k % 3:] + sides[:k % 3]:  # in turn, another one first each time (a box warms up over a visit)
            env = dict(os.environ)
            env.pop("CPECAN_HIP_LIB", None)
            if side == "parent":
                env["CPECAN_HIP_LIB"] = os.path.abspath(parent_lib)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "stage", str(n)] +
                               (["ring"] if side != "branch" else []), env=env,
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
            if r.returncode != 0:
                raise RuntimeError("%s failed (%d): %s" % (side, r.returncode, r.stderr[-2000:]))
            for line in r.stdout.splitlines():
                print("%s: %s" % (side, line), flush=True)
            runs[side].append(json.loads([l for l in r.stdout.splitlines() if l.startswith("medians ")][-1][8:]))
    for side in sides:
        for key in runs[side][0]:
            v = [r[key] for r in runs[side]]
            print("ab %s, %s: process medians (ms) %s, median %.1f, spread %.1f" % (
                side, key, " ".join("%.1f" % x for x in v), statistics.median(v), max(v) - min(v)), flush=True)
    for label in [k[:-len(" ring")] for k in runs["branch"][0] if k.endswith(" ring")]:
        p = statistics.median(r[label + " ring"] for r in runs["parent"])
        a = statistics.median(r[label + " ring"] for r in runs["branch alone"])
        q = statistics.median(r[label + " ring"] for r in runs["branch"])
        f = statistics.median(r[label + " fused"] for r in runs["branch"])
        print("ab %s: un-flagged batch alone, parent %.1f ms, branch %.1f ms (parent / branch %.3fx); beside the fused "
              "batch, ring %.1f ms, fused %.1f ms (ring / fused %.3fx)" % (label, p, a, p / a, q, f, q / f), flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "stage"
    if what == "ab":
        ab(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 1024)
    else:
        stage(int(sys.argv[2]) if len(sys.argv) > 2 else 1024, len(sys.argv) > 3 and sys.argv[3] == "ring")

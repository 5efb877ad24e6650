"""The HDP machine's E-step on the four-cell wave build with its expectations summed and its assignments selected inside
the sweep back (CPECAN_FLAG_HDP_FOUR_CELLS_FUSED_ESTEP: the _hf4 build, bands of 185..248 k-mers) against the same
kernels' path through the ring of backward cells and cpecan_k_wv_expect_h4 -- what a batch without the flag runs -- for
the paragraph in DESIGN.md (section 5, round 28).
The shape: reads of 2 000 k-mers (16 distinct ones repeated, events drawn around the modes of tests/golden/
testTemplate.nhdp, an anchor every 25 k-mers), assignment threshold 0.05, at two even diagonal expansions, 120 and 160:
a widest band of 196 and of 236 k-mers, near the two ends of the build's range.  The tool asserts four cells per lane and
prints the width.
  stage [reads [ring]]   one process, one device: per band a batch without the flag and one with it, run in turn (ring,
                      fused, ring, fused, ...), medians of three wall times of run() + sync() after a warm-up, cells
                      from the batch's own per-read counts.  With `ring`, and with a library that does not know the flag
                      (the parent commit's, through CPECAN_HIP_LIB), the batch without the flag alone.
  ab PARENT_LIB [reads]   three processes in turn, three times each: `stage reads ring` with CPECAN_HIP_LIB=PARENT_LIB, the
                      same with this tree's library (the un-flagged figure of this tree beside the parent's, like for
                      like: one batch alive), and `stage reads` with this tree's library; medians of the processes' medians.
The share of windows the fused batch sends down the re-sweep is read from a kernel trace of `stage`: the re-sweep kernel
returns at once for an alignment whose window needs none, so the summed duration of cpecan_k_wv_resweep_fx_hf4 over that
of cpecan_k_wv_backward_fx_hf4 bounds it from above.
Run on the GPU box: python tests/tools/bench_hdp_four_cells_fused_estep.py stage|ab ..."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]

REPS = 3
DISTINCT = 16
EXPANSIONS = (120, 160)
CELLS = {120: 4, 160: 4}
THRESHOLD = 0.05
FLAG = 262144  # CPECAN_FLAG_HDP_FOUR_CELLS_FUSED_ESTEP


def reads(ctx, n):
    import pyoracle as o  # (the .nhdp reader only)
    from harness import cp, hdp_batch, make_items
    nhdp = o.load_nhdp(os.path.join(ROOT, "tests", "golden", "testTemplate.nhdp"))
    batch, _ = hdp_batch(5, min(n, DISTINCT), 2000, 25, nhdp)
    distinct = len(batch["items"])
    batch["items"] = [dict(batch["items"][i % distinct], model=0) for i in range(n)]
    ctx.modelsh_create([(cp.NANOPORE_TRANSITIONS, nhdp["alphabet"], nhdp["grid"], nhdp["y"], nhdp["slope"],
                         nhdp["kmer_row"])])
    return batch, make_items(batch, (1, 1))


def timed(b):
    t0 = time.perf_counter()
    b.run()
    b.sync()
    return time.perf_counter() - t0


def stage(n, ring_only=False):
    from harness import band_params, cp
    ctx = cp.Context(0)
    batch, items = reads(ctx, n)
    out = {}
    for e in EXPANSIONS:
        bp = band_params(THRESHOLD, 1000, 40, e)
        knows = cp.plan_expectation_pass(cp.MACHINE_HDP, cp.MODE_EXPECTATIONS, cp.KERNEL_AUTO, FLAG, 200) == 1
        forms = (("ring", 0), ("fused", FLAG)) if knows and not ring_only else (("ring", 0),)
        # (both batches stay alive: an HDP wave batch is one stream group on the context's lanes, and they run in turn)
        bs = [cp.Batch(ctx, items, batch["x_chars"], batch["events"], batch["anchors"], bp,
                       flags=cp.FLAG_EXPECTATIONS | f, hdp=True) for _, f in forms]
        times = [[] for _ in bs]
        for b in bs:  # warm-up (and the run that sizes the pair lists)
            timed(b)
            b.counts()
        for _ in range(REPS):
            for k, b in enumerate(bs):  # ring, fused, ring, fused, ...
                times[k].append(timed(b))
        for k, ((form, _), b) in enumerate(zip(forms, bs)):
            info = b.info()
            assert info["family"] == "wave" and info["cells_per_lane"] == CELLS[e] and info["fused_expectations"] == k, info
            assert 185 <= info["max_band_width"] <= 248, info
            pairs, _, cells = b.counts()
            med = statistics.median(times[k])
            out["%d %s" % (e, form)] = med * 1e3
            print("stage expansion %d, %s: %d reads, widest band %d, %d cells per lane, %d cells, %d assignments, "
                  "runs (ms) %s, median %.1f ms, spread %.1f ms, %.2f Gcells/s" % (
                      e, form, b.n, info["max_band_width"], info["cells_per_lane"], int(cells.sum()), int(pairs.sum()),
                      " ".join("%.1f" % (t * 1e3) for t in times[k]), med * 1e3,
                      (max(times[k]) - min(times[k])) * 1e3, int(cells.sum()) / med / 1e9), flush=True)
        if len(bs) == 2:
            print("stage expansion %d: ring / fused = %.3fx" % (e, statistics.median(times[0]) / statistics.median(times[1])),
                  flush=True)
        for b in bs:
            b.close()
    ctx.close()
    print("medians " + json.dumps(out), flush=True)


def ab(parent_lib, n):
    runs = {"parent": [], "branch alone": [], "branch": []}
    for _ in range(REPS):
        for side in ("parent", "branch alone", "branch"):  # in turn
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
    for side in ("parent", "branch alone", "branch"):
        for key in sorted(runs[side][0]):
            v = [r[key] for r in runs[side]]
            print("ab %s, expansion %s: process medians (ms) %s, median %.1f, spread %.1f" % (
                side, key, " ".join("%.1f" % x for x in v), statistics.median(v), max(v) - min(v)), flush=True)
    for e in EXPANSIONS:
        p = statistics.median(r["%d ring" % e] for r in runs["parent"])
        a = statistics.median(r["%d ring" % e] for r in runs["branch alone"])
        q = statistics.median(r["%d ring" % e] for r in runs["branch"])
        f = statistics.median(r["%d fused" % e] for r in runs["branch"])
        print("ab expansion %d: un-flagged batch alone, parent %.1f ms, branch %.1f ms (parent / branch %.3fx); beside the "
              "fused batch, ring %.1f ms, fused %.1f ms (ring / fused %.3fx)" % (e, p, a, p / a, q, f, q / f), flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "stage"
    if what == "ab":
        ab(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 1024)
    else:
        stage(int(sys.argv[2]) if len(sys.argv) > 2 else 1024, len(sys.argv) > 3 and sys.argv[3] == "ring")

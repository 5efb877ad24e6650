"""The wide builds of the workgroup-per-alignment kernels (CPECAN_FLAG_WIDE_BANDS: six and eight waves per workgroup)
against the general kernel on the same batch, for the table in DESIGN.md: strawMan reads of 2 000 k-mers x 4 000 events
whose anchors are sparse enough for a widest band of about 320 (six waves) and about 450 k-mers (eight), posterior
decode and E-step.  Runs of (a) no flag -- the general kernel, what such a batch ran on before the flag -- and (b) the
flag alternate on one device; the figure is the median of five wall times of run() + sync(), cells counted from the
band table (the batch's own per-read counts of in-band cells).
Run on the GPU box: python tests/tools/bench_wide_bands.py [reads [flag-only]] ; `widths` as the first argument prints
the widest bands only (no GPU); `flag-only` runs (b) alone, twice per batch (for a kernel trace)."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import synth  # noqa: E402
from harness import band_params, cp, make_items  # noqa: E402

# (label, anchor spacing, diagonalExpansion)
CONFIGS = [("six waves", 200, 120), ("eight waves", 250, 200)]
REPS = 5


def widest(batch, e):
    w = 0
    for it in batch["items"]:
        an = batch["anchors"][it["anchor_offset"]: it["anchor_offset"] + it["n_anchors"]]
        L, R = cp.band_construct(an, it["lX"], it["lY"], e)
        w = max(w, int(((R - L) // 2 + 1).max()))
    return w


def main():
    widths_only = len(sys.argv) > 1 and sys.argv[1] == "widths"
    n = int(sys.argv[2 if widths_only else 1]) if len(sys.argv) > (2 if widths_only else 1) else 1024
    flag_only = not widths_only and len(sys.argv) > 2 and sys.argv[2] == "flag-only"
    ctx = None if widths_only else cp.Context(0)
    for label, every, e in CONFIGS:
        batch = synth.make_batch(5, n, 2000, 4000, anchor_every=every)
        if widths_only:
            print("%s: %d reads, anchors every %d, expansion %d: widest band %d" % (label, n, every, e, widest(batch, e)),
                  flush=True)
            continue
        bp = band_params(0.01, 1000, 40, e)
        ctx.models_clear()
        ctx.models_create([(cp.NANOPORE_TRANSITIONS, m, gx, gy) for m, gx, gy in batch["models"]])
        items = make_items(batch, (1, 1))
        for mode, what in ((cp.MODE_POSTERIOR, "posterior"), (cp.MODE_EXPECTATIONS, "expectations")):
            bs = [cp.Batch(ctx, items, batch["x_chars"], batch["events"], batch["anchors"], bp, mode, cp.KERNEL_AUTO, f)
                  for f in ((cp.FLAG_WIDE_BANDS,) if flag_only else (0, cp.FLAG_WIDE_BANDS))]
            times = [[] for _ in bs]
            for b in bs:  # warm-up (and, for the posterior decode, the pair allocation settles)
                b.run(); b.sync()
            for _ in range(1 if flag_only else REPS):
                for k, b in enumerate(bs):  # (a), (b), (a), (b), ...
                    t0 = time.perf_counter(); b.run(); b.sync(); times[k].append(time.perf_counter() - t0)
            for k, b in enumerate(bs):
                info = b.info()
                cells = int(b.counts()[2].sum())
                med = statistics.median(times[k])
                print("%s %s %s: %d reads, widest band %d, %s kernel%s, %d cells, runs (ms) %s, median %.1f ms, "
                      "%.2f Gcells/s" % (label, what, "(b) flag" if k or flag_only else "(a) no flag", b.n, info["max_band_width"],
                                         info["kernel"], " (%d waves)" % info["waves_per_workgroup"]
                                         if "waves_per_workgroup" in info else "", cells,
                                         " ".join("%.1f" % (t * 1e3) for t in times[k]), med * 1e3, cells / med / 1e9),
                      flush=True)
            if not flag_only:
                print("%s %s: no flag / flag = %.2fx" % (label, what,
                                                         statistics.median(times[0]) / statistics.median(times[1])), flush=True)
            for b in bs:
                b.close()
    if ctx is not None:
        ctx.close()


if __name__ == "__main__":
    main()

"""The E-step builds of the vanilla machine on the workgroup-per-alignment kernels (CPECAN_FLAG_WIDE_BANDS_VANILLA_ESTEP
on a vanilla batch of expectations: four, six and eight waves per workgroup) against the general kernel on the same
batch, for the table in DESIGN.md: the batches bench_vanilla_wide.py draws for the posterior builds -- vanilla reads of
2 000 k-mers x 4 000 events, a scaled model per read, whose anchors are sparse enough for a widest band of about 230
(four waves), 320 (six) and 450 k-mers (eight) -- created with CPECAN_FLAG_EXPECTATIONS.  Runs of (a) no flag --
cpecan_k_generalv, what such a batch runs on without the flag -- and (b) the flag alternate in one process on one
device; the figure is the median of five wall times of run() + sync() after a warm-up, cells counted from the band
table (the batch's own per-read counts of in-band cells).
Run on the GPU box: python tests/tools/bench_vanilla_wide_estep.py [reads [flag-only]] ; `widths` as the first argument
prints the widest bands only (no GPU); `flag-only` runs (b) alone, twice per batch (for a kernel trace)."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import pyoracle as o  # noqa: E402  (model construction only)
import synth  # noqa: E402
from harness import band_params, cp, make_items  # noqa: E402
from bench_vanilla_wide import CONFIGS, REPS, widest  # noqa: E402  (the same batches)
from test_vanilla_gpu import skip_bins  # noqa: E402

ESTEP = cp.FLAG_WIDE_BANDS_VANILLA_ESTEP


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
        models = [o.VanillaModel(m, skip_bins(i % 8), gy, 0.17 if i % 2 == 0 else 0.14, 0.55 if i % 2 == 0 else 0.49)
                  for i, (m, _, gy) in enumerate(batch["models"])]
        ctx.models_clear()
        ctx.modelsv_create([(m.scalars, m.match, m.skip, m.gap_y) for m in models])
        del models
        items = make_items(batch, (1, 1))
        bs = [cp.Batch(ctx, items, batch["x_chars"], batch["events"], batch["anchors"], bp,
                       flags=cp.FLAG_EXPECTATIONS | f, vanilla=True) for f in ((ESTEP,) if flag_only else (0, ESTEP))]
        times = [[] for _ in bs]
        for b in bs:  # warm-up
            b.run(); b.sync()
        for _ in range(1 if flag_only else REPS):
            for k, b in enumerate(bs):  # (a), (b), (a), (b), ...
                t0 = time.perf_counter(); b.run(); b.sync(); times[k].append(time.perf_counter() - t0)
        for k, b in enumerate(bs):
            info = b.info()
            cells = int(b.counts()[2].sum())
            med = statistics.median(times[k])
            print("%s E-step %s: %d reads, widest band %d, %s kernel%s, %d cells, runs (ms) %s, median %.1f ms, "
                  "spread %.1f ms, %.2f Gcells/s" % (
                      label, "(b) flag" if k or flag_only else "(a) no flag", b.n, info["max_band_width"], info["kernel"],
                      " (%d waves)" % info["waves_per_workgroup"] if "waves_per_workgroup" in info else "", cells,
                      " ".join("%.1f" % (t * 1e3) for t in times[k]), med * 1e3,
                      (max(times[k]) - min(times[k])) * 1e3, cells / med / 1e9), flush=True)
        if not flag_only:
            print("%s E-step: no flag / flag = %.2fx" % (label, statistics.median(times[0]) / statistics.median(times[1])),
                  flush=True)
        for b in bs:
            b.close()
    if ctx is not None:
        ctx.close()


if __name__ == "__main__":
    main()

"""The 4-state machine on its one-wave-per-alignment kernels (CPECAN_FLAG_SM4_WAVE, cpecan_kernel_wave4.hip) against
the general kernel (cpecan_k_general4, what a batch without the flag runs on), for the record in DESIGN.md 5.

Shapes: 1024 and 4096 alignments of 2 000 k-mers x 4 000 events (one shared model: 4096 tables of 590 KB would time
the upload), anchors every 50 k-mers, at the driver's diagonalExpansion of 50 (bands of about 100 cells: two cells per
lane) and at 8 (at most 64 cells: one cell per lane).  A flagged and an un-flagged batch of the same reads live on one
context and run in turn, A B A B ..., after a warm-up run of each; the time is the device's, between the events the
library records around run ... sync (Batch.elapsed_ms).  Prints one line per shape: the median of each, Gcells/s and the
ratio.  Run on the GPU box: python tests/tools/bench_sm4_wave.py [alignments ...]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import pyoracle as o  # noqa: E402  (model construction only)
import synth  # noqa: E402
from harness import band_params, cp, make_items  # noqa: E402

REPEATS = 5
counts = [int(v) for v in sys.argv[1:]] or [1024, 4096]
ctx = cp.Context(0)
for n in counts:
    batch = synth.make_batch(5, n, 2000, 4000, anchor_every=50, distinct_models=False)
    models = [o.Sm4Model(m, gy) for (m, _, gy) in batch["models"]]
    ctx.models_clear()
    ctx.models4_create([(m.transitions, m.match, m.gap_x, m.gap_y) for m in models])
    for expansion in (50, 8):
        bp = band_params(0.01, 1000, 40, expansion)
        made = {}
        for what, flags in (("general", 0), ("wave", cp.FLAG_SM4_WAVE)):
            b = cp.Batch(ctx, make_items(batch, (1, 1)), batch["x_chars"], batch["events"], batch["anchors"], bp,
                         flags=flags, sm4=True)
            assert b.kernel_family()["wave"] == (1 if flags else 0), b.info()
            b.run()
            b.sync()
            made[what] = b
        ms = {what: [] for what in made}
        for _ in range(REPEATS):
            for what, b in made.items():
                b.run()
                b.sync()
                ms[what].append(b.elapsed_ms()[0])
        cells = int(made["wave"].counts()[2].sum())
        pairs = [int(b.counts()[0].sum()) for b in made.values()]
        assert pairs[0] == pairs[1] and cells == int(made["general"].counts()[2].sum())
        g, w = statistics.median(ms["general"]), statistics.median(ms["wave"])
        width = made["wave"].info()["max_band_width"]
        assert width <= (128 if expansion == 50 else 64), width
        print("sm4 %d alignments, expansion %d (widest band %d, %s): general %.1f ms (%.2f Gcells/s, %.1f..%.1f), "
              "wave %.1f ms (%.2f Gcells/s, %.1f..%.1f), general / wave %.2f" % (
                  n, expansion, width, "cpecan_k_wave4_l1" if width <= 64 else "cpecan_k_wave4_l2", g, cells / g / 1e6,
                  min(ms["general"]), max(ms["general"]), w, cells / w / 1e6, min(ms["wave"]), max(ms["wave"]), g / w),
              flush=True)
        for b in made.values():
            b.close()
ctx.close()

"""The HDP machine's E-step summed inside the workgroup kernels' sweep back (CPECAN_FLAG_WIDE_BANDS_HDP_FUSED_ESTEP: the
_hf6 / _hf8 builds) against the same kernels' path through the ring of backward cells and the expectation kernel
(CPECAN_FLAG_WIDE_BANDS_HDP_ESTEP alone: _he6 / _he8), for the table in DESIGN.md: bench_hdp_wide_estep.py's two batches
-- 1024 HDP reads of 2 000 k-mers on the reference's serialized HDP (tests/golden/testTemplate.nhdp), widest band 321 and
441, as CPECAN_FLAG_EXPECTATIONS batches with the assignment threshold 0.05; the batch holds 16 distinct reads, repeated
up to the read count.  Runs of (a) the wide-bands E-step flag alone and (b) the same batch with the fused flag alternate
in one process on one device; the figure is the median of five wall times of run() + sync() after a warm-up, plus the
spread of the five; cells counted from the band table.  The assignment counts of the two are printed and must agree.
Run on the GPU box: python tests/tools/bench_hdp_wide_fused_estep.py [reads [fused-only]] ; `fused-only` runs (b) alone,
twice per batch (for a kernel trace)."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import pyoracle as o  # noqa: E402  (the serialized HDP only)
from harness import band_params, cp, hdp_batch, make_items  # noqa: E402

# (label, anchor spacing, diagonalExpansion): bench_hdp_wide_estep.py's
CONFIGS = [("six waves", 60, 140), ("eight waves", 60, 260)]
REPS = 5
DISTINCT = 16
RING = cp.FLAG_WIDE_BANDS_HDP_ESTEP
FUSED = RING | cp.FLAG_WIDE_BANDS_HDP_FUSED_ESTEP


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    fused_only = len(sys.argv) > 2 and sys.argv[2] == "fused-only"
    nhdp = o.load_nhdp(os.path.join(ROOT, "tests", "golden", "testTemplate.nhdp"))
    ctx = cp.Context(0)
    for label, every, e in CONFIGS:
        batch, _ = hdp_batch(5, DISTINCT, 2000, every, nhdp)
        batch["items"] = [batch["items"][i % DISTINCT] for i in range(n)]
        bp = band_params(0.05, 1000, 40, e)
        ctx.models_clear()
        ctx.modelsh_create([(cp.NANOPORE_TRANSITIONS, nhdp["alphabet"], nhdp["grid"], nhdp["y"], nhdp["slope"],
                             nhdp["kmer_row"])])
        items = make_items(batch, (1, 1))
        bs = [cp.Batch(ctx, items, batch["x_chars"], batch["events"], batch["anchors"], bp,
                       flags=cp.FLAG_EXPECTATIONS | f, hdp=True) for f in ((FUSED,) if fused_only else (RING, FUSED))]
        times = [[] for _ in bs]
        for b in bs:  # warm-up (the allocation of the assignments settles)
            b.run(); b.sync()
        for _ in range(1 if fused_only else REPS):
            for k, b in enumerate(bs):  # (a), (b), (a), (b), ...
                t0 = time.perf_counter(); b.run(); b.sync(); times[k].append(time.perf_counter() - t0)
        pairs = []
        for k, b in enumerate(bs):
            info = b.info()
            counts = b.counts()
            cells = int(counts[2].sum())
            pairs.append(int(counts[0].sum()))
            med = statistics.median(times[k])
            print("%s E-step %s: %d reads, widest band %d, %s kernel (%d waves), fused_expectations %d, %d cells, "
                  "%d assignments, runs (ms) %s, median %.1f ms, spread %.1f ms, %.2f Gcells/s" % (
                      label, "(b) fused" if k or fused_only else "(a) ring", b.n, info["max_band_width"], info["kernel"],
                      info.get("waves_per_workgroup", 0), info["fused_expectations"], cells, pairs[-1],
                      " ".join("%.1f" % (t * 1e3) for t in times[k]), med * 1e3,
                      (max(times[k]) - min(times[k])) * 1e3, cells / med / 1e9), flush=True)
        if not fused_only:
            assert pairs[0] == pairs[1], pairs
            print("%s E-step: ring / fused = %.2fx" % (label, statistics.median(times[0]) / statistics.median(times[1])),
                  flush=True)
        for b in bs:
            b.close()
    ctx.close()


if __name__ == "__main__":
    main()

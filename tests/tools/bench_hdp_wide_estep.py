"""The E-step builds of the HDP machine on the workgroup-per-alignment kernels (CPECAN_FLAG_WIDE_BANDS_HDP_ESTEP on an HDP
batch of expectations: six and eight waves per workgroup) against the general kernel on the same batch, for the table in
DESIGN.md: bench_hdp_wide.py's two configurations -- HDP reads of 2 000 k-mers on the reference's serialized HDP
(tests/golden/testTemplate.nhdp) whose anchors are sparse enough for a widest band inside each class -- as
CPECAN_FLAG_EXPECTATIONS batches with the assignment threshold 0.05.  The batch holds 16 distinct reads, repeated up to
the read count.  Runs of (a) no flag -- cpecan_k_generalh, what such a batch runs on without the flag -- and (b) the
flag alternate in one process on one device; the figure is the median of five wall times of run() + sync() after a
warm-up, cells counted from the band table (the batch's own per-read counts of in-band cells).
Run on the GPU box: python tests/tools/bench_hdp_wide_estep.py [reads [flag-only]] ; `widths` as the first argument
prints the widest bands only (no GPU); `flag-only` runs (b) alone, twice per batch (for a kernel trace)."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import pyoracle as o  # noqa: E402  (the serialized HDP only)
from harness import band_params, cp, hdp_batch, make_items  # noqa: E402

# (label, anchor spacing, diagonalExpansion)
CONFIGS = [("six waves", 60, 140), ("eight waves", 60, 260)]
REPS = 5
DISTINCT = 16


def widest(batch, e):
    w = 0
    for it in batch["items"][:DISTINCT]:
        an = batch["anchors"][it["anchor_offset"]: it["anchor_offset"] + it["n_anchors"]]
        L, R = cp.band_construct(an, it["lX"], it["lY"], e)
        w = max(w, int(((R - L) // 2 + 1).max()))
    return w


def main():
    widths_only = len(sys.argv) > 1 and sys.argv[1] == "widths"
    n = int(sys.argv[2 if widths_only else 1]) if len(sys.argv) > (2 if widths_only else 1) else 1024
    flag_only = not widths_only and len(sys.argv) > 2 and sys.argv[2] == "flag-only"
    nhdp = o.load_nhdp(os.path.join(ROOT, "tests", "golden", "testTemplate.nhdp"))
    ctx = None if widths_only else cp.Context(0)
    for label, every, e in CONFIGS:
        batch, _ = hdp_batch(5, DISTINCT, 2000, every, nhdp)
        batch["items"] = [batch["items"][i % DISTINCT] for i in range(n)]
        if widths_only:
            print("%s: %d reads, anchors every %d, expansion %d: widest band %d" % (label, n, every, e, widest(batch, e)),
                  flush=True)
            continue
        bp = band_params(0.05, 1000, 40, e)
        ctx.models_clear()
        ctx.modelsh_create([(cp.NANOPORE_TRANSITIONS, nhdp["alphabet"], nhdp["grid"], nhdp["y"], nhdp["slope"],
                             nhdp["kmer_row"])])
        items = make_items(batch, (1, 1))
        bs = [cp.Batch(ctx, items, batch["x_chars"], batch["events"], batch["anchors"], bp,
                       flags=cp.FLAG_EXPECTATIONS | f, hdp=True)
              for f in ((cp.FLAG_WIDE_BANDS_HDP_ESTEP,) if flag_only else (0, cp.FLAG_WIDE_BANDS_HDP_ESTEP))]
        times = [[] for _ in bs]
        for b in bs:  # warm-up (the allocation of the assignments settles)
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

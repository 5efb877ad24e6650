"""The strawMan E-step on the six- and eight-wave workgroup kernels with its expectations summed inside the sweep back
(CPECAN_FLAG_WIDE_BANDS_FUSED_ESTEP / CPECAN_EXPECT_FUSED_WIDE=1: the fused builds f6 and f8) against the same kernels'
path through the ring of backward cells and the expectation kernel (r6, r8) -- what the parent commit runs -- for the
paragraph in DESIGN.md.  One measurement, after tests/tools/bench_workgroup_fused_estep.py's `stage`:
  stage   one workgroup batch alone at six and at eight waves per workgroup (1024 reads of 2000 k-mers x 4000 events, 16
          distinct ones repeated, anchors every 50 k-mers; the batch's default two stream groups), ring and fused
          alternating, medians of three: wall time of run() + sync(), cpecan_hip_batch_stage_ms and Gcells/s;
  once    one such batch of one form at both widths, run four times: what a kernel trace is taken of
          (`rocprofv3 --kernel-trace --stats -- python tests/tools/bench_wide_fused_estep.py once ring|fused`, each form
          in a run of its own).
Run on the GPU box: python tests/tools/bench_wide_fused_estep.py stage [reads] | once ring|fused [reads]."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]

REPS = 3
DISTINCT = 16
# waves per workgroup -> diagonal expansion (anchors every 50 k-mers, two events per k-mer: the widest band of these
# reads is 54 + expansion k-mers)
EXPANSION = {6: 250, 8: 400}


def shape(rows, n):
    import synth
    from harness import band_params, make_items
    batch = synth.make_batch(40 + rows, DISTINCT, 2000, 4000, anchor_every=50)
    batch["items"] = [batch["items"][i % DISTINCT] for i in range(n)]
    return batch, make_items(batch, (1, 1)), band_params(0.01, 1000, 40, EXPANSION[rows])


def create(cp, ctx, batch, items, bp, rows, fused):
    """one batch alive at a time: the streams of two share the process's few hardware queues"""
    b = cp.Batch(ctx, items, batch["x_chars"], batch["events"], batch["anchors"], bp, cp.MODE_EXPECTATIONS,
                 cp.KERNEL_AUTO, cp.FLAG_WORKGROUP_KERNELS | cp.FLAG_WIDE_BANDS |
                 (cp.FLAG_WIDE_BANDS_FUSED_ESTEP if fused else 0))
    info = b.info()
    assert info["family"] == "workgroup" and info["waves_per_workgroup"] == rows, info
    assert info["fused_expectations"] == int(fused), info
    return b, info


def stage(n):
    from harness import cp
    ctx = cp.Context(0)
    for rows in (6, 8):
        batch, items, bp = shape(rows, n)
        ctx.models_clear()
        ctx.models_create([(cp.NANOPORE_TRANSITIONS, m, gx, gy) for (m, gx, gy) in batch["models"]])
        times, stages, last = [[], []], [[], []], [None, None]
        for _ in range(REPS):
            for k in (0, 1):  # ring, fused, ring, fused, ...
                b, info = create(cp, ctx, batch, items, bp, rows, k == 1)
                b.run(); b.sync()
                three = []
                for _ in range(3):
                    t0 = time.perf_counter(); b.run(); b.sync(); three.append(time.perf_counter() - t0)
                times[k].append(statistics.median(three))
                stages[k].append(b.stage_ms())
                last[k] = (info, int(b.counts()[2].sum()), b.n)
                b.close()
        for k in (0, 1):
            info, cells, reads = last[k]
            med = statistics.median(times[k])
            print("stage %d waves, %s: %d reads, widest band %d, %d cells, batches (ms, each the median of three runs) %s, "
                  "median %.1f ms, %.2f Gcells/s; stage_ms summed over the two stream groups (forward, backward and "
                  "after, launches) %s" % (
                      rows, "fused" if k else "ring", reads, info["max_band_width"], cells,
                      " ".join("%.1f" % (t * 1e3) for t in times[k]), med * 1e3, cells / med / 1e9,
                      " ".join("(%.1f, %.1f, %d)" % s for s in stages[k])), flush=True)
        print("stage %d waves: ring / fused = %.3fx" % (rows, statistics.median(times[0]) / statistics.median(times[1])),
              flush=True)
    ctx.close()


def once(form, n):
    from harness import cp
    ctx = cp.Context(0)
    for rows in (6, 8):
        batch, items, bp = shape(rows, n)
        ctx.models_clear()
        ctx.models_create([(cp.NANOPORE_TRANSITIONS, m, gx, gy) for (m, gx, gy) in batch["models"]])
        b, info = create(cp, ctx, batch, items, bp, rows, form == "fused")
        for _ in range(4):
            b.run(); b.sync()
        print("once %d waves, %s: %s" % (rows, form, info), flush=True)
        b.close()
    ctx.close()


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "stage"
    if what == "stage":
        stage(int(sys.argv[2]) if len(sys.argv) > 2 else 1024)
    elif what == "once" and len(sys.argv) > 2 and sys.argv[2] in ("ring", "fused"):
        once(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 1024)
    else:
        sys.exit(__doc__)

"""The strawMan E-step on the workgroup-per-alignment kernels with its expectations summed inside the sweep back
(CPECAN_FLAG_WORKGROUP_FUSED_ESTEP / CPECAN_EXPECT_FUSED_WORKGROUP=1: the fused builds of one to four waves) against the
same kernels' path through the ring of backward cells and the expectation kernel -- what the parent commit runs -- for the
paragraph in DESIGN.md.  Two measurements on one device, variable off and on alternating, medians of three:
  em      `bench.py --gpus 1 --mode em` with its defaults (BASELINE configs[3], four contexts) and with --em-contexts 2,
          each run a process of its own, the variable set in its environment or not; the figure is bench.py's ms_per_step;
  stage   one workgroup batch alone at each number of waves per workgroup (1024 reads of 2000 k-mers x 4000 events, 16
          distinct ones repeated; the batch's default two stream groups): wall time of run() + sync() and
          cpecan_hip_batch_stage_ms;
(The kernel traces beside them are `rocprofv3 --kernel-trace --stats -- python bench.py --gpus 1 --mode em --steps 4
--warmup 1`, once with the variable and once without.)
Run on the GPU box: python tests/tools/bench_workgroup_fused_estep.py em|stage [reads]."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]

VAR = "CPECAN_EXPECT_FUSED_WORKGROUP"
REPS = 3
# stage: waves per workgroup -> diagonal expansion (anchors every 50 k-mers, two events per k-mer: the widest band of
# these reads is 54 + expansion k-mers)
EXPANSION = {1: 2, 2: 40, 3: 100, 4: 150}


def bench_line(extra, fused):
    env = dict(os.environ)
    env.pop(VAR, None)
    if fused:
        env[VAR] = "1"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--mode", "em"] + extra,
                         env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    if out.returncode != 0 or not lines:
        raise RuntimeError("bench.py failed (%d): %s" % (out.returncode, out.stderr[-2000:]))
    return json.loads(lines[-1])


def em():
    for label, extra in (("four contexts (defaults)", []), ("two contexts", ["--em-contexts", "2"])):
        ms = {False: [], True: []}
        for _ in range(REPS):
            for fused in (False, True):  # ring, fused, ring, fused, ...
                d = bench_line(extra, fused)
                k = d["config"]["kernel"]
                assert k["family"] == "workgroup" and k["fused_expectations"] == int(fused), k
                ms[fused].append(d["ms_per_step"])
                print("em %s, %s: %s" % (label, "fused" if fused else "ring", json.dumps(d)), flush=True)
        for fused in (False, True):
            print("em %s, %s: ms per iteration %s, median %.1f" % (
                label, "fused" if fused else "ring", " ".join("%.1f" % v for v in ms[fused]),
                statistics.median(ms[fused])), flush=True)
        print("em %s: ring / fused = %.3fx" % (label, statistics.median(ms[False]) / statistics.median(ms[True])),
              flush=True)


def stage(n):
    import synth
    from harness import band_params, cp, make_items
    ctx = cp.Context(0)
    distinct = 16
    for rows in (1, 2, 3, 4):
        batch = synth.make_batch(40 + rows, distinct, 2000, 4000, anchor_every=50)
        batch["items"] = [batch["items"][i % distinct] for i in range(n)]
        bp = band_params(0.01, 1000, 40, EXPANSION[rows])
        ctx.models_clear()
        ctx.models_create([(cp.NANOPORE_TRANSITIONS, m, gx, gy) for (m, gx, gy) in batch["models"]])
        items = make_items(batch, (1, 1))
        times, stages, last = [[], []], [[], []], [None, None]
        for _ in range(REPS):
            for k, f in enumerate((0, cp.FLAG_WORKGROUP_FUSED_ESTEP)):  # ring, fused, ring, fused, ...
                # one batch alive at a time: the streams of two share the process's few hardware queues, and the batch
                # whose two stream groups land on one queue runs them one after the other
                b = cp.Batch(ctx, items, batch["x_chars"], batch["events"], batch["anchors"], bp, cp.MODE_EXPECTATIONS,
                             cp.KERNEL_AUTO, cp.FLAG_WORKGROUP_KERNELS | f)
                b.run(); b.sync()
                three = []
                for _ in range(3):
                    t0 = time.perf_counter(); b.run(); b.sync(); three.append(time.perf_counter() - t0)
                times[k].append(statistics.median(three))
                stages[k].append(b.stage_ms())
                info = b.info()
                assert info["family"] == "workgroup" and info["waves_per_workgroup"] == rows, info
                assert info["fused_expectations"] == k, info
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


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "em"
    reads = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    {"em": em, "stage": lambda: stage(reads)}[what]()

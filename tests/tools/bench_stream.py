"""One workload two ways in one process, alternating, for the record in DESIGN.md section 5 (profiles/r30_stream_ab.txt):
  (a) what callers had: getAlignedPairsUsingAnchorsBatch per chunk of R reads, one chunk after the other;
  (b) the stream (cpecan_stream_*) with maxReadsPerChunk = R, with and without its grouping by kernel.
Synthetic strawMan reads of tests/synth.py, --chunks x --reads of --events events against --kmers k-mers at expansion
--expansion (default 8 x 256 of 10000 x 5000 at 100), taken from --distinct distinct reads in turn; one machine over the
unscaled model.  Two workloads: every read with its own anchors ("uniform"), and one read in --reads with an anchor jump
that takes its band past 248 k-mers ("outlier").  After one warm-up pass of every way, --repeats passes of each,
alternating; ms per chunk as min / median / max, and beside each pass the shader clock of a small probe batch of the same
shape run right after it (cpecan_hip_batch_shader_clock_mhz reads a batch's own run; the host library's batches are not
the caller's to ask; a reading outside 500-3000 MHz, which the probe's counters gave once, is no clock and is printed as ?).
Run on the GPU box: python tests/tools/bench_stream.py [--chunks N] [--reads R] ..."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import host_api as h  # noqa: E402
import stream_api as sa  # noqa: E402
import synth  # noqa: E402
from harness import band_params, cp, make_items  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=8)
    ap.add_argument("--reads", type=int, default=256)
    ap.add_argument("--events", type=int, default=10000)
    ap.add_argument("--kmers", type=int, default=5000)
    ap.add_argument("--expansion", type=int, default=100)
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--jump", type=int, default=260)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--workloads", default="uniform,outlier", help="which of the two to run")
    a = ap.parse_args()
    import torch
    print("box: %s, %s" % (os.uname().nodename, torch.cuda.get_device_name(0)), flush=True)
    L = sa.lib()
    R, n = a.reads, a.chunks * a.reads
    sm, get_x = sa.machine("strawman")
    p = sa.params(expansion=a.expansion, min_diags=1000)
    lengths = [(a.kmers, a.events)] * a.distinct
    plain = sa.synthetic_reads(30, lengths, get_x, anchor_every=50)
    wide = sa.synthetic_reads(30, lengths[:1], get_x, anchor_every=50, jumps=[a.jump])[0]
    widths = [cp.band_extent(rd.anchors, rd.lX, rd.lY, a.expansion)[0] for rd in plain]
    print("%d chunks x %d reads of %d events x %d k-mers, expansion %d: bands of %d..%d k-mers; the outlier read: %d" % (
        a.chunks, R, a.events, a.kmers, a.expansion, min(widths), max(widths),
        cp.band_extent(wide.anchors, wide.lX, wide.lY, a.expansion)[0]), flush=True)
    workloads = {"uniform": [plain[i % a.distinct] for i in range(n)],
                 "outlier": [wide if i % R == R // 2 else plain[i % a.distinct] for i in range(n)]}

    # the probe: a small batch of the same shape through the C-ABI, whose forward sweeps tell the shader clock
    ctx = cp.Context(0)
    pb = synth.make_batch(30, 16, a.kmers, a.events, anchor_every=50, distinct_models=False)
    ctx.models_create([(cp.NANOPORE_TRANSITIONS,) + tuple(pb["models"][0])])
    probe = cp.Batch(ctx, make_items(pb, (1, 1)), pb["x_chars"], pb["events"], pb["anchors"],
                     band_params(0.01, 1000, 40, a.expansion), cp.MODE_POSTERIOR, cp.KERNEL_AUTO, 0)

    def clock():
        probe.run()
        probe.sync()
        return probe.shader_clock_mhz()

    vp = C.c_void_p

    def batch_calls(reads):
        t0 = time.perf_counter()
        for c in range(a.chunks):
            part = reads[c * R:(c + 1) * R]
            sms = (vp * R)(*[sm] * R)
            sxs = (vp * R)(*[rd.sX for rd in part])
            sys_ = (vp * R)(*[rd.sY for rd in part])
            ans = (vp * R)(*[rd.lst for rd in part])
            out = L.getAlignedPairsUsingAnchorsBatch(R, sms, sxs, sys_, ans, p, True, True)
            for i in range(R):
                L.stList_destruct(out[i])
        return (time.perf_counter() - t0) * 1e3 / a.chunks, None

    def stream_of(one_class):
        def run(reads):
            chunks, count = [], [0]

            def on_result(_arg, _tag, lst):
                count[0] += 1
                if lst:
                    L.stList_destruct(lst)

            def on_chunk(_arg, c):
                chunks.append((c.contents.nReads, c.contents.kernel, c.contents.rows))

            cb_r, cb_c = sa.RESULT_FN(on_result), sa.CHUNK_FN(on_chunk)
            o = sa.StreamOptions(maxReadsPerChunk=R, oneClass=one_class)
            t0 = time.perf_counter()
            s = L.cpecan_stream_open(p, True, True, C.byref(o), cb_r, cb_c, None)
            for i, rd in enumerate(reads):
                L.cpecan_stream_submit(s, i, sm, rd.sX, rd.sY, rd.lst)
            refused = C.c_int64(0)
            L.cpecan_stream_close(s, None, C.byref(refused), None)
            ms = (time.perf_counter() - t0) * 1e3 / a.chunks
            assert count[0] == len(reads) and refused.value == 0
            return ms, chunks
        return run

    ways = [("(a) batch call per chunk", batch_calls), ("(b) stream, grouped", stream_of(0)),
            ("(b) stream, oneClass", stream_of(1))]
    for name, reads in workloads.items():
        if name not in a.workloads.split(","):
            continue
        use = ways if name == "outlier" else ways[:2]
        times = {w: [] for w, _ in use}
        shape = {}
        for rep in range(a.repeats + 1):  # the first pass warms up (code objects, pinned memory, the allocator's cache)
            for w, run in use:
                ms, chunks = run(reads)
                mhz = clock()
                if rep:
                    times[w].append((ms, mhz))
                    shape[w] = chunks
        print("%s workload: ms per chunk of %d reads (%d chunks' worth of reads per pass), %d passes" % (name, R, a.chunks, a.repeats))
        for w, _ in use:
            ms = [t for t, _ in times[w]]
            print("  %-26s min %9.2f  median %9.2f  max %9.2f   probe clock MHz %s" % (
                w, min(ms), float(np.median(ms)), max(ms), " ".join("%.0f" % m if 500 <= m <= 3000 else "?" for _, m in times[w])))
            if shape[w]:
                kinds = {}
                for nr, k, rows in shape[w]:
                    key = "general" if k == sa.KERNEL_GENERAL else "%d cells per lane" % rows
                    kinds[key] = (kinds.get(key, (0, 0))[0] + 1, kinds.get(key, (0, 0))[1] + nr)
                print("      chunks: " + ", ".join("%d on %s (%d reads)" % (c, k, r) for k, (c, r) in sorted(kinds.items())))
        med = {w: float(np.median([t for t, _ in times[w]])) for w, _ in use}
        spread = max(t for t, _ in times[ways[0][0]]) - min(t for t, _ in times[ways[0][0]])
        print("  stream / batch calls: %.3f (spread of (a)'s own passes: %.2f ms)" % (med[ways[1][0]] / med[ways[0][0]], spread))
        if name == "outlier":
            print("  oneClass / grouped: %.2f" % (med[ways[2][0]] / med[ways[1][0]]))
    probe.close()
    ctx.close()


if __name__ == "__main__":
    main()

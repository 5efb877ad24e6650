"""The streamed E-step measured three ways in one process, for the record in DESIGN.md section 5 (profiles/r31_stream_estep_*.txt):
  (1) --reads C3-shaped reads (--events events x --kmers k-mers, expansion --expansion), every read with a machine of its
      own scaled for it, strawMan and vanilla: getExpectationsUsingAnchorsBatch on all of them against the expectation
      stream (cpecan_stream_open_expectations) in chunks of --chunkReads, alternating, medians of --repeats passes after
      one warm-up pass of each;
  (2) the readback of one such batch through the C-ABI: one cpecan_hip_batch_sum_expectations against the loop of
      cpecan_hip_batch_fetch_expectations over its models with the host's adds (what add_sums does per model), at
      several model counts.  Both are timed around ctypes calls into preallocated buffers: a call costs the loop about a
      microsecond per model beside its blocking copy.  With --timing one more streamed pass runs under CPECAN_TIMING=1,
      whose per-chunk lines on stderr carry the consumer's own readback ("expectations ... ms");
  (3) a mixed-width set like test_stream_gpu.CLASS_JUMPS scaled to --reads reads (no jump, a jump that needs three cells
      per lane, a jump past 248 k-mers, in turn), one strawMan machine: grouped by kernel against oneClass = 1.
Reads are taken from --distinct distinct ones in turn.
Run on the GPU box: python tests/tools/bench_stream_estep.py [--reads N] [--chunkReads R] ..."""
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
import stream_estep_api as se  # noqa: E402
import synth  # noqa: E402
from harness import band_params, cp, make_items  # noqa: E402

HMM_TYPE = {"strawman": 2, "vanilla": 4}  # StateMachineType threeState, vanilla


def scaled_machines(kind, scalings):
    """one machine per read over the synthetic pore model, scaled for that read as vanillaAlign's build_state_machine does"""
    L = sa.lib()
    out = []
    for sc in scalings:
        sm, get_x = sa.machine(kind)
        L.emissions_signal_scaleModel(sm, *[float(v) for v in sc])
        out.append(sm)
    return out, get_x


def raw_reads(config_id, n, kmers, events, get_x, jumps=None):
    """reads of synth.make_read with their events as drawn (for machines scaled per read), and their scalings"""
    match = synth.synthetic_pore_model()[0]
    reads, scalings = [], []
    for r in range(n):
        rd = synth.make_read(np.random.default_rng(synth.SEED0 + config_id * 1000 + r), match, kmers, events, 50)
        reads.append(sa.SeqRead(rd["seq"], rd["events"], get_x, sa.with_jump(rd["anchors"], jumps[r] if jumps else 0)))
        scalings.append(rd["scale_params"])
    return reads, scalings


def median_ms(ts):
    return float(np.median(ts)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1024)
    ap.add_argument("--chunkReads", type=int, default=256)
    ap.add_argument("--events", type=int, default=10000)
    ap.add_argument("--kmers", type=int, default=5000)
    ap.add_argument("--expansion", type=int, default=100)
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--models", default="1,8,64,256,1024", help="model counts of part (2)")
    ap.add_argument("--parts", default="1,2,3")
    ap.add_argument("--timing", action="store_true")
    a = ap.parse_args()
    import torch
    print("box: %s, %s" % (os.uname().nodename, torch.cuda.get_device_name(0)), flush=True)
    L = se.lib()
    vp = C.c_void_p
    L.getExpectationsUsingAnchorsBatch.argtypes = [C.c_int64, C.POINTER(vp), vp, C.POINTER(vp), C.POINTER(vp),
                                                   C.POINTER(vp), C.POINTER(h.Params), C.c_bool, C.c_bool]
    n = a.reads
    p = sa.params(expansion=a.expansion, min_diags=1000)

    def streamed(kind, sms, reads, **options):
        target = se.Target(kind)
        t0 = time.perf_counter()
        out = se.run_stream(sms, reads, p, target, **options)
        dt = time.perf_counter() - t0
        assert out["n_refused"] == 0 and len(out["done"]) == len(reads)
        return dt, target.vector(), out["chunks"]

    if "1" in a.parts.split(","):
        for kind in ("strawman", "vanilla"):
            get_x = "sequence_getKmer" if kind == "strawman" else "sequence_getKmer2"
            distinct, scalings = raw_reads(31, a.distinct, a.kmers, a.events, get_x)
            sms, _ = scaled_machines(kind, [scalings[i % a.distinct] for i in range(n)])
            reads = [distinct[i % a.distinct] for i in range(n)]
            arr = lambda xs: (vp * n)(*xs)
            c_sms, c_sx, c_sy, c_an = arr(sms), arr([r.sX for r in reads]), arr([r.sY for r in reads]), arr([r.lst for r in reads])

            def batch_call():
                hmm = L.hmmContinuous_getEmptyHmm(HMM_TYPE[kind], 0.0, 0.01)
                t0 = time.perf_counter()
                L.getExpectationsUsingAnchorsBatch(n, c_sms, hmm, c_sx, c_sy, c_an, p, True, True)
                dt = time.perf_counter() - t0
                lik = C.cast(hmm, C.POINTER(C.c_double))[0]
                L.hmmContinuous_destruct(hmm, HMM_TYPE[kind])
                return dt, lik

            times = {"batch": [], "stream": []}
            for rep in range(a.repeats + 1):
                dt, lik = batch_call()
                ds, vec, chunks = streamed(kind, sms, reads, maxReadsPerChunk=a.chunkReads)
                assert np.isclose(vec[-1], lik, rtol=1e-9), (vec[-1], lik)
                if rep:
                    times["batch"].append(dt)
                    times["stream"].append(ds)
            print("(1) %s, %d reads of %d x %d, a model per read: getExpectationsUsingAnchorsBatch %.1f ms (%.1f..%.1f), "
                  "stream in %d chunks of <= %d %.1f ms (%.1f..%.1f), stream / batch %.3f" % (
                      kind, n, a.events, a.kmers, median_ms(times["batch"]), min(times["batch"]) * 1e3,
                      max(times["batch"]) * 1e3, len(chunks), a.chunkReads, median_ms(times["stream"]),
                      min(times["stream"]) * 1e3, max(times["stream"]) * 1e3,
                      median_ms(times["stream"]) / median_ms(times["batch"])), flush=True)
            if a.timing:
                os.environ["CPECAN_TIMING"] = "1"
                streamed(kind, sms, reads, maxReadsPerChunk=a.chunkReads)
                del os.environ["CPECAN_TIMING"]
            for sm in sms:
                L.stateMachine_destruct(sm)

    if "2" in a.parts.split(","):
        ctx = cp.Context(0)
        raw = cp.lib()
        for kind in ("strawman", "vanilla"):
            for m in [int(v) for v in a.models.split(",")]:
                data = synth.make_batch(32, m, 200, 400, anchor_every=40)
                match, gap_x, gap_y = data["base_model"]
                ctx.models_clear()
                if kind == "strawman":
                    ctx.models_create_scaled((cp.NANOPORE_TRANSITIONS, match, gap_x, gap_y), data["scalings"])
                    b = cp.Batch(ctx, make_items(data, (1, 1)), data["x_chars"], data["events"], data["anchors"],
                                 band_params(0.01, 120, 40, 20), cp.MODE_EXPECTATIONS, cp.KERNEL_AUTO, cp.FLAG_SMALL_FOOTPRINT)
                else:
                    import pyoracle as o
                    base = o.VanillaModel(match, np.linspace(0.4, 0.05, 30), gap_y)
                    ctx.modelsv_create_scaled((base.scalars, base.match, base.skip, base.gap_y), data["scalings"])
                    b = cp.Batch(ctx, make_items(data, (1, 1)), data["x_chars"], data["events"], data["anchors"],
                                 band_params(0.01, 120, 40, 20), flags=cp.FLAG_EXPECTATIONS, vanilla=True)
                b.run()
                b.sync()
                length = b.expectation_len()
                out, e, acc = np.zeros(length), np.zeros(length), np.zeros(length)
                po, pe = out.ctypes.data, e.ctypes.data
                t_sum, t_loop = [], []
                for rep in range(a.repeats + 2):
                    t0 = time.perf_counter()
                    raw.cpecan_hip_batch_sum_expectations(b.h, po)
                    t1 = time.perf_counter()
                    acc[:] = 0.0
                    for k in range(m):
                        raw.cpecan_hip_batch_fetch_expectations(b.h, k, pe)
                        acc += e
                    t2 = time.perf_counter()
                    if rep > 1:
                        t_sum.append(t1 - t0)
                        t_loop.append(t2 - t1)
                assert np.allclose(out, acc, rtol=1e-12, atol=0)
                print("(2) %s, %4d models x %d doubles: device sum %.3f ms, fetch loop with host adds %.3f ms, loop / sum %.1f" % (
                    kind, m, length, median_ms(t_sum), median_ms(t_loop), median_ms(t_loop) / median_ms(t_sum)), flush=True)
                b.close()
        ctx.close()

    if "3" in a.parts.split(","):
        sm, get_x = sa.machine("strawman")
        jumps = [0, 90, 260] * ((a.distinct + 2) // 3)
        distinct = sa.synthetic_reads(33, [(a.kmers, a.events)] * a.distinct, get_x, anchor_every=50, jumps=jumps[:a.distinct])
        reads = [distinct[i % a.distinct] for i in range(n)]
        widths = [cp.band_extent(rd.anchors, rd.lX, rd.lY, a.expansion)[0] for rd in distinct]
        print("(3) bands of the mixed set: %s" % sorted(set(widths)))
        times = {0: [], 1: []}
        shape = {}
        for rep in range(a.repeats + 1):
            for one in (0, 1):
                dt, _, chunks = streamed("strawman", sm, reads, maxReadsPerChunk=a.chunkReads, oneClass=one)
                if rep:
                    times[one].append(dt)
                    shape[one] = sorted({(c["kernel"], c["wave"], c["rows"]) for c in chunks})
        print("(3) mixed widths, %d reads, one machine: grouped %.1f ms on %s, oneClass %.1f ms on %s, oneClass / grouped %.2f" % (
            n, median_ms(times[0]), shape[0], median_ms(times[1]), shape[1], median_ms(times[1]) / median_ms(times[0])), flush=True)


if __name__ == "__main__":
    main()

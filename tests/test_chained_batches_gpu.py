"""Chained batches against the oracle: the schedules bench.py times (two batches ping-ponged with
cpecan_hip_batch_run_after, the assembly sweeps on their three-window ring with the post kernel on its own stream, or
on the small-footprint ring) and runs in --mode service (three contexts, the models of one rebuilt while the other two
are queued), follows between the kernel families, and what a follower's ordering promises (include/cpecan_hip.h).
Then the assembly sweeps' decode fallbacks and degenerate items.

Reads shaped for the assembly sweeps: about 1 200 k-mers x 2 400 events (lengths spread by length_sigma 0.2, so that
reads end in different windows), anchors every 50, diagonalExpansion 100 (bands of 121-158 k-mers), a traceback every
300 diagonals, 40 back: 8 and more windows, so the forward sweep's waits on windows w - 2 and w - 3 and both halves of
the scratch are used.  Every result is bit-identical to the oracle's (cells, totals, exponents, pairs)."""
import numpy as np
import pytest

import pyoracle as o
import synth
from harness import (assert_same_pairs, assert_same_posterior, band_params, batch_results, cp, make_items, run_gpu,
                     run_oracle_item)

pytestmark = pytest.mark.gpu

N = 8
ASM_BP = band_params(0.01, 300, 40, 100)
WAVE2_BP = band_params(0.01, 300, 40, 20)
RAGGED = (1, 1)

_DATA = {}
_ORACLE = {}


def data(seed):
    """a batch of N reads and the same batch with its per-read tables scaled by the oracle's scaleModel (the device
    scales them itself: cpecan_hip_models_create_scaled)"""
    if seed not in _DATA:
        bt = synth.make_batch(seed, N, 1200, 2400, anchor_every=50, length_sigma=0.2)
        match, gx, gy = bt["base_model"]
        base = o.Sm3Model(match, gy, gx)
        bt["models"] = [(base.scaled(*[float(v) for v in sc]).match, gx, gy) for sc in bt["scalings"]]
        _DATA[seed] = bt
    return _DATA[seed]


def oracle(seed, i, bp):
    key = (seed, i, bp.threshold, bp.minDiagsBetweenTraceBack, bp.traceBackDiagonals, bp.diagonalExpansion)
    if key not in _ORACLE:
        _ORACLE[key] = run_oracle_item(data(seed), i, bp, RAGGED)
    return _ORACLE[key]


def new_batch(cx, seed, bp, flags=0, model_base=0, clear=True):
    bt = data(seed)
    if clear:
        cx.models_clear()
    cx.models_create_scaled((cp.NANOPORE_TRANSITIONS,) + bt["base_model"], bt["scalings"])
    items = make_items(bt, RAGGED)
    items["model_id"] += model_base
    b = cp.Batch(cx, items, bt["x_chars"], bt["events"], bt["anchors"], bp, cp.MODE_POSTERIOR, cp.KERNEL_AUTO, flags)
    b.seed, b.bp = seed, bp
    return b


def assert_assembly(b):
    info = b.info()
    assert info["assembly_sweeps"] == 2 and 121 <= info["max_band_width"] <= 158, info


def check(b):
    """the batch's results through its own readback, against the oracle"""
    for i, g in enumerate(batch_results(b)):
        assert_same_posterior(g, oracle(b.seed, i, b.bp), (b.seed, i))


def test_reads_span_many_windows():
    """the shape: at least 8 traceback windows per read, reads of different lengths"""
    bt = data(201)
    lens = [it["lX"] + it["lY"] for it in bt["items"]]
    assert min(lens) > 8 * (300 - 41) and len(set(lens)) == N


@pytest.mark.parametrize("flags", [0, cp.FLAG_SMALL_FOOTPRINT], ids=["three-window-ring", "small-footprint"])
def test_bench_schedule(flags):
    """bench.py run_steps: six steps over two contexts, step s on batch s % 2 after step s - 1's batch, a batch waited
    for only when it is needed again -- and compared with the oracle after every wait"""
    ctxs = [cp.Context(0) for _ in range(2)]
    bs = [new_batch(cx, 201 + k, ASM_BP, flags) for k, cx in enumerate(ctxs)]
    for b in bs:
        assert_assembly(b)
    pending = [False, False]
    for s in range(6):
        j = s % 2
        if pending[j]:
            bs[j].sync()
            check(bs[j])
        bs[j].run(after=bs[(s - 1) % 2] if s > 0 else None)
        pending[j] = True
    for k in range(2):  # the oldest first
        bs[k].sync()
        check(bs[k])
    for cx in ctxs:
        cx.close()


def test_service_schedule():
    """bench.py --mode service: three contexts; batch k is made on context k % 3 (models cleared and rebuilt) while the
    batches of the other two are queued, run after batch k - 1, and waited for when its slot is needed again"""
    ctxs = [cp.Context(0) for _ in range(3)]
    slot = [None] * 3
    n = 5
    for k in range(n):
        if slot[k % 3] is not None:
            slot[k % 3].sync()
            check(slot[k % 3])
            slot[k % 3].close()
        slot[k % 3] = b = new_batch(ctxs[k % 3], 210 + k, ASM_BP, cp.FLAG_SMALL_FOOTPRINT)
        assert_assembly(b)
        b.run(after=slot[(k - 1) % 3] if k > 0 else None)
    for k in range(n - 3, n):
        slot[k % 3].sync()
        check(slot[k % 3])
    for cx in ctxs:
        cx.close()


FOLLOWS = {
    "assembly-after-compiled": ((201, WAVE2_BP, 0), (202, ASM_BP, 0)),
    "assembly-after-workgroup": ((201, ASM_BP, cp.FLAG_WORKGROUP_KERNELS), (202, ASM_BP, 0)),
    "compiled-after-assembly": ((201, ASM_BP, 0), (202, WAVE2_BP, 0)),
}


@pytest.mark.parametrize("name", list(FOLLOWS) + ["one-context"])
def test_mixed_follows(name):
    if name == "one-context":
        cx = cp.Context(0)
        ctxs = [cx]
        a = new_batch(cx, 201, ASM_BP)
        b = new_batch(cx, 202, ASM_BP, model_base=N, clear=False)
        assert_assembly(b)
    else:
        ctxs = [cp.Context(0), cp.Context(0)]
        (sa, bpa, fa), (sb, bpb, fb) = FOLLOWS[name]
        a = new_batch(ctxs[0], sa, bpa, fa)
        b = new_batch(ctxs[1], sb, bpb, fb)
    assert_assembly(a if name == "compiled-after-assembly" else b)
    a.run()
    b.run(after=a)
    b.sync()
    a.sync()
    check(a)
    check(b)
    for cx in ctxs:
        cx.close()


def test_cycle_without_host_sync():
    """A; B after A; A after B; B after A -- one wait at the end"""
    ctxs = [cp.Context(0), cp.Context(0)]
    a = new_batch(ctxs[0], 201, ASM_BP)
    b = new_batch(ctxs[1], 202, ASM_BP)
    a.run()
    b.run(after=a)
    a.run(after=b)
    b.run(after=a)
    b.sync()
    a.sync()
    check(a)
    check(b)
    for cx in ctxs:
        cx.close()


def test_earlier_batches_read_through_their_own_readback():
    """the contract of cpecan_hip_batch_run_after: a follower may start before what it follows has finished (after
    that batch's last forward sweep); only the last follower is waited for, and every earlier batch's counts, pairs
    and totals are read through that batch's own readback"""
    ctxs = [cp.Context(0) for _ in range(3)]
    bs = [new_batch(cx, 201 + k, ASM_BP) for k, cx in enumerate(ctxs)]
    for k, b in enumerate(bs):
        b.run(after=bs[k - 1] if k > 0 else None)
    bs[-1].sync()
    for b in bs:
        check(b)
    for cx in ctxs:
        cx.close()


# ---- the assembly sweeps' decode fallbacks ----

@pytest.fixture(scope="module")
def ctx():
    c = cp.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("threshold", [0.01, 1e-7, 0.0])
def test_assembly_decode_paths_match_oracle(ctx, threshold):
    """after the assembly sweep back: the candidate decode (1e-7: long candidate lists that overflow, 0: every cell,
    the count-then-allocate re-run) and the full-scan decode (CPECAN_FLAG_SCAN_DECODE), against the oracle and each
    other"""
    batch = synth.make_batch(221, 3, 700, 1400, anchor_every=50)
    bp = band_params(threshold, 300, 40, 100)
    runs = []
    for flags in (0, cp.FLAG_SCAN_DECODE):
        res, b = run_gpu(ctx, batch, bp, flags=flags, ragged=RAGGED)
        assert b.info()["assembly_sweeps"] == 2
        b.close()
        runs.append(res)
    for i in range(3):
        ref = run_oracle_item(batch, i, bp, RAGGED)
        for res in runs:
            assert_same_posterior(res[i], ref, i)
        assert np.array_equal(runs[0][i]["triples"], runs[1][i]["triples"])
        assert np.array_equal(runs[0][i]["logp"], runs[1][i]["logp"])


def test_assembly_batch_with_degenerate_items(ctx):
    """empty and 1 x 1 alignments inside a batch that runs on the assembly sweeps"""
    batch = synth.make_batch(222, 3, 700, 1400, anchor_every=50)
    base = batch["items"][0]
    batch["items"] += [dict(base, lX=0, n_anchors=0), dict(base, lY=0, n_anchors=0),
                       dict(base, lX=0, lY=0, n_anchors=0), dict(base, lX=1, lY=1, n_anchors=0)]
    res, b = run_gpu(ctx, batch, ASM_BP, ragged=RAGGED)
    assert b.info()["assembly_sweeps"] == 2
    b.close()
    for i in range(len(batch["items"])):
        ref = run_oracle_item(batch, i, ASM_BP, RAGGED)
        if i < 3:
            assert_same_posterior(res[i], ref, i)
        else:  # (an empty alignment's in-band cell count is the library's own: the bar of the compiled kernels' test)
            assert np.array_equal(res[i]["totals_xay"], ref["totals_xay"]), i
            assert np.array_equal(res[i]["totals"], ref["totals"]), i
            assert_same_pairs(res[i], ref)

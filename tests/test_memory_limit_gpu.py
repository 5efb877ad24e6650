"""Device-memory accounting and the per-context limit of the C-ABI (cpecan_hip_batch_device_bytes, cpecan_hip_ctx_memory,
cpecan_hip_ctx_set_memory_limit, CPECAN_ELIMIT), through binding.py.

The limit L sits just above what a 4-read batch needs over its whole life (stream_api.limit_case): that figure plus the
room the allocator's block reuse may take, a quarter and 4 KB per block.  The same 16 reads hold more than twice that."""
import numpy as np
import pytest

import stream_api as sa
from harness import batch_results, cp, make_items

pytestmark = pytest.mark.gpu


def _create(ctx, batch, bp):
    return cp.Batch(ctx, make_items(batch, (1, 1)), batch["x_chars"], batch["events"], batch["anchors"], bp,
                    cp.MODE_POSTERIOR, cp.KERNEL_AUTO, cp.FLAG_SMALL_FOOTPRINT)


def _models(ctx, batch):
    ctx.models_clear()
    ctx.models_create([(cp.NANOPORE_TRANSITIONS,) + tuple(batch["models"][0])])


def test_limit_refuses_the_large_batch_and_leaves_the_context_usable():
    free = cp.Context(0)
    case = sa.limit_case(cp, free)
    b4, b16, L, bp = case["b4"], case["b16"], case["L"], case["bp"]
    print("device bytes: 4 reads %d, 16 reads %d, 4 reads over their life %d, limit %d" % (b4, b16, case["need4"], L))
    assert b4 > 0 and L > b4 and b16 > 2 * L

    # the unlimited context's results of the 4-read batch
    _models(free, case["batch4"])
    ref = _create(free, case["batch4"], bp)
    ref.run()
    ref.sync()
    want = batch_results(ref)
    assert free.memory()["live"] >= ref.device_bytes() > 0
    ref.close()

    ctx = cp.Context(0)
    assert ctx.memory() == dict(live=0, peak=0)
    ctx.set_memory_limit(L)
    _models(ctx, case["batch4"])
    tables = ctx.memory()["live"]
    assert tables > 0
    b = _create(ctx, case["batch4"], bp)
    assert ctx.memory()["live"] == tables + b.device_bytes()
    b.run()
    b.sync()
    got = batch_results(b)
    for g, w in zip(got, want):
        assert np.array_equal(g["triples"], w["triples"]) and np.array_equal(g["logp"], w["logp"])
        assert np.array_equal(g["totals"], w["totals"]) and len(g["triples"]) > 0
    assert ctx.memory()["peak"] <= L
    b.close()
    assert ctx.memory()["live"] == tables

    # the same 16 reads do not fit: CPECAN_ELIMIT, everything taken is released, the context goes on
    before = ctx.memory()["live"]
    with pytest.raises(cp.CpecanError) as ei:
        _create(ctx, case["batch16"], bp)
    assert ei.value.code == cp.ELIMIT
    assert str(L) in str(ei.value) and "limit" in str(ei.value)
    assert ctx.memory()["live"] == before
    assert ctx.memory()["peak"] <= L
    again = _create(ctx, case["batch4"], bp)
    again.run()
    again.sync()
    for g, w in zip(batch_results(again), want):
        assert np.array_equal(g["triples"], w["triples"])
    assert ctx.memory()["peak"] <= L
    again.close()

    # a run refused for its pack buffers (the limit set to what the context holds: nothing more fits) leaves a batch
    # that runs once the limit is lifted, with the same results
    ctx.set_memory_limit(0)
    fresh = _create(ctx, case["batch4"], bp)
    held = ctx.memory()["live"]
    ctx.set_memory_limit(held)
    with pytest.raises(cp.CpecanError) as ei:
        fresh.run()
    assert ei.value.code == cp.ELIMIT and ctx.memory()["live"] == held
    ctx.set_memory_limit(0)
    fresh.run()
    fresh.sync()
    for g, w in zip(batch_results(fresh), want):
        assert np.array_equal(g["triples"], w["triples"]) and np.array_equal(g["totals"], w["totals"])
    fresh.close()

    # the same for a readback: at threshold 0 the items' shares of the pair buffer are too small, the readback grows
    # them, and the limit refuses the larger buffer; with the limit lifted the same call runs the batch again and
    # gives what an unlimited context gives
    flat = cp.BandParams(0.0, bp.minDiagsBetweenTraceBack, bp.traceBackDiagonals, bp.diagonalExpansion)
    _models(free, case["batch4"])
    ref = _create(free, case["batch4"], flat)
    ref.run()
    ref.sync()
    want_flat = batch_results(ref)
    ref.close()
    assert sum(len(w["triples"]) for w in want_flat) > sum(4 * (it["lX"] + it["lY"]) + 64 for it in case["batch4"]["items"])
    grown = _create(ctx, case["batch4"], flat)
    grown.run()
    grown.sync()
    held = ctx.memory()["live"]
    ctx.set_memory_limit(held)
    with pytest.raises(cp.CpecanError) as ei:
        grown.counts()
    assert ei.value.code == cp.ELIMIT
    with pytest.raises(cp.CpecanError) as ei:  # (and again, while nothing has changed)
        grown.pairs(0, 1)
    assert ei.value.code == cp.ELIMIT
    ctx.set_memory_limit(0)
    for g, w in zip(batch_results(grown), want_flat):
        assert np.array_equal(g["triples"], w["triples"]) and np.array_equal(g["logp"], w["logp"])
        assert np.array_equal(g["totals"], w["totals"])
    grown.close()

    # a limit below the model table refuses the table, and lifting it lets the context work again
    ctx.models_clear()
    assert ctx.memory()["live"] == 0
    ctx.set_memory_limit(4096)
    with pytest.raises(cp.CpecanError) as ei:
        ctx.models_create([(cp.NANOPORE_TRANSITIONS,) + tuple(case["batch4"]["models"][0])])
    assert ei.value.code == cp.ELIMIT and ctx.memory()["live"] == 0
    ctx.set_memory_limit(0)
    _models(ctx, case["batch4"])
    assert ctx.memory(reset_peak=True)["live"] == tables and ctx.memory()["peak"] == tables
    ctx.close()
    free.close()

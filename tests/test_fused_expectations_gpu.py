"""The strawMan E-step with its Baum-Welch expectations summed inside the wave kernels' sweep back
(the default; CPECAN_EXPECT_FUSED=0 opts out): which batches take it, and its sums against the oracle and against the path through the ring
of backward cells and the expectation kernel."""
import os

import numpy as np
import pytest

import dist_em
import pyoracle as o
import synth
from harness import band_params, cp, hdp_batch, make_items, run_oracle_item, with_gap_switch

pytestmark = pytest.mark.gpu


def _run(ctx, batch, bp, mode=cp.MODE_EXPECTATIONS, flags=0, ragged=(1, 1), transitions=None, after=None):
    t = transitions if transitions is not None else cp.NANOPORE_TRANSITIONS
    ctx.models_clear()
    ctx.models_create([(t, m, gx, gy) for (m, gx, gy) in batch["models"]])
    b = cp.Batch(ctx, make_items(batch, ragged), batch["x_chars"], batch["events"], batch["anchors"], bp, mode,
                 cp.KERNEL_AUTO, flags)
    b.run()
    b.sync()
    return b


def _expectations(b, batch):
    return [b.expectations(k) for k in range(len(batch["models"]))]


def _oracle(batch, bp, ragged=(1, 1), transitions=None):
    out = []
    for k in range(len(batch["models"])):
        hmm = o.OrcExpectations()
        for i, it in enumerate(batch["items"]):
            if it["model"] == k:
                run_oracle_item(batch, i, bp, ragged, transitions=transitions, expectations=hmm)
        out.append(np.concatenate([np.array(hmm.transitions), np.array(hmm.kmerGap), [hmm.likelihood]]))
    return out


def _assert_close(got, ref, rtol=1e-9, atol=1e-12):
    for g, r in zip(got, ref):
        assert np.allclose(g[:-1], r[:-1], rtol=rtol, atol=atol)
        assert np.isclose(g[-1], r[-1], rtol=1e-12) and g[-1] < 0


# (diagonal expansion, band width, cells per lane)
SHAPES = [(40, 120, 2), (100, 300, 3), (150, 300, 4)]


@pytest.mark.parametrize("expansion,width,cells", SHAPES)
def test_fused_batches_match_the_oracle(monkeypatch, expansion, width, cells):
    monkeypatch.setenv("CPECAN_EXPECT_FUSED", "1")
    ctx = cp.Context(0)
    batch = synth.make_batch(11 + cells, 4, 700, 1400, anchor_every=50)  # several models, ragged ends
    bp = band_params(0.01, width, 40, expansion)
    b = _run(ctx, batch, bp)
    info = b.info()
    assert info.get("cells_per_lane") == cells and info["fused_expectations"] == 1, info
    got = _expectations(b, batch)
    b.close()
    _assert_close(got, _oracle(batch, bp))
    ctx.close()


def test_fused_against_the_ring_of_backward_cells(monkeypatch):
    ctx = cp.Context(0)
    batch = synth.make_batch(5, 5, 600, 1200, anchor_every=40)
    bp = band_params(0.01, 300, 40, 100)
    monkeypatch.setenv("CPECAN_EXPECT_FUSED", "0")
    b = _run(ctx, batch, bp)
    assert b.info()["fused_expectations"] == 0
    ring = _expectations(b, batch)
    b.close()
    monkeypatch.setenv("CPECAN_EXPECT_FUSED", "1")
    b = _run(ctx, batch, bp)
    assert b.info()["fused_expectations"] == 1
    fused = _expectations(b, batch)
    b.close()
    for f, r in zip(fused, ring):
        assert np.allclose(f[:-1], r[:-1], rtol=1e-11, atol=1e-300)
        assert np.isclose(f[-1], r[-1], rtol=1e-12)
    ctx.close()


def test_forced_resweep_and_gap_switch(monkeypatch):
    """every window down the fallback (swept back once more against the exact totals), with and without a model that
    lets gap Y switch to gap X"""
    monkeypatch.setenv("CPECAN_EXPECT_FUSED", "1")
    monkeypatch.setenv("CPECAN_EXPECT_RESWEEP", "1")
    ctx = cp.Context(0)
    batch = synth.make_batch(23, 3, 600, 1200, anchor_every=40)
    bp = band_params(0.01, 120, 40, 40)
    for t in (None, with_gap_switch(cp.NANOPORE_TRANSITIONS, 0.05)):
        b = _run(ctx, batch, bp, transitions=t)
        assert b.info()["fused_expectations"] == 1
        got = _expectations(b, batch)
        b.close()
        _assert_close(got, _oracle(batch, bp, transitions=t))
    ctx.close()


def test_other_batches_keep_the_ring_of_backward_cells(monkeypatch):
    monkeypatch.setenv("CPECAN_EXPECT_FUSED", "1")
    ctx = cp.Context(0)
    batch = synth.make_batch(3, 2, 300, 600, anchor_every=30)
    bp = band_params(0.01, 120, 40, 40)
    for mode, flags in ((cp.MODE_POSTERIOR, 0), (cp.MODE_EXPECTATIONS, cp.FLAG_WORKGROUP_KERNELS)):
        b = _run(ctx, batch, bp, mode=mode, flags=flags)
        assert b.info()["fused_expectations"] == 0
        b.close()
    monkeypatch.delenv("CPECAN_EXPECT_FUSED")
    b = _run(ctx, batch, bp)
    assert b.info()["fused_expectations"] == 1  # the default
    b.close()
    monkeypatch.setenv("CPECAN_EXPECT_FUSED", "0")
    b = _run(ctx, batch, bp)
    assert b.info()["fused_expectations"] == 0
    b.close()
    ctx.close()


def test_gap_switch_on_the_estimate_path(monkeypatch):
    """a model that lets gap Y switch to gap X, the sums scaled from the estimate (no forced re-sweep)"""
    monkeypatch.setenv("CPECAN_EXPECT_FUSED", "1")
    ctx = cp.Context(0)
    batch = synth.make_batch(29, 3, 700, 1400, anchor_every=50)
    t = with_gap_switch(cp.NANOPORE_TRANSITIONS, 0.05)
    for expansion in (40, 100):
        bp = band_params(0.01, 300, 40, expansion)
        b = _run(ctx, batch, bp, transitions=t)
        assert b.info()["fused_expectations"] == 1
        got = _expectations(b, batch)
        b.close()
        _assert_close(got, _oracle(batch, bp, transitions=t))
    ctx.close()


def test_chained_rounds_and_two_contexts(monkeypatch):
    """two batches of two contexts, the second run behind the first (run(after=...)), three rounds; the segment
    records in scratch are reused from round to round"""
    monkeypatch.setenv("CPECAN_EXPECT_FUSED", "1")
    bp = band_params(0.01, 300, 40, 100)
    batches = [synth.make_batch(31, 3, 600, 1200, anchor_every=40), synth.make_batch(32, 3, 600, 1200, anchor_every=40)]
    ctxs = [cp.Context(0), cp.Context(0)]
    bs = []
    for ctx, batch in zip(ctxs, batches):
        ctx.models_clear()
        ctx.models_create([(cp.NANOPORE_TRANSITIONS, m, gx, gy) for (m, gx, gy) in batch["models"]])
        bs.append(cp.Batch(ctx, make_items(batch, (1, 1)), batch["x_chars"], batch["events"], batch["anchors"], bp,
                           cp.MODE_EXPECTATIONS, cp.KERNEL_AUTO, 0))
        assert bs[-1].info()["fused_expectations"] == 1
    refs = [_oracle(batch, bp) for batch in batches]
    for _ in range(3):
        bs[0].run()
        bs[1].run(after=bs[0])
        for b, batch, ref in zip(bs, batches, refs):
            b.sync()
            _assert_close(_expectations(b, batch), ref)
    for b in bs:
        b.close()
    for c in ctxs:
        c.close()


def test_persistent_e_step_after_a_model_change(monkeypatch):
    monkeypatch.setenv("CPECAN_EXPECT_FUSED", "1")
    ctx, ctx3, ctx4 = cp.Context(0), cp.Context(0), cp.Context(0)
    batch = synth.make_batch(47, 6, 150, 310, anchor_every=30)
    bp = band_params(0.01, 100, 20, 40)
    reads = list(range(len(batch["items"])))
    gap0 = batch["models"][0][1]
    got = dist_em.gpu_e_step(cp, ctx, batch, bp, reads, cp.NANOPORE_TRANSITIONS, gap0)
    hmm = o.OrcExpectations()
    for i in reads:
        run_oracle_item(batch, i, bp, (1, 1), expectations=hmm)
    ref = np.concatenate([np.array(hmm.transitions), np.array(hmm.kmerGap), [hmm.likelihood]])
    assert np.allclose(got, ref, rtol=1e-9, atol=1e-12)
    keep = dist_em.PersistentEStep(cp, [ctx3, ctx4], batch, bp, reads, cp.NANOPORE_TRANSITIONS, gap0)
    assert np.allclose(keep(cp.NANOPORE_TRANSITIONS, gap0), got, rtol=1e-12, atol=1e-300)
    t1, g1 = dist_em.m_step(got + np.r_[np.full(dist_em.EXP_LEN - 1, 1e-9), 0.0])
    again = keep(t1, g1)
    assert np.allclose(again, dist_em.gpu_e_step(cp, ctx, batch, bp, reads, t1, g1), rtol=1e-12, atol=1e-300)
    assert again[-1] > got[-1]
    keep.close()
    for c in (ctx, ctx3, ctx4):
        c.close()


def test_vanilla_and_hdp_batches_keep_the_ring(monkeypatch, golden_dir, template_model):
    monkeypatch.setenv("CPECAN_EXPECT_FUSED", "1")
    ctx = cp.Context(0)
    bp = band_params(0.01, 120, 40, 40)
    batch = synth.make_batch(57, 2, 300, 600, anchor_every=30)
    match, skip, gapy = template_model
    m = o.VanillaModel(match, skip, gapy)
    ctx.models_clear()
    ctx.modelsv_create([(m.scalars, m.match, m.skip, m.gap_y)] * len(batch["models"]))
    b = cp.Batch(ctx, make_items(batch, (1, 1)), batch["x_chars"], batch["events"], batch["anchors"], bp,
                 cp.MODE_EXPECTATIONS, vanilla=True)
    assert b.info()["fused_expectations"] == 0
    b.close()
    nhdp = o.load_nhdp(os.path.join(golden_dir, "testTemplate.nhdp"))
    hb, _ = hdp_batch(61, 2, 400, 80, nhdp)
    ctx.models_clear()
    ctx.modelsh_create([(cp.NANOPORE_TRANSITIONS, nhdp["alphabet"], nhdp["grid"], nhdp["y"], nhdp["slope"],
                         nhdp["kmer_row"])])
    b = cp.Batch(ctx, make_items(hb, (1, 1)), hb["x_chars"], hb["events"], hb["anchors"], bp, cp.MODE_EXPECTATIONS,
                 hdp=True)
    assert b.info()["fused_expectations"] == 0
    b.close()
    ctx.close()

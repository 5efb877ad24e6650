"""The strawMan E-step with its Baum-Welch expectations summed inside the sweep back of the workgroup-per-alignment
kernels (CPECAN_FLAG_WORKGROUP_FUSED_ESTEP, or CPECAN_EXPECT_FUSED_WORKGROUP=1; the fused builds of one to four waves,
cpecan_k_sy_backward_f1.._f4): its sums against the oracle at each width, against the same kernels' path through the
ring of backward cells and the expectation kernel, down the fallback (windows swept back once more against the exact
totals), where the oracle has NaN, in batches that are run again and chained, and on a short seeded fuzz; and which
batches ignore the flag.

The bars are the suite's for expectations (tests/test_fused_expectations_gpu.py, tests/test_fuzz_expectations_gpu.py):
the 9 transitions and 4096 gap-X bins to rtol 1e-9 / atol 1e-12 of the oracle and the likelihood to rtol 1e-12; fused
against the ring to rtol 1e-11 / atol 1e-300 and rtol 1e-12; NaN exactly where the oracle has NaN.  One more needs no
oracle: every gap-X term enters one transition and one k-mer bin, so for reads of ACGT the bins sum to the three gap-X
transitions (rtol 1e-12) -- a per-slot gap record that is dropped or counted twice shows there.

Band widths: with anchors every 50 k-mers and twice as many events as k-mers the widest band is 52 + expansion k-mers,
so expansions 4, 40, 100 and 150 give 56, 92, 152 and 202 k-mers: one, two, three and four waves per workgroup, the
first with the band filling the one-wave build's slots exactly."""
import os

import numpy as np
import pytest

import dist_em
import pyoracle as o
import synth
from harness import band_params, cp, hdp_batch, make_items, run_gpu, with_gap_switch
from test_fuzz_expectations_gpu import (DEGENERATE, assert_expectations_match, assert_gap_x_invariant,
                                        assert_same_totals, case_batch, case_id, cases, ctx, env, non_acgt_batch,
                                        oracle_expectations, trained, transitions_of)

__all__ = ["ctx", "trained"]  # (the fuzz module's fixtures: one context, one trained transition set)

WG = cp.FLAG_WORKGROUP_KERNELS
FUSED = cp.FLAG_WORKGROUP_KERNELS | cp.FLAG_WORKGROUP_FUSED_ESTEP
SWITCH = with_gap_switch(cp.NANOPORE_TRANSITIONS, 0.05)
EXPANSION = {1: 4, 2: 40, 3: 100, 4: 150}  # waves per workgroup -> diagonal expansion (see above)
_ORACLE = {}


def rows_of(width):
    return 1 + (width > 56) + (width > 120) + (width > 184)


def shape(rows, seed=50, n=4, lX=700, lY=1400):
    """n reads with a model each, ragged ends, several traceback windows per read, at the band width of `rows` waves"""
    return (synth.make_batch(seed + rows, n, lX, lY, anchor_every=50), band_params(0.01, 300, 40, EXPANSION[rows]))


def oracle(key, batch, bp, ragged=(1, 1), t=None):
    if key not in _ORACLE:
        _ORACLE[key] = oracle_expectations(batch, bp, ragged, t)
    return _ORACLE[key]


def run(ctx, batch, bp, flags=FUSED, ragged=(1, 1), t=None, **environment):
    """(per-item results, info(), per-model expectation vectors) of one expectation batch"""
    with env(**environment):
        res, b = run_gpu(ctx, batch, bp, mode=cp.MODE_EXPECTATIONS, kernel=cp.KERNEL_AUTO, flags=flags, ragged=ragged,
                         transitions=t)
    info = b.info()
    got = [b.expectations(k) for k in range(len(batch["models"]))]
    b.close()
    return res, info, got


def assert_fused(info, rows):
    assert info["kernel"] == "systolic" and info["family"] == "workgroup", info
    assert info["waves_per_workgroup"] == rows and info["fused_expectations"] == 1, info


def assert_close(got, ref):
    """tests/test_fused_expectations_gpu.py::_assert_close"""
    for g, r in zip(got, ref):
        assert np.allclose(g[:-1], r[:-1], rtol=1e-9, atol=1e-12), \
            np.flatnonzero(~np.isclose(g[:-1], r[:-1], rtol=1e-9, atol=1e-12))[:20]
        assert np.isclose(g[-1], r[-1], rtol=1e-12) and g[-1] < 0
        assert_gap_x_invariant(g)


def assert_ring_close(fused, ring):
    """the bar of test_fused_against_the_ring_of_backward_cells"""
    for f, r in zip(fused, ring):
        assert np.allclose(f[:-1], r[:-1], rtol=1e-11, atol=1e-300), \
            np.flatnonzero(~np.isclose(f[:-1], r[:-1], rtol=1e-11, atol=1e-300))[:20]
        assert np.isclose(f[-1], r[-1], rtol=1e-12)


# ------------------------------------------ 1. against the oracle at each width ------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [1, 2, 3, 4])
def test_fused_matches_the_oracle(ctx, rows):
    batch, bp = shape(rows)
    ref_items, ref = oracle(("shape", rows), batch, bp)
    assert all(len(r["totals"]) > 50 for r in ref_items)  # five windows or more per item
    res, info, got = run(ctx, batch, bp)
    assert_fused(info, rows)
    assert_same_totals(res, ref_items)
    assert_close(got, ref)


# ------------------------------------------------ 2. against the ring path ------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [1, 2, 3, 4])
def test_fused_against_the_ring_of_backward_cells(ctx, rows):
    batch, bp = shape(rows, seed=70, n=5, lX=600, lY=1200)
    res, info, ring = run(ctx, batch, bp, flags=WG)
    assert info["family"] == "workgroup" and info["waves_per_workgroup"] == rows and info["fused_expectations"] == 0
    res_f, info, fused = run(ctx, batch, bp)
    assert_fused(info, rows)
    assert_same_totals(res_f, res)
    assert_ring_close(fused, ring)


# ----------------------------------------------------- 3. the fallback -----------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("t", [None, SWITCH], ids=["defaults", "switch"])
@pytest.mark.parametrize("resweep", ["1", "2"])
@pytest.mark.parametrize("rows", [1, 3])
def test_forced_resweep(ctx, rows, resweep, t):
    """every window (1), or the windows whose item and window parity differ (2: one launch has both paths and an item
    alternates between them), swept back once more against the exact totals"""
    batch, bp = shape(rows, seed=80, n=3, lX=600, lY=1200)
    ref_items, ref = oracle(("resweep", rows, t is None), batch, bp, t=t)
    res, info, got = run(ctx, batch, bp, t=t, CPECAN_EXPECT_RESWEEP=resweep)
    assert_fused(info, rows)
    assert_same_totals(res, ref_items)
    assert_close(got, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [2, 4])
def test_gap_switch_on_the_estimate_path(ctx, rows):
    """a model that lets gap Y switch to gap X (the ninth term), the sums scaled from the estimate"""
    batch, bp = shape(rows, seed=90, n=3)
    ref_items, ref = oracle(("switch", rows), batch, bp, t=SWITCH)
    res, info, got = run(ctx, batch, bp, t=SWITCH, CPECAN_EXPECT_RESWEEP=None)
    assert_fused(info, rows)
    assert_same_totals(res, ref_items)
    assert got[0][7] > 0  # gap Y -> gap X is taken
    assert_close(got, ref)


# ---------------------------------------------------- 4. NaN placement ----------------------------------------------------


def nan_batch():
    """three 300 x 600 reads, the second with an N in its middle; then, on the first read's bytes and events and with a
    model each, an item without k-mers (0 x 5) and one of fewer k-mers than a band is wide (20 x 45)"""
    batch = non_acgt_batch(301, 3, 300, 600, 1, 150, "N")
    base, m0 = batch["items"][0], batch["models"][0]
    items, models = list(batch["items"]), list(batch["models"])
    assert (0, 5) in DEGENERATE
    for lX, lY in ((0, 5), (20, 45)):
        items.append(dict(base, lX=lX, lY=lY, n_anchors=0, model=len(models)))
        models.append(m0)
    return dict(batch, items=items, models=models)


def test_nan_batch_on_the_oracle():
    """(CPU) the comparison below is not empty: the oracle alone has NaN sums for the read with the N and for the item
    without k-mers, and finite blocks for the others"""
    for rows in (1, 2):
        _, ref = oracle(("nan", rows), nan_batch(), band_params(0.01, 100, 40, EXPANSION[rows]))
        assert np.any(np.isnan(ref[1])) and np.any(np.isnan(ref[3]))
        assert sum(1 for v in ref if np.all(np.isfinite(v))) == 3 and np.all(np.isfinite(ref[4]))


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [1, 2])
def test_nan_where_the_oracle_and_the_ring_have_nan(ctx, rows):
    batch = nan_batch()
    bp = band_params(0.01, 100, 40, EXPANSION[rows])
    ref_items, ref = oracle(("nan", rows), batch, bp)
    _, info, ring = run(ctx, batch, bp, flags=WG)
    assert info["family"] == "workgroup" and info["fused_expectations"] == 0, info
    res, info, got = run(ctx, batch, bp)
    assert_fused(info, rows)
    assert_same_totals(res, ref_items)
    for k, (g, r, q) in enumerate(zip(got, ref, ring)):
        assert np.array_equal(np.isnan(g), np.isnan(r)), (k, np.flatnonzero(np.isnan(g) != np.isnan(r))[:20])
        assert np.array_equal(np.isnan(g), np.isnan(q)), (k, np.flatnonzero(np.isnan(g) != np.isnan(q))[:20])
        assert_expectations_match(g, r, k)  # the same non-finite entries, the finite ones to the oracle's bar
        ok = np.isfinite(q)
        assert np.allclose(g[:-1][ok[:-1]], q[:-1][ok[:-1]], rtol=1e-11, atol=1e-300), k
        if ok[-1]:
            assert np.isclose(g[-1], q[-1], rtol=1e-12), k


# --------------------------------------------------- 5. who ignores it ---------------------------------------------------


@pytest.mark.gpu
def test_the_variable_alone_turns_a_workgroup_batch_fused(ctx):
    batch, bp = shape(2, seed=100, n=2, lX=300, lY=600)
    _, ref = oracle("variable", batch, bp)
    _, info, got = run(ctx, batch, bp, flags=WG, CPECAN_EXPECT_FUSED_WORKGROUP="1")
    assert_fused(info, 2)
    assert_close(got, ref)
    for value in ("0", None):  # ... and nothing else does
        _, info, _ = run(ctx, batch, bp, flags=WG, CPECAN_EXPECT_FUSED_WORKGROUP=value)
        assert info["family"] == "workgroup" and info["fused_expectations"] == 0, info


@pytest.mark.gpu
def test_a_posterior_batch_ignores_the_flag(ctx):
    batch, bp = shape(2, seed=100, n=2, lX=300, lY=600)
    out = []
    for flags in (WG, FUSED):
        res, b = run_gpu(ctx, batch, bp, mode=cp.MODE_POSTERIOR, kernel=cp.KERNEL_AUTO, flags=flags, ragged=(1, 1))
        info = b.info()
        b.close()
        assert info["family"] == "workgroup" and info["fused_expectations"] == 0, info
        out.append(res)
    for g, r in zip(*out):
        assert np.array_equal(g["triples"], r["triples"]) and np.array_equal(g["logp"], r["logp"])
        assert np.array_equal(g["totals"], r["totals"])


@pytest.mark.gpu
def test_a_wave_batch_stays_on_its_own_fused_pass(ctx):
    batch, bp = shape(2, seed=100, n=2, lX=300, lY=600)
    out = []
    for flags, var in ((0, None), (cp.FLAG_WORKGROUP_FUSED_ESTEP, "1")):
        _, info, got = run(ctx, batch, bp, flags=flags, CPECAN_EXPECT_FUSED_WORKGROUP=var, CPECAN_EXPECT_FUSED=None)
        assert info["family"] == "wave" and info["cells_per_lane"] == 2 and info["fused_expectations"] == 1, info
        out.append(got)
    for g, r in zip(*out):
        assert np.allclose(g, r, rtol=1e-12, atol=1e-300)
    # ... and, opted out of that, on its ring of backward cells
    _, info, _ = run(ctx, batch, bp, flags=cp.FLAG_WORKGROUP_FUSED_ESTEP, CPECAN_EXPECT_FUSED="0")
    assert info["family"] == "wave" and info["fused_expectations"] == 0, info


@pytest.mark.gpu
def test_vanilla_and_hdp_batches_ignore_the_flag(ctx, golden_dir, template_model):
    bp = band_params(0.01, 120, 40, 40)
    batch = synth.make_batch(57, 2, 300, 600, anchor_every=30)
    match, skip, gapy = template_model
    m = o.VanillaModel(match, skip, gapy)
    nhdp = o.load_nhdp(os.path.join(golden_dir, "testTemplate.nhdp"))
    hb, _ = hdp_batch(61, 2, 400, 80, nhdp)

    def vanilla(flags):
        ctx.models_clear()
        ctx.modelsv_create([(m.scalars, m.match, m.skip, m.gap_y)] * len(batch["models"]))
        return cp.Batch(ctx, make_items(batch, (1, 1)), batch["x_chars"], batch["events"], batch["anchors"], bp,
                        flags=cp.FLAG_EXPECTATIONS | flags, vanilla=True), len(batch["models"])

    def hdp(flags):
        ctx.models_clear()
        ctx.modelsh_create([(cp.NANOPORE_TRANSITIONS, nhdp["alphabet"], nhdp["grid"], nhdp["y"], nhdp["slope"],
                             nhdp["kmer_row"])])
        return cp.Batch(ctx, make_items(hb, (1, 1)), hb["x_chars"], hb["events"], hb["anchors"], bp,
                        flags=cp.FLAG_EXPECTATIONS | flags, hdp=True), 1

    for create in (vanilla, hdp):
        out = []
        for flags, var in ((0, None), (cp.FLAG_WORKGROUP_FUSED_ESTEP, "1")):
            with env(CPECAN_EXPECT_FUSED_WORKGROUP=var):
                b, n = create(flags)
            b.run()
            b.sync()
            assert b.info()["fused_expectations"] == 0, b.info()
            out.append((b.info(), [b.expectations(k) for k in range(n)]))
            b.close()
        assert out[0][0] == out[1][0]
        for g, r in zip(out[0][1], out[1][1]):
            assert np.allclose(g, r, rtol=1e-12, atol=1e-300, equal_nan=True)


@pytest.mark.gpu
def test_a_wide_bands_batch_keeps_the_ring(ctx):
    """300 k-mers of band: the six-wave build of CPECAN_FLAG_WIDE_BANDS, which has no fused form"""
    batch = synth.make_batch(24, 1, 400, 800, anchor_every=400)
    bp = band_params(0.01, 200, 40, 196)
    out = []
    for flags in (WG | cp.FLAG_WIDE_BANDS, FUSED | cp.FLAG_WIDE_BANDS):
        _, info, got = run(ctx, batch, bp, flags=flags)
        assert info["max_band_width"] == 300, info
        assert info["family"] == "workgroup" and info["waves_per_workgroup"] == 6 and info["fused_expectations"] == 0
        out.append(got)
    for g, r in zip(*out):
        assert np.allclose(g, r, rtol=1e-12, atol=1e-300)


# ------------------------------------------------ 6. reuse and concurrency ------------------------------------------------


@pytest.mark.gpu
def test_a_batch_run_three_times(ctx):
    """the segment records of a run are the next run's scratch: the same sums each time"""
    batch, bp = shape(1, seed=110, n=3, lX=600, lY=1200)
    _, ref = oracle("thrice", batch, bp)
    ctx.models_clear()
    ctx.models_create([(cp.NANOPORE_TRANSITIONS, m, gx, gy) for (m, gx, gy) in batch["models"]])
    b = cp.Batch(ctx, make_items(batch, (1, 1)), batch["x_chars"], batch["events"], batch["anchors"], bp,
                 cp.MODE_EXPECTATIONS, cp.KERNEL_AUTO, FUSED)
    assert_fused(b.info(), 1)
    runs = []
    for _ in range(3):
        b.run()
        b.sync()
        runs.append([b.expectations(k) for k in range(len(batch["models"]))])
        assert_close(runs[-1], ref)
    b.close()
    for again in runs[1:]:
        assert_ring_close(again, runs[0])  # (atomic additions: equal to rounding)


@pytest.mark.gpu
def test_chained_rounds_and_two_contexts():
    """a fused workgroup batch on each of two contexts, the second run behind the first, three rounds"""
    bp = band_params(0.01, 300, 40, 100)
    batches = [synth.make_batch(31, 3, 600, 1200, anchor_every=50), synth.make_batch(32, 3, 600, 1200, anchor_every=50)]
    refs = [oracle(("chain", k), batch, bp)[1] for k, batch in enumerate(batches)]
    ctxs = [cp.Context(0), cp.Context(0)]
    bs = []
    for c, batch in zip(ctxs, batches):
        c.models_clear()
        c.models_create([(cp.NANOPORE_TRANSITIONS, m, gx, gy) for (m, gx, gy) in batch["models"]])
        bs.append(cp.Batch(c, make_items(batch, (1, 1)), batch["x_chars"], batch["events"], batch["anchors"], bp,
                           cp.MODE_EXPECTATIONS, cp.KERNEL_AUTO, FUSED))
        assert_fused(bs[-1].info(), 3)
    for _ in range(3):
        bs[0].run()
        bs[1].run(after=bs[0])
        for b, batch, ref in zip(bs, batches, refs):
            b.sync()
            assert_close([b.expectations(k) for k in range(len(batch["models"]))], ref)
    for b in bs:
        b.close()
    for c in ctxs:
        c.close()


@pytest.mark.gpu
def test_persistent_e_step_after_a_model_change(monkeypatch):
    """em.PersistentEStep over two contexts picks the workgroup kernels; the variable makes its batches fused"""
    monkeypatch.setenv("CPECAN_EXPECT_FUSED_WORKGROUP", "1")
    one, ctx3, ctx4 = cp.Context(0), cp.Context(0), cp.Context(0)
    batch = synth.make_batch(47, 6, 150, 310, anchor_every=30)
    bp = band_params(0.01, 100, 20, 40)
    reads = list(range(len(batch["items"])))
    gap0 = batch["models"][0][1]
    got = dist_em.gpu_e_step(cp, one, batch, bp, reads, cp.NANOPORE_TRANSITIONS, gap0)
    keep = dist_em.PersistentEStep(cp, [ctx3, ctx4], batch, bp, reads, cp.NANOPORE_TRANSITIONS, gap0)
    for _, b in keep.batches:
        info = b.info()
        assert info["family"] == "workgroup" and info["fused_expectations"] == 1, info
    assert np.allclose(keep(cp.NANOPORE_TRANSITIONS, gap0), got, rtol=1e-12, atol=1e-300)
    t1, g1 = dist_em.m_step(got + np.r_[np.full(dist_em.EXP_LEN - 1, 1e-9), 0.0])
    again = keep(t1, g1)
    assert np.allclose(again, dist_em.gpu_e_step(cp, one, batch, bp, reads, t1, g1), rtol=1e-12, atol=1e-300)
    assert again[-1] > got[-1]
    keep.close()
    for c in (one, ctx3, ctx4):
        c.close()


# --------------------------------------------------- 7. a short seeded fuzz ---------------------------------------------------

# the fuzz module's generator, its cases with an expansion of 10..150 (the generator draws even ones: 10, 20, 40, 60, 100,
# 120; 15 is not one getPosteriorProbsWithBanding takes): lengths, traceback spacing, anchors every 8..120 k-mers or none,
# ragged ends, the three transition sets, one model per read or one for all
FUZZ = [c for c in cases(40, 20261019) if 10 <= c["e"] <= 150][:12]


@pytest.mark.gpu
@pytest.mark.parametrize("case", FUZZ, ids=case_id)
def test_random_fused_expectations(ctx, case, request):
    t, gx = transitions_of(case, request.getfixturevalue("trained") if case["tset"] == "trained" else None)
    batch = case_batch(case, gx)
    bp = band_params(case["thr"], case["md"], case["tb"], case["e"])
    ref_items, ref = oracle_expectations(batch, bp, case["ragged"], t)
    res, info, got = run(ctx, batch, bp, ragged=case["ragged"], t=t)
    if info["max_band_width"] > 248:  # (no anchors and a long read: the general kernel, which has no such pass)
        assert info["kernel"] == "general" and info["fused_expectations"] == 0, info
    else:
        assert_fused(info, rows_of(info["max_band_width"]))
    assert_same_totals(res, ref_items)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert_expectations_match(g, r, k)
        assert g[-1] < 0
        assert_gap_x_invariant(g, k)

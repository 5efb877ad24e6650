"""The strawMan E-step with its Baum-Welch expectations summed inside the sweep back of the six- and eight-wave
workgroup kernels (CPECAN_FLAG_WIDE_BANDS_FUSED_ESTEP, or CPECAN_EXPECT_FUSED_WIDE=1; the fused builds
cpecan_k_sy_backward_f6 / _f8, bands of 249..376 and 377..504 k-mers): its sums against the oracle at each width and at
the edges of both builds, against the same kernels' path through the ring of backward cells and the expectation kernel,
down the fallback (windows swept back once more against the exact totals), where the oracle has NaN, in batches that are
run again and chained, and on a short seeded fuzz; and which batches ignore the flag.

The bars are those of tests/test_workgroup_fused_expectations_gpu.py: the 9 transitions and 4096 gap-X bins to rtol 1e-9 /
atol 1e-12 of the oracle and the likelihood to rtol 1e-12; fused against the ring to rtol 1e-11 / atol 1e-300 and rtol
1e-12; totals bit-identical; NaN exactly where the oracle has NaN; and for reads of ACGT the bins sum to the three gap-X
transitions (rtol 1e-12).

Band widths: the shapes are those of tests/test_wide_workgroup_gpu.py (sparse anchors and a wide expansion); the widest
band of the others is computed on the CPU with the oracle's band table (widest_band) and asserted by the CPU tests of
this file."""
import os

import numpy as np
import pytest

import dist_em
import pyoracle as o
import synth
from harness import band_params, cp, hdp_batch, make_items, run_gpu, with_gap_switch, with_gap_x
from test_fuzz_expectations_gpu import (DEGENERATE, assert_expectations_match, assert_gap_x_invariant,
                                        assert_same_totals, ctx, env, non_acgt_batch, oracle_expectations, trained)
from test_wide_workgroup_gpu import SHAPES, build_of, exact_width_batch, shape_batch
from test_workgroup_fused_expectations_gpu import assert_close, assert_ring_close

__all__ = ["ctx", "trained"]  # (the fuzz module's fixtures: one context, one trained transition set)

WG = cp.FLAG_WORKGROUP_KERNELS
WIDE = cp.FLAG_WIDE_BANDS
FUSED = WG | WIDE | cp.FLAG_WIDE_BANDS_FUSED_ESTEP
SWITCH = with_gap_switch(cp.NANOPORE_TRANSITIONS, 0.05)
_ORACLE = {}


def widest_band(batch, e):
    """the widest band of a batch, in k-mers, from the oracle's band table (tests/test_fuzz_expectations_gpu.py)"""
    w = 0
    for it in batch["items"]:
        if it["lX"] == 0 or it["lY"] == 0:
            continue
        an = batch["anchors"][it["anchor_offset"]: it["anchor_offset"] + it["n_anchors"]]
        L, R = o.band(an, it["lX"], it["lY"], e)
        w = max(w, int(((R - L) // 2 + 1).max()))
    return w


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


def assert_wide(info, rows, fused):
    assert info["kernel"] == "systolic" and info["family"] == "workgroup", info
    assert info["waves_per_workgroup"] == rows and build_of(info["max_band_width"]) == rows, info
    assert info["fused_expectations"] == fused, info


def shape_bp(s):
    return band_params(0.01, s["md"], s["tb"], s["e"])


def shape_id(s):
    return "f%d-seed%d" % (s["rows"], s["seed"])


# ------------------------------------------ 1. against the oracle at each width ------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_fused_matches_the_oracle(ctx, shape):
    batch, bp = shape_batch(shape), shape_bp(shape)
    ref_items, ref = oracle(("shape", shape["seed"]), batch, bp, shape["ragged"])
    assert (shape["lX"] + shape["lY"]) // shape["md"] >= 3  # several traceback windows
    res, info, got = run(ctx, batch, bp, ragged=shape["ragged"])
    assert_wide(info, shape["rows"], 1)
    assert_same_totals(res, ref_items)
    assert_close(got, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("width", [249, 376, 377, 504])
def test_fused_at_the_edges_of_the_wide_builds(ctx, width):
    """the alignment on the band's upper edge; 376 and 504 fill every slot of a build"""
    batch, bp = exact_width_batch(width)
    ragged = (width % 2, 1)
    ref_items, ref = oracle(("edge", width), batch, bp, ragged)
    res, info, got = run(ctx, batch, bp, ragged=ragged)
    assert info["max_band_width"] == width
    assert_wide(info, build_of(width), 1)
    assert_same_totals(res, ref_items)
    assert_close(got, ref)


# ------------------------------------------------ 2. against the ring path ------------------------------------------------


def assert_fused_against_the_ring(ctx, batch, bp, ragged, rows):
    res, info, ring = run(ctx, batch, bp, flags=WIDE, ragged=ragged)
    assert_wide(info, rows, 0)
    res_f, info, fused = run(ctx, batch, bp, ragged=ragged)
    assert_wide(info, rows, 1)
    assert_same_totals(res_f, res)
    assert_ring_close(fused, ring)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_fused_against_the_ring_of_backward_cells(ctx, shape):
    assert_fused_against_the_ring(ctx, shape_batch(shape), shape_bp(shape), shape["ragged"], shape["rows"])


@pytest.mark.gpu
@pytest.mark.parametrize("width", [249, 376, 377, 504])
def test_fused_against_the_ring_at_the_edges(ctx, width):
    batch, bp = exact_width_batch(width)
    assert_fused_against_the_ring(ctx, batch, bp, (width % 2, 1), build_of(width))


# ----------------------------------------------------- 3. the fallback -----------------------------------------------------

# rows: (seed, reads, k-mers, events, anchors every, expansion, the widest band that gives)
FALLBACK = {6: (80, 3, 600, 1200, 250, 90, 341), 8: (81, 3, 700, 1400, 300, 180, 481)}


def fallback_shape(rows):
    seed, n, lX, lY, every, e, _ = FALLBACK[rows]
    return synth.make_batch(seed, n, lX, lY, anchor_every=every), band_params(0.01, 300, 40, e)


def test_fallback_band_widths_on_the_oracle():
    """(CPU) the two batches have the widest bands they are named for"""
    for rows, shape in FALLBACK.items():
        batch, bp = fallback_shape(rows)
        assert widest_band(batch, shape[5]) == shape[6] and build_of(shape[6]) == rows


@pytest.mark.gpu
@pytest.mark.parametrize("t", [None, SWITCH], ids=["defaults", "switch"])
@pytest.mark.parametrize("resweep", ["1", "2"])
@pytest.mark.parametrize("rows", [6, 8])
def test_forced_resweep(ctx, rows, resweep, t):
    """every window (1), or the windows whose item and window parity differ (2: one launch has both paths and an item
    alternates between them), swept back once more against the exact totals"""
    batch, bp = fallback_shape(rows)
    ref_items, ref = oracle(("resweep", rows, t is None), batch, bp, t=t)
    res, info, got = run(ctx, batch, bp, t=t, CPECAN_EXPECT_RESWEEP=resweep)
    assert info["max_band_width"] == FALLBACK[rows][6]
    assert_wide(info, rows, 1)
    assert_same_totals(res, ref_items)
    assert_close(got, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [6, 8])
def test_gap_switch_on_the_estimate_path(ctx, rows):
    """a model that lets gap Y switch to gap X (the ninth term), the sums scaled from the estimate"""
    batch, bp = fallback_shape(rows)
    ref_items, ref = oracle(("resweep", rows, False), batch, bp, t=SWITCH)
    res, info, got = run(ctx, batch, bp, t=SWITCH, CPECAN_EXPECT_RESWEEP=None)
    assert_wide(info, rows, 1)
    assert_same_totals(res, ref_items)
    assert got[0][7] > 0  # gap Y -> gap X is taken
    assert_close(got, ref)


# ---------------------------------------------------- 4. NaN placement ----------------------------------------------------

# rows: (k-mers, events, expansion, the widest band, NaN entries in the model of the read with the N)
NAN = {6: (400, 800, 300, 352, 243), 8: (500, 1000, 440, 474, 377)}


def nan_batch(rows):
    """three reads, the second with an N in its middle and one anchor gap as long as the read; then, on the first read's
    bytes and events and with a model each, an item without k-mers (0 x 5) and one of fewer k-mers than a band is wide
    (20 x 45)"""
    lX, lY = NAN[rows][:2]
    batch = non_acgt_batch(301, 3, lX, lY, 1, lX // 2, "N", every=lX)
    base, m0 = batch["items"][0], batch["models"][0]
    items, models = list(batch["items"]), list(batch["models"])
    assert (0, 5) in DEGENERATE
    for x, y in ((0, 5), (20, 45)):
        items.append(dict(base, lX=x, lY=y, n_anchors=0, model=len(models)))
        models.append(m0)
    return dict(batch, items=items, models=models), band_params(0.01, 200, 40, NAN[rows][2])


def test_nan_batch_on_the_oracle():
    """(CPU) the comparison below is not empty: the oracle alone has NaN sums for the read with the N and for the item
    without k-mers and in no other model, and the batches have the bands they are named for"""
    for rows, (_, _, e, width, n_nan) in NAN.items():
        batch, bp = nan_batch(rows)
        assert widest_band(batch, e) == width and build_of(width) == rows
        _, ref = oracle(("nan", rows), batch, bp)
        assert int(np.isnan(ref[1]).sum()) == n_nan and int(np.isnan(ref[3]).sum()) == 2
        for k in (0, 2, 4):
            assert np.all(np.isfinite(ref[k])), k


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [6, 8])
def test_nan_where_the_oracle_and_the_ring_have_nan(ctx, rows):
    batch, bp = nan_batch(rows)
    ref_items, ref = oracle(("nan", rows), batch, bp)
    _, info, ring = run(ctx, batch, bp, flags=WIDE)
    assert_wide(info, rows, 0)
    res, info, got = run(ctx, batch, bp)
    assert info["max_band_width"] == NAN[rows][3]
    assert_wide(info, rows, 1)
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
@pytest.mark.parametrize("rows", [6, 8])
def test_a_posterior_batch_ignores_the_flag(ctx, rows):
    batch, bp = fallback_shape(rows)
    out = []
    for flags in (WIDE, WIDE | cp.FLAG_WIDE_BANDS_FUSED_ESTEP):
        with env(CPECAN_EXPECT_FUSED_WIDE="1" if flags != WIDE else None):
            res, b = run_gpu(ctx, batch, bp, mode=cp.MODE_POSTERIOR, kernel=cp.KERNEL_AUTO, flags=flags, ragged=(1, 1))
        info = b.info()
        b.close()
        assert_wide(info, rows, 0)
        out.append(res)
    for g, r in zip(*out):
        assert np.array_equal(g["triples"], r["triples"]) and np.array_equal(g["logp"], r["logp"])
        assert np.array_equal(g["totals"], r["totals"])


@pytest.mark.gpu
def test_a_band_of_four_waves_stays_on_its_ring_build(ctx):
    """202 k-mers of band: flag 2048's ground, which 4096 does not reach"""
    batch = synth.make_batch(51, 2, 300, 600, anchor_every=50)
    bp = band_params(0.01, 300, 40, 150)
    for flags, var in ((WG | cp.FLAG_WIDE_BANDS_FUSED_ESTEP, None), (WG | WIDE | cp.FLAG_WIDE_BANDS_FUSED_ESTEP, "1")):
        _, info, _ = run(ctx, batch, bp, flags=flags, CPECAN_EXPECT_FUSED_WIDE=var, CPECAN_EXPECT_FUSED_WORKGROUP=None)
        assert info["max_band_width"] == 202, info
        assert info["family"] == "workgroup" and info["waves_per_workgroup"] == 4 and info["fused_expectations"] == 0


@pytest.mark.gpu
def test_without_the_wide_bands_flag_a_wide_band_runs_on_the_general_kernel(ctx):
    batch = synth.make_batch(24, 1, 400, 800, anchor_every=400)
    bp = band_params(0.01, 200, 40, 196)
    _, ref = oracle("general", batch, bp)
    for flags in (cp.FLAG_WIDE_BANDS_FUSED_ESTEP, WG | cp.FLAG_WIDE_BANDS_FUSED_ESTEP):
        _, info, got = run(ctx, batch, bp, flags=flags, CPECAN_EXPECT_FUSED_WIDE="1", CPECAN_WIDE_BANDS=None)
        assert info["max_band_width"] == 300 and info["kernel"] == "general" and info["fused_expectations"] == 0, info
        assert_close(got, ref)


@pytest.mark.gpu
def test_a_band_past_504_runs_on_the_general_kernel(ctx):
    batch, bp = exact_width_batch(505)
    _, info, _ = run(ctx, batch, bp)
    assert info["max_band_width"] == 505 and info["kernel"] == "general" and info["fused_expectations"] == 0, info


@pytest.mark.gpu
def test_vanilla_and_hdp_batches_ignore_the_flag(ctx, golden_dir, template_model):
    """(the construction of tests/test_workgroup_fused_expectations_gpu.py's test of that name)"""
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
        for flags, var in ((0, None), (cp.FLAG_WIDE_BANDS_FUSED_ESTEP, "1")):
            with env(CPECAN_EXPECT_FUSED_WIDE=var):
                b, n = create(flags)
            b.run()
            b.sync()
            assert b.info()["fused_expectations"] == 0, b.info()
            out.append((b.info(), [b.expectations(k) for k in range(n)]))
            b.close()
        assert out[0][0] == out[1][0]
        for g, r in zip(out[0][1], out[1][1]):
            assert np.allclose(g, r, rtol=1e-12, atol=1e-300, equal_nan=True)


# ----------------------------------------------------- 6. the variables -----------------------------------------------------


@pytest.mark.gpu
def test_the_variables(ctx):
    batch, bp = fallback_shape(6)
    _, ref = oracle(("resweep", 6, True), batch, bp)
    off = dict(CPECAN_EXPECT_FUSED_WORKGROUP=None, CPECAN_WIDE_BANDS=None, CPECAN_EXPECT_FUSED_WIDE=None)
    # the variable with the wide-bands flag, and with the wide-bands variable and no flag at all
    for flags, environment in ((WIDE, dict(off, CPECAN_EXPECT_FUSED_WIDE="1")),
                               (0, dict(off, CPECAN_EXPECT_FUSED_WIDE="1", CPECAN_WIDE_BANDS="1"))):
        _, info, got = run(ctx, batch, bp, flags=flags, **environment)
        assert_wide(info, 6, 1)
        assert_close(got, ref)
    # ... and nothing else does: "0", unset, the narrower builds' variable
    for environment in (dict(off, CPECAN_EXPECT_FUSED_WIDE="0"), off, dict(off, CPECAN_EXPECT_FUSED_WORKGROUP="1")):
        _, info, _ = run(ctx, batch, bp, flags=WIDE, **environment)
        assert_wide(info, 6, 0)


# ------------------------------------------------ 7. reuse and concurrency ------------------------------------------------


@pytest.mark.gpu
def test_a_batch_run_three_times(ctx):
    """the segment records of a run are the next run's scratch: the same sums each time"""
    batch, bp = fallback_shape(6)
    _, ref = oracle(("resweep", 6, True), batch, bp)
    ctx.models_clear()
    ctx.models_create([(cp.NANOPORE_TRANSITIONS, m, gx, gy) for (m, gx, gy) in batch["models"]])
    b = cp.Batch(ctx, make_items(batch, (1, 1)), batch["x_chars"], batch["events"], batch["anchors"], bp,
                 cp.MODE_EXPECTATIONS, cp.KERNEL_AUTO, FUSED)
    assert_wide(b.info(), 6, 1)
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
    """an eight-wave fused batch on each of two contexts, the second run behind the first, three rounds"""
    bp = band_params(0.01, 300, 40, 180)
    batches = [fallback_shape(8)[0], synth.make_batch(63, 3, 800, 1600, anchor_every=300)]
    refs = [oracle(("resweep", 8, True), batches[0], bp)[1], oracle(("shape", 63), batches[1], bp)[1]]
    ctxs = [cp.Context(0), cp.Context(0)]
    bs = []
    for c, batch in zip(ctxs, batches):
        c.models_clear()
        c.models_create([(cp.NANOPORE_TRANSITIONS, m, gx, gy) for (m, gx, gy) in batch["models"]])
        bs.append(cp.Batch(c, make_items(batch, (1, 1)), batch["x_chars"], batch["events"], batch["anchors"], bp,
                           cp.MODE_EXPECTATIONS, cp.KERNEL_AUTO, FUSED))
        assert_wide(bs[-1].info(), 8, 1)
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


PERSISTENT = dict(seed=47, n=4, lX=400, lY=820, every=200, e=160)


def persistent_batch():
    p = PERSISTENT
    return synth.make_batch(p["seed"], p["n"], p["lX"], p["lY"], anchor_every=p["every"]), band_params(0.01, 150, 20, p["e"])


def test_persistent_batch_is_wide_on_the_oracle():
    """(CPU) both halves of the reads, as PersistentEStep deals them to two contexts, have a widest band of a wide build"""
    batch, _ = persistent_batch()
    for k in range(2):
        part = dict(batch, items=batch["items"][k::2])
        assert build_of(widest_band(part, PERSISTENT["e"])) in (6, 8)


@pytest.mark.gpu
def test_persistent_e_step_after_a_model_change(monkeypatch):
    """em.PersistentEStep over two contexts picks the workgroup kernels; the two variables make its wide batches fused"""
    monkeypatch.setenv("CPECAN_WIDE_BANDS", "1")
    monkeypatch.setenv("CPECAN_EXPECT_FUSED_WIDE", "1")
    one, ctx3, ctx4 = cp.Context(0), cp.Context(0), cp.Context(0)
    batch, bp = persistent_batch()
    reads = list(range(len(batch["items"])))
    gap0 = batch["models"][0][1]
    got = dist_em.gpu_e_step(cp, one, batch, bp, reads, cp.NANOPORE_TRANSITIONS, gap0)
    keep = dist_em.PersistentEStep(cp, [ctx3, ctx4], batch, bp, reads, cp.NANOPORE_TRANSITIONS, gap0)
    for _, b in keep.batches:
        info = b.info()
        assert info["family"] == "workgroup" and info["waves_per_workgroup"] in (6, 8), info
        assert info["fused_expectations"] == 1, info
    assert np.allclose(keep(cp.NANOPORE_TRANSITIONS, gap0), got, rtol=1e-12, atol=1e-300)
    t1, g1 = dist_em.m_step(got + np.r_[np.full(dist_em.EXP_LEN - 1, 1e-9), 0.0])
    again = keep(t1, g1)
    assert np.allclose(again, dist_em.gpu_e_step(cp, one, batch, bp, reads, t1, g1), rtol=1e-12, atol=1e-300)
    assert again[-1] > got[-1]
    keep.close()
    for c in (one, ctx3, ctx4):
        c.close()


# --------------------------------------------------- 8. a short seeded fuzz ---------------------------------------------------


def fuzz_cases(per_build=4, seed=20261019):
    """seeded shapes with anchors every 150..400 k-mers, even expansions of 60..300, ragged ends, the three transition
    sets and reads of one length or of different ones; kept are the first `per_build` whose widest band (the oracle's
    band table, on the CPU) is the six-wave build's and the first `per_build` of the eight-wave build's"""
    rng = np.random.default_rng(seed)
    kept = {6: [], 8: []}
    for k in range(200):
        lX = int(rng.integers(350, 800))
        c = dict(k=k, seed=8000 + k, n=int(rng.integers(1, 4)), lX=lX, lY=int(lX * rng.uniform(1.6, 2.3)),
                 every=int(rng.integers(150, 401)), e=2 * int(rng.integers(30, 151)), tb=int(rng.integers(1, 60)),
                 ragged=(int(rng.integers(0, 2)), int(rng.integers(0, 2))),
                 tset=str(rng.choice(["defaults", "switch", "trained"])), sigma=float(rng.choice([0.0, 0.4])))
        c["md"] = c["tb"] + 2 + int(rng.integers(0, 350))
        c["width"] = widest_band(fuzz_batch(c), c["e"])
        rows = build_of(c["width"])
        if rows is not None and len(kept[rows]) < per_build:
            kept[rows].append(c)
        if all(len(v) == per_build for v in kept.values()):
            break
    return kept[6] + kept[8]


def fuzz_batch(c):
    return synth.make_batch(c["seed"], c["n"], c["lX"], c["lY"], anchor_every=c["every"], length_sigma=c["sigma"])


FUZZ = fuzz_cases()


def test_the_fuzz_has_four_cases_on_each_build():
    """(CPU)"""
    assert [build_of(c["width"]) for c in FUZZ] == [6] * 4 + [8] * 4
    assert len(set(c["tset"] for c in FUZZ)) == 3 and len(set(c["sigma"] for c in FUZZ)) == 2


@pytest.mark.gpu
@pytest.mark.parametrize("case", FUZZ, ids=lambda c: "f%d-x%d" % (build_of(c["width"]), c["seed"]))
def test_random_wide_fused_expectations(ctx, case, request):
    t, gx = (SWITCH, None) if case["tset"] == "switch" else (cp.NANOPORE_TRANSITIONS, None)
    batch = fuzz_batch(case)
    if case["tset"] == "trained":
        t, gx = request.getfixturevalue("trained")
        batch = with_gap_x(batch, gx)
    bp = band_params(0.01, case["md"], case["tb"], case["e"])
    ref_items, ref = oracle_expectations(batch, bp, case["ragged"], t)
    res, info, got = run(ctx, batch, bp, ragged=case["ragged"], t=t)
    assert info["max_band_width"] == case["width"]
    assert_wide(info, build_of(case["width"]), 1)
    assert_same_totals(res, ref_items)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert_expectations_match(g, r, k)
        assert g[-1] < 0
        assert_gap_x_invariant(g, k)

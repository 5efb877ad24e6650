"""Seeded random sweep of the strawMan Baum-Welch E-step against the oracle, on every path a batch can take: the
wave kernels' fused sums (the default: expectations summed per refresh segment inside the sweep back, scaled from the
forward kernel's estimate), the same with windows forced down the re-sweep against the exact totals (all of them, or
every other one so that one launch has both), the wave kernels' ring of backward cells (CPECAN_EXPECT_FUSED=0), the
workgroup family and, where the band is wider than 248 k-mers, the general kernel.  Also: the band widths at the
edges of the wave builds, non-ACGT bytes in a read, and degenerate items inside an expectation batch.

The bars are the suite's: totals bit-identical, transitions and k-mer gap sums to rtol 1e-9 (atol 1e-12), the
likelihood to rtol 1e-12, fused against the ring to rtol 1e-11, and where the oracle has non-finite entries the device
has the same ones.  One bar needs no oracle: every gap-X term enters one transition (M->X, X->X or Y->X) and one
k-mer bin, so for reads of ACGT only the 4096 bins sum to T[1] + T[4] + T[7] (to rtol 1e-12) -- a dropped or doubled
per-slot record shows there even where the per-bin tolerance would let it through."""
import contextlib
import os

import numpy as np
import pytest

import pyoracle as o
import synth
from harness import (assert_same_posterior, band_params, cp, run_gpu, run_oracle_item, trained_transitions,
                     with_gap_switch, with_gap_x)

# CPECAN_FUZZ_SCALE=N runs N times as many cases (the first ones are the default run's)
SCALE = max(1, int(os.environ.get("CPECAN_FUZZ_SCALE", "1")))

SWITCH = with_gap_switch(cp.NANOPORE_TRANSITIONS, 0.05)
GAP_X = (1, 4, 7)  # M->X, X->X, Y->X among the nine transitions


@pytest.fixture(scope="module")
def ctx():
    c = cp.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def trained(ctx):
    return trained_transitions(ctx)


def cases(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        lX = int(rng.integers(20, 700))
        c = dict(k=k, seed=9000 + k, lX=lX, lY=max(8, int(lX * rng.uniform(0.8, 2.6))),
                 every=int(rng.choice([8, 20, 50, 120, 10 ** 6])),
                 e=int(rng.choice([0, 2, 10, 20, 40, 60, 100, 120, 180])),
                 tb=int(rng.integers(1, 60)), thr=float(rng.choice([0.5, 0.01, 1e-4])),
                 ragged=(int(rng.integers(0, 2)), int(rng.integers(0, 2))),
                 tset=str(rng.choice(["defaults", "switch", "trained"])),
                 n=int(rng.integers(2, 4)), distinct=k % 2 == 0,  # half one model per read, half one shared model
                 sigma=float(rng.choice([0.0, 0.0, 0.3])))         # some batches of reads of different lengths
        c["md"] = c["tb"] + 2 + int(rng.integers(0, 350))  # traceBackDiagonals + 1 < minDiagsBetweenTraceBack
        out.append(c)
    return out


CASES = cases(40 * SCALE, 20261015)


def case_id(c):
    return "x%d" % c["seed"]


def case_batch(c, gx=None):
    batch = synth.make_batch(c["seed"], c["n"], c["lX"], c["lY"], anchor_every=c["every"],
                             distinct_models=c["distinct"], length_sigma=c["sigma"])
    return with_gap_x(batch, gx)


def expectation_vector(hmm):
    return np.concatenate([np.array(hmm.transitions[:]), np.array(hmm.kmerGap[:]), [hmm.likelihood]])


def oracle_expectations(batch, bp, ragged, t=None):
    """(per-item oracle results, per-model expectation vectors [9 transitions | 4096 gap-X bins | likelihood])"""
    hmms = [o.OrcExpectations() for _ in batch["models"]]
    res = [run_oracle_item(batch, i, bp, ragged, transitions=t, expectations=hmms[it["model"]])
           for i, it in enumerate(batch["items"])]
    return res, [expectation_vector(h) for h in hmms]


@contextlib.contextmanager
def env(**kw):
    """the C-ABI's knobs, read when a batch is created: None unsets"""
    keep = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# how each path is asked for: (batch flags, CPECAN_EXPECT_FUSED, CPECAN_EXPECT_RESWEEP)
VARIANTS = dict(fused=(0, None, None), ring=(0, "0", None), workgroup=(cp.FLAG_WORKGROUP_KERNELS, None, None),
                resweep=(0, None, "1"), half=(0, None, "2"))


def run_expectations(ctx, batch, bp, ragged, variant, transitions=None, model_transitions=None):
    """(per-item results, info(), per-model expectation vectors) of one expectation batch on one path"""
    flags, fused, resweep = VARIANTS[variant]
    with env(CPECAN_EXPECT_FUSED=fused, CPECAN_EXPECT_RESWEEP=resweep):
        res, b = run_gpu(ctx, batch, bp, mode=cp.MODE_EXPECTATIONS, kernel=cp.KERNEL_AUTO, flags=flags, ragged=ragged,
                         transitions=transitions, model_transitions=model_transitions)
    info = b.info()
    got = [b.expectations(k) for k in range(len(batch["models"]))]
    b.close()
    return res, info, got


def assert_path(info, variant):
    """the batch ran where `variant` sends it: bands up to 248 k-mers on the systolic kernels (the wave family at the
    fewest cells per lane from 2), wider ones on the general kernel"""
    w = info["max_band_width"]
    if w > 248:
        assert info["kernel"] == "general" and info["fused_expectations"] == 0, info
        return
    assert info["kernel"] == "systolic", info
    if variant == "workgroup":
        assert info["family"] == "workgroup" and info["fused_expectations"] == 0, info
        return
    assert info["family"] == "wave" and info["cells_per_lane"] == 2 + (w > 120) + (w > 184), info
    assert info["fused_expectations"] == (0 if variant == "ring" else 1), info


def assert_same_totals(res, ref, what=""):
    for i, (g, r) in enumerate(zip(res, ref)):
        assert np.array_equal(g["totals_xay"], r["totals_xay"]), (what, i)
        assert np.array_equal(np.asarray(g["totals"]).view(np.uint64), np.asarray(r["totals"]).view(np.uint64)), \
            (what, i)


def assert_expectations_match(got, ref, what=""):
    """one model's vector against the oracle's: the same non-finite entries (NaN where it has NaN, the same
    infinities), the finite transitions and bins to rtol 1e-9 / atol 1e-12, a finite likelihood to rtol 1e-12"""
    got, ref = np.asarray(got), np.asarray(ref)
    bad = ~np.isfinite(ref)
    assert np.array_equal(~np.isfinite(got), bad), (what, np.flatnonzero(~np.isfinite(got) != bad)[:20])
    assert np.array_equal(got[bad], ref[bad], equal_nan=True), what
    ok = ~bad[:-1]
    assert np.allclose(got[:-1][ok], ref[:-1][ok], rtol=1e-9, atol=1e-12), \
        (what, np.flatnonzero(~np.isclose(got[:-1], ref[:-1], rtol=1e-9, atol=1e-12) & ok)[:20])
    if not bad[-1]:
        assert np.isclose(got[-1], ref[-1], rtol=1e-12, atol=0), (what, got[-1], ref[-1])


def assert_gap_x_invariant(v, what=""):
    """the 4096 gap-X bins sum to the three gap-X transitions (reads of ACGT only: a gap-X term of a k-mer that is not
    one counts in the transitions and in no bin)"""
    v = np.asarray(v)
    assert np.isclose(v[9:9 + 4096].sum(), v[list(GAP_X)].sum(), rtol=1e-12, atol=0), \
        (what, v[9:9 + 4096].sum(), v[list(GAP_X)].sum())


def transitions_of(c, trained=None):
    """(transitions, gap-X table or None) of a case's transition set"""
    if c["tset"] == "switch":
        return SWITCH, None
    if c["tset"] == "trained":
        return trained
    return cp.NANOPORE_TRANSITIONS, None


_ORACLE = {}
_FUSED = {}


def oracle_of(key, batch, bp, ragged, t):
    if key not in _ORACLE:
        _ORACLE[key] = oracle_expectations(batch, bp, ragged, t)
    return _ORACLE[key]


def variants_of(c):
    """every case on the fused path, the ring, the workgroup family and every other window re-swept; every fourth
    case with every window re-swept"""
    return ["fused", "ring", "workgroup", "half"] + (["resweep"] if c["k"] % 4 == 0 else [])


# ------------------------------------------------ 1. the sweep ------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("case,variant", [(c, v) for c in CASES for v in variants_of(c)],
                         ids=lambda x: case_id(x) if isinstance(x, dict) else x)
def test_random_expectations(ctx, case, variant, request):
    t, gx = transitions_of(case, request.getfixturevalue("trained") if case["tset"] == "trained" else None)
    batch = case_batch(case, gx)
    bp = band_params(case["thr"], case["md"], case["tb"], case["e"])
    ref_items, ref = oracle_of(case_id(case), batch, bp, case["ragged"], t)
    res, info, got = run_expectations(ctx, batch, bp, case["ragged"], variant, transitions=t)
    assert_path(info, variant)
    assert_same_totals(res, ref_items, variant)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert_expectations_match(g, r, (variant, k))
        assert g[-1] < 0
        assert_gap_x_invariant(g, (variant, k))
    if variant == "fused":
        _FUSED[case_id(case)] = got
    elif variant == "ring" and info["fused_expectations"] == 0 and info["kernel"] == "systolic":
        fused = _FUSED.get(case_id(case))
        if fused is None:
            fused = run_expectations(ctx, batch, bp, case["ragged"], "fused", transitions=t)[2]
        for f, r in zip(fused, got):  # the bar of test_fused_against_the_ring_of_backward_cells
            assert np.allclose(f[:-1], r[:-1], rtol=1e-11, atol=1e-300)
            assert np.isclose(f[-1], r[-1], rtol=1e-12)


def test_oracle_gap_x_invariant():
    """(CPU) the oracle keeps the invariant the sweep asserts on the device, on the sweep's first cases"""
    for c in CASES[:6]:
        if c["tset"] == "trained":  # (its transitions come from a GPU E-step)
            continue
        t, _ = transitions_of(c)
        batch = case_batch(c)
        bp = band_params(c["thr"], c["md"], c["tb"], c["e"])
        _, ref = oracle_of(case_id(c), batch, bp, c["ragged"], t)
        for k, v in enumerate(ref):
            assert np.all(np.isfinite(v)), (case_id(c), k)
            assert v[list(GAP_X)].sum() > 0
            assert_gap_x_invariant(v, (case_id(c), k))


# ------------------------------------ 2. the edges of the wave builds' bands ------------------------------------

# (widest band, seed, expansion): two 300 x 600 reads, anchors every 50 k-mers; the expansion has to be even
# (getPosteriorProbsWithBanding :880-884), and a seed's widths step by two with it
EDGES = [(120, 703, 68), (121, 700, 70), (184, 703, 132), (185, 700, 134), (248, 703, 196), (249, 700, 198)]


def edge_batch(seed):
    return synth.make_batch(seed, 2, 300, 600, anchor_every=50)


def edge_bp(e):
    return band_params(0.01, 100, 40, e)


def test_edge_band_widths_on_the_oracle():
    """(CPU) each expansion gives the widest band it is named for"""
    for width, seed, e in EDGES:
        batch = edge_batch(seed)
        w = 0
        for it in batch["items"]:
            an = batch["anchors"][it["anchor_offset"]: it["anchor_offset"] + it["n_anchors"]]
            L, R = o.band(an, it["lX"], it["lY"], e)
            w = max(w, int(((R - L) // 2 + 1).max()))
        assert w == width, (seed, e, w, width)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["fused", "ring", "posterior"])
@pytest.mark.parametrize("width,seed,e", EDGES, ids=["w%d" % w for w, _, _ in EDGES])
def test_band_edges(ctx, width, seed, e, variant):
    """bands that fill a build's slots exactly (120, 184, 248) and one k-mer past them"""
    batch = edge_batch(seed)
    bp = edge_bp(e)
    ragged = (1, 1)
    if variant == "posterior":
        res, b = run_gpu(ctx, batch, bp, kernel=cp.KERNEL_AUTO, ragged=ragged)
        assert b.info()["max_band_width"] == width
        b.close()
        for i in range(len(batch["items"])):
            assert_same_posterior(res[i], run_oracle_item(batch, i, bp, ragged), i)
        return
    ref_items, ref = oracle_of(("edge", seed, e), batch, bp, ragged, None)
    res, info, got = run_expectations(ctx, batch, bp, ragged, variant)
    assert info["max_band_width"] == width
    assert_path(info, variant)
    assert_same_totals(res, ref_items, variant)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert_expectations_match(g, r, (variant, k))
        assert_gap_x_invariant(g, (variant, k))


# ------------------------- 3. windows on the estimate path and on the re-sweep in one launch -------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(40, 120, 2), (100, 300, 3), (150, 300, 4)], ids=["l2", "l3", "l4"])
def test_half_the_windows_resweep(ctx, shape):
    """the shapes of test_fused_expectations_gpu.py (four reads, one model each, several windows) with
    CPECAN_EXPECT_RESWEEP=2: items 0 and 2 re-sweep their odd windows, items 1 and 3 their even ones"""
    expansion, md, cells = shape
    batch = synth.make_batch(11 + cells, 4, 700, 1400, anchor_every=50)
    bp = band_params(0.01, md, 40, expansion)
    ref_items, ref = oracle_of(("half", cells), batch, bp, (1, 1), None)
    res, info, got = run_expectations(ctx, batch, bp, (1, 1), "half")
    assert info["cells_per_lane"] == cells and info["fused_expectations"] == 1, info
    assert all(len(r["totals"]) > 20 for r in ref_items)  # several windows per item
    assert_same_totals(res, ref_items)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert_expectations_match(g, r, k)
        assert_gap_x_invariant(g, k)


# ------------------------------------------ 4. bytes other than ACGT ------------------------------------------

# (name, position in the read's lX + 5 characters, byte): the middle, inside the first k-mer, the last character, and
# a lowercase base (the reference's getKmerIndex knows upper case only)
NON_ACGT = [("middle", 150, "N"), ("first-kmer", 2, "N"), ("last", 304, "N"), ("lowercase", 200, "a")]


def non_acgt_batch(seed, n, lX, lY, bad, pos, ch, every=50):
    """n reads, one model each; read `bad` with byte `ch` at `pos`"""
    batch = synth.make_batch(seed, n, lX, lY, anchor_every=every)
    it = batch["items"][bad]
    x = bytearray(batch["x_chars"])
    x[it["x_offset"] + pos] = ord(ch)
    return dict(batch, x_chars=bytes(x))


def test_non_acgt_on_the_oracle():
    """(CPU) what the device has to reproduce: the totals of the windows over the byte are -inf, the bad read's
    model gets NaN transitions (all but X->Y, never taken) and NaN in some k-mer bins, a likelihood of -inf; the
    models of the other reads stay finite and keep the gap-X invariant"""
    bp = band_params(0.01, 100, 40, 40)
    for name, pos, ch in NON_ACGT:
        batch = non_acgt_batch(301, 3, 300, 600, 1, pos, ch)
        items, ref = oracle_expectations(batch, bp, (1, 1))
        tot = np.asarray(items[1]["totals"])
        assert np.any(tot == -np.inf) and not np.any(np.isnan(tot)), name
        v = ref[1]
        assert np.array_equal(np.flatnonzero(np.isnan(v[:9])), [0, 1, 2, 3, 4, 6, 7, 8]), name
        nb = int(np.isnan(v[9:9 + 4096]).sum())
        assert 0 < nb < 4096 and not np.any(np.isinf(v[9:9 + 4096])), (name, nb)
        assert v[-1] == -np.inf, name
        for k in (0, 2):
            assert np.all(np.isfinite(items[k]["totals"])) and np.all(np.isfinite(ref[k])), (name, k)
            assert_gap_x_invariant(ref[k], (name, k))


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["fused", "ring", "workgroup", "half"])
@pytest.mark.parametrize("name,pos,ch", NON_ACGT, ids=[n for n, _, _ in NON_ACGT])
def test_non_acgt_expectations(ctx, name, pos, ch, variant):
    batch = non_acgt_batch(301, 3, 300, 600, 1, pos, ch)
    bp = band_params(0.01, 100, 40, 40)
    ref_items, ref = oracle_of(("acgt", name), batch, bp, (1, 1), None)
    res, info, got = run_expectations(ctx, batch, bp, (1, 1), variant)
    assert_path(info, variant)
    assert_same_totals(res, ref_items, variant)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert_expectations_match(g, r, (variant, k))
        if k != 1:
            assert_gap_x_invariant(g, (variant, k))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["wave", "assembly", "workgroup"])
@pytest.mark.parametrize("name,pos,ch", NON_ACGT, ids=[n for n, _, _ in NON_ACGT])
def test_non_acgt_posteriors(ctx, name, pos, ch, shape):
    """the same bytes in posterior batches: the wave kernels, a batch shaped for the assembly sweeps, the workgroup
    family -- cells, totals (-inf included) and pairs identical to the oracle"""
    if shape == "assembly":
        batch = non_acgt_batch(82, 3, 700, 1400, 1, pos, ch)
        bp = band_params(0.01, 300, 40, 100)
    else:
        batch = non_acgt_batch(301, 3, 300, 600, 1, pos, ch)
        bp = band_params(0.01, 100, 40, 40)
    res, b = run_gpu(ctx, batch, bp, kernel=cp.KERNEL_AUTO,
                     flags=cp.FLAG_WORKGROUP_KERNELS if shape == "workgroup" else 0, ragged=(1, 1))
    info = b.info()
    b.close()
    assert info["kernel"] == "systolic" and info["family"] == ("workgroup" if shape == "workgroup" else "wave"), info
    if shape == "assembly":
        assert info["assembly_sweeps"] == 2, info
    for i in range(3):
        assert_same_posterior(res[i], run_oracle_item(batch, i, bp, (1, 1)), (name, i))


# ------------------------------------- 5. degenerate items in an expectation batch -------------------------------------

DEGENERATE = [(0, 0), (0, 5), (5, 0), (1, 1), (3, 4)]


def degenerate_batch():
    """two 300 x 600 reads, then items of DEGENERATE's shapes on the first read's bytes and events, each with a model of
    its own"""
    batch = synth.make_batch(302, 2, 300, 600, anchor_every=50)
    base, m0 = batch["items"][0], batch["models"][0]
    items, models = list(batch["items"]), list(batch["models"])
    for lX, lY in DEGENERATE:
        items.append(dict(base, lX=lX, lY=lY, n_anchors=0, model=len(models)))
        models.append(m0)
    return dict(batch, items=items, models=models)


RAGGED = [(0, 0), (1, 1), (1, 0), (0, 1)]


def test_degenerate_items_on_the_oracle():
    """(CPU) the oracle's answers for the degenerate items: 0 x 0 nothing at all; 0 x 5 one total of -inf and NaN in
    the two transitions into gap Y; 5 x 0 five gap-X terms, a finite likelihood; 1 x 1 and 3 x 4 finite"""
    bp = band_params(0.01, 100, 40, 40)
    for ragged in RAGGED:
        items, ref = oracle_expectations(degenerate_batch(), bp, ragged)
        v = dict(zip(DEGENERATE, ref[2:]))
        t = dict(zip(DEGENERATE, [r["totals"] for r in items[2:]]))
        assert len(t[(0, 0)]) == 0 and not np.any(v[(0, 0)])
        assert list(t[(0, 5)]) == [-np.inf] and v[(0, 5)][-1] == -np.inf
        assert np.array_equal(np.flatnonzero(np.isnan(v[(0, 5)])), [2, 8])
        assert np.count_nonzero(v[(0, 5)][:-1] == v[(0, 5)][:-1]) == 9 + 4096 - 2  # (NaN != NaN) the rest 0
        assert not np.any(v[(0, 5)][:9][[0, 1, 3, 4, 5, 6, 7]]) and not np.any(v[(0, 5)][9:-1])
        assert np.isclose(v[(5, 0)][list(GAP_X)].sum(), 5.0, rtol=1e-12) and np.count_nonzero(v[(5, 0)][9:-1]) == 5
        assert np.isfinite(v[(5, 0)][-1])
        for shape in ((5, 0), (1, 1), (3, 4)):
            assert np.all(np.isfinite(v[shape])) and np.all(np.isfinite(t[shape])), (ragged, shape)
            assert_gap_x_invariant(v[shape], (ragged, shape))
        if ragged == (1, 1):  # both ends free: the 1 x 1 item's mass enters the match state from gap X and gap Y
            assert v[(1, 1)][3] > 0 and v[(1, 1)][6] > 0 and v[(1, 1)][0] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["fused", "ring", "workgroup", "half"])
@pytest.mark.parametrize("ragged", RAGGED, ids=["r%d%d" % r for r in RAGGED])
def test_degenerate_items_expectations(ctx, ragged, variant):
    """totals and expectations per model equal the oracle's, NaN and -inf included (the in-band cell count of an
    empty item is the library's own: it is not compared, as in test_chained_batches_gpu.py)"""
    batch = degenerate_batch()
    bp = band_params(0.01, 100, 40, 40)
    ref_items, ref = oracle_of(("degenerate", ragged), batch, bp, ragged, None)
    res, info, got = run_expectations(ctx, batch, bp, ragged, variant)
    assert_path(info, variant)
    assert_same_totals(res, ref_items, variant)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert_expectations_match(g, r, (variant, k))
        if np.all(np.isfinite(r)):
            assert_gap_x_invariant(g, (variant, k))

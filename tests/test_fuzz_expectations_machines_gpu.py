"""Seeded random sweep of the Baum-Welch E-steps of the vanilla, HDP and 5-state DNA machines against the oracle, on
every path a batch of theirs can take, as test_fuzz_expectations_gpu.py does for the strawMan machine:

- vanilla: the wave builds v2, v3 (AUTO), cpecan_k_generalv (CPECAN_FLAG_GENERAL_KERNEL, and AUTO past 184 k-mers),
  a narrow band on the wider build (CPECAN_SYSTOLIC_ROWS=3);
- HDP: the wave builds h2, h3, h4, cpecan_k_generalh (the flag, and AUTO past 248 k-mers), a narrow band on h3 and h4
  (CPECAN_SYSTOLIC_ROWS), its assignments per read;
- DNA: one wave per alignment, a pair of waves, cpecan_k_general5 (the flag, and both wave forms past 192 cells).

Random window geometry, all four ragged-end pairs, three thresholds, several models in one batch with reads of
different lengths, a finite gap-Y to gap-X switch in the HDP E-step; then degenerate items inside an E-step batch,
bytes other than ACGT in a vanilla or DNA read (E-step and posterior decode), and a batch run twice.

The bars are the suite's: sums to rtol 1e-9 / atol 1e-12, a finite likelihood to rtol 1e-12, the same non-finite
entries as the oracle, the HDP assignments and their exponents bit-identical and in the reference's order per read,
every item's totals bit-identical to the oracle's posterior run of that item.

A vanilla batch that meets a k-mer that is none -- a byte outside ACGT, or the k-mer past the end of an item of no or
one k-mer -- runs on cpecan_k_generalv whatever is asked for: the reference answers NaN there and NaN spreads through
its logAdd, which the general kernel reproduces and the register-resident kernels' branch-free logAdd does not (see
DESIGN.md).  The tests of such batches assert that route.

HDP reads with a character outside the alphabet are left out: the reference exits there (see
test_hdp_workgroup_gpu.test_a_column_that_is_no_kmer_scores_minus_infinity and DESIGN.md).  The DNA E-step with a base
outside ACGT is defined on the oracle as in the reference (cell_updateExpectations adds the transition and leaves
the emission bin out, impl/pairwiseAligner.c:421), so it is compared too.

CPECAN_FUZZ_SCALE=N runs N times as many sweep cases (the first ones are the default run's)."""
import os

import numpy as np
import pytest

import pyoracle as o
import synth
from harness import (assert_same_pairs, band_params, batch_results, cp, hdp_batch, make_items, orc_params,
                     trained_transitions, with_gap_switch)
from test_band_edges_machines_gpu import cached, read_of
from test_dna5_gpu import KERNEL_FORMS, KERNEL_IDS, evolve, pick_form
from test_fuzz_expectations_gpu import (DEGENERATE, NON_ACGT, RAGGED, assert_expectations_match, degenerate_batch, env,
                                        non_acgt_batch)
from test_hdp_workgroup_gpu import reads_batch
from test_vanilla_gpu import skip_bins
from test_vanilla_workgroup_gpu import SHAPES as VANILLA_WIDE_SHAPES
from test_vanilla_workgroup_gpu import build_of, shape_batch, vanilla_models

SCALE = max(1, int(os.environ.get("CPECAN_FUZZ_SCALE", "1")))
N_CASES = 16  # per machine at the default scale

SWITCH = with_gap_switch(cp.NANOPORE_TRANSITIONS, 0.05)
EVERY = [8, 20, 50, 120, 10 ** 6]  # (the last: no anchors)
NO_ANCHORS = np.zeros((0, 2), np.int64)
# the widest band of each wave build: v2 / h2, v3 / h3, h4 (k-mers); one, two, three cells per lane of wave5 (cells)
W2, W3, W4 = 120, 184, 248
D1, D2, D3 = 64, 128, 192


@pytest.fixture(scope="module")
def ctx():
    c = cp.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def trained(ctx):
    return trained_transitions(ctx)[0]


@pytest.fixture(scope="module")
def nhdp(golden_dir):
    return o.load_nhdp(os.path.join(golden_dir, "testTemplate.nhdp"))


def geometry(rng, c, expansions):
    """the draws every machine's cases share: anchors, expansion, window geometry, ragged ends, reads, their lengths"""
    c.update(every=int(rng.choice(EVERY)), e=int(rng.choice(expansions)), tb=int(rng.integers(1, 60)),
             ragged=(int(rng.integers(0, 2)), int(rng.integers(0, 2))), n=int(rng.integers(2, 4)),
             sigma=float(rng.choice([0.0, 0.3])), two=c["k"] % 2 == 0)
    c["md"] = c["tb"] + 2 + int(rng.integers(0, 350))  # traceBackDiagonals + 1 < minDiagsBetweenTraceBack
    return c


def case_id(c):
    return "%s%d" % (c["machine"], c["seed"])


def ids(x):
    return case_id(x) if isinstance(x, dict) else str(x)


def bp_of(c):
    return band_params(c["thr"], c["md"], c["tb"], c["e"])


def widest(batch_items, e):
    """the widest band of (anchors, lX, lY) triples on the oracle's band table"""
    return max(int(((R - L) // 2 + 1).max()) for an, lX, lY in batch_items for L, R in [o.band(an, lX, lY, e)])


def signal_width(batch, e):
    return widest([(read_of(batch, it)[2], it["lX"], it["lY"]) for it in batch["items"]], e)


def assert_wave_path(info, variant, width, last):
    """a vanilla (last = W3) or HDP (last = W4) E-step ran where `variant` sends it: 'general' on the general kernel;
    'auto' on the wave build of the fewest cells per lane that holds the band, past the last build on the general
    kernel; 'rows3', 'rows4' on the build of at least that many cells per lane"""
    assert info["max_band_width"] == width, (info, width)
    if variant == "general" or width > last:
        assert info["kernel"] == "general", info
        return
    rows = max(2 + (width > W2) + (width > W3), int(variant[4:]) if variant.startswith("rows") else 2)
    assert info["kernel"] == "systolic" and info["family"] == "wave" and info["cells_per_lane"] == rows, (info, rows)


def rows_env(variant):
    return variant[4:] if variant.startswith("rows") else None


def posterior_of(model, x, lX, y, anchors, p, ragged):
    """the oracle's posterior run of one item, its pairs in emission order"""
    r = o.aligned_pairs_using_anchors(model, x, lX, y, anchors, p, ragged[0], ragged[1])
    r["triples"], r["logp"] = r["triples"][::-1], r["logp"][::-1]
    return r


def same_doubles(g, r):
    """bit for bit, but a NaN for a NaN whatever its sign and payload (the host's 0 * inf is 0xFFF8..., the device's
    0x7FF8...: neither the reference nor IEEE 754 gives a NaN's sign a meaning)"""
    g, r = np.asarray(g, np.float64), np.asarray(r, np.float64)
    nan = np.isnan(r)
    return g.shape == r.shape and np.array_equal(np.isnan(g), nan) and \
        np.array_equal(g[~nan].view(np.uint64), r[~nan].view(np.uint64))


def assert_same_totals(res, ref, what=""):
    """test_fuzz_expectations_gpu.assert_same_totals with same_doubles"""
    for i, (g, r) in enumerate(zip(res, ref)):
        assert np.array_equal(g["totals_xay"], r["totals_xay"]), (what, i)
        assert same_doubles(g["totals"], r["totals"]), (what, i, g["totals"], r["totals"])


def assert_same_posterior(g, r, what=""):
    """harness.assert_same_posterior with same_doubles for the totals"""
    assert g["cells"] == r["cells"], (what, g["cells"], r["cells"])
    assert_same_totals([g], [r], what)
    assert_same_pairs(g, r)


def assert_sane(ref, what):
    """what the sweep asks of each of a case's oracle vectors: finite, a negative likelihood, a third of the sums in
    use"""
    for k, v in enumerate(ref):
        assert np.all(np.isfinite(v)) and v[-1] < 0, (what, k)
        assert 3 * np.count_nonzero(v[:-1]) >= len(v) - 1, (what, k, np.count_nonzero(v[:-1]))


# ------------------------------------------------------ vanilla ------------------------------------------------------


def vanilla_cases(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        lX = int(rng.integers(20, 601))
        c = dict(machine="v", k=k, seed=9100 + k, lX=lX, lY=max(8, int(lX * rng.uniform(0.8, 2.6))),
                 thr=float(rng.choice([0.5, 0.01, 1e-4])))
        out.append(geometry(rng, c, [0, 2, 10, 20, 40, 60, 100, 120, 180]))
    return out


VANILLA = vanilla_cases(N_CASES * SCALE, 1)


def vanilla_batch(c):
    """(batch, models): one VanillaModel per read where c['two'] (alternating strand factors, skip bins of its own),
    else one shared"""
    batch = synth.make_batch(c["seed"], c["n"], c["lX"], c["lY"], anchor_every=c["every"], distinct_models=c["two"],
                             length_sigma=c["sigma"])
    return batch, vanilla_models(batch)


def vanilla_oracle(batch, models, bp, ragged):
    """per-model vectors [30 beta | 30 alpha | likelihood] of the oracle's E-step"""
    p = orc_params(bp, split=1 << 60)
    hmms = [o.OrcExpectationsV() for _ in models]
    for it in batch["items"]:
        x, ev, an = read_of(batch, it)
        o.expectations_v_using_anchors(models[it["model"]], x, it["lX"], ev, an, p, hmms[it["model"]], ragged[0],
                                       ragged[1])
    return [h.as_array() for h in hmms]


def vanilla_posteriors(batch, models, bp, ragged):
    p = orc_params(bp, split=1 << 60)
    return [posterior_of(models[it["model"]], x, it["lX"], ev, an, p, ragged)
            for it in batch["items"] for x, ev, an in [read_of(batch, it)]]


def run_vanilla(ctx, batch, models, bp, ragged, variant, flags=cp.FLAG_EXPECTATIONS, twice=False):
    """(per-item results, info(), per-model vectors) of one vanilla batch; twice: of its first and of its second run"""
    ctx.models_clear()
    mids = ctx.modelsv_create([(m.scalars, m.match, m.skip, m.gap_y) for m in models])
    with env(CPECAN_SYSTOLIC_ROWS=rows_env(variant)):
        b = cp.Batch(ctx, make_items(batch, ragged), batch["x_chars"], batch["events"], batch["anchors"], bp,
                     flags=flags | (cp.FLAG_GENERAL_KERNEL if variant == "general" else 0), vanilla=True)
    info = b.info()
    runs = []
    for _ in range(2 if twice else 1):
        b.run()
        b.sync()
        runs.append((batch_results(b), info,
                     [b.expectations(m) for m in mids] if flags & cp.FLAG_EXPECTATIONS else None))
    b.close()
    return runs if twice else runs[0]


def check_vanilla(key, res, got, batch, models, bp, ragged, what):
    assert_same_totals(res, cached(key + ("post",), lambda: vanilla_posteriors(batch, models, bp, ragged)), what)
    ref = cached(key + ("e",), lambda: vanilla_oracle(batch, models, bp, ragged))
    for k, (g, r) in enumerate(zip(got, ref)):
        assert_expectations_match(g, r, (what, k))
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("case,variant", [(c, v) for c in VANILLA for v in ["auto", "general"] +
                                          (["rows3"] if c["k"] % 4 == 0 else [])], ids=ids)
def test_random_vanilla_expectations(ctx, case, variant):
    batch, models = vanilla_batch(case)
    bp = bp_of(case)
    res, info, got = run_vanilla(ctx, batch, models, bp, case["ragged"], variant)
    assert_wave_path(info, variant, signal_width(batch, case["e"]), W3)
    ref = check_vanilla((case_id(case),), res, got, batch, models, bp, case["ragged"], variant)
    assert_sane(ref, case_id(case))


# -------------------------------------------------------- HDP --------------------------------------------------------

TSETS = ["defaults", "switch", "trained"]


def hdp_cases(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        c = dict(machine="h", k=k, seed=9300 + k, lX=int(rng.integers(20, 601)),
                 thr=float(rng.choice([0.5, 0.05, 0.01])), tset=int(rng.integers(0, 3)))
        geometry(rng, c, [0, 2, 10, 20, 40, 60, 100, 120, 180])
        f = np.clip(rng.lognormal(0.0, c["sigma"], c["n"]), 0.25, 1.5) if c["sigma"] > 0 else np.ones(c["n"])
        c["ls"] = [min(600, max(12, int(c["lX"] * v))) for v in f]
        # the transition sets of the batch's models: one, or two different ones with the reads dealt between them
        c["tsets"] = [TSETS[c["tset"]]] + ([TSETS[(c["tset"] + 1 + k // 2 % 2) % 3]] if c["two"] else [])
        out.append(c)
    return out


HDP = hdp_cases(N_CASES * SCALE, 9)


def hdp_case_batch(c, nhdp):
    batch = reads_batch(c["seed"], c["ls"], min(c["every"], 10 ** 5), nhdp)
    items = [dict(it, model=i % len(c["tsets"]), **(dict(n_anchors=0) if c["every"] == 10 ** 6 else {}))
             for i, it in enumerate(batch["items"])]
    return dict(batch, items=items)


def transitions_named(name, trained=None):
    return {"defaults": cp.NANOPORE_TRANSITIONS, "switch": SWITCH, "trained": trained}[name]


def hdp_oracle(batch, models, bp, ragged, read_of=read_of):
    """(per read: the oracle's E-step of that read alone; per model: [9 transitions | likelihood] summed over its
    reads)"""
    p = orc_params(bp, split=1 << 60)
    reads, vec = [], [np.zeros(10) for _ in models]
    for it in batch["items"]:
        x, ev, an = read_of(batch, it)
        r = o.expectations_h_using_anchors(models[it["model"]], [(x, it["lX"], ev, an)], p, bp.threshold, ragged[0],
                                           ragged[1])
        reads.append(r)
        vec[it["model"]] = vec[it["model"]] + np.concatenate([r["transitions"], [r["likelihood"]]])
    return reads, vec


def hdp_posteriors(batch, models, bp, ragged, read_of=read_of):
    p = orc_params(bp, split=1 << 60)
    return [posterior_of(models[it["model"]], x, it["lX"], ev, an, p, ragged)
            for it in batch["items"] for x, ev, an in [read_of(batch, it)]]


def run_hdp(ctx, nhdp, batch, ts, bp, ragged, variant, twice=False):
    """(per-item results: the assignments as pairs; info(); per-model vectors) of one HDP E-step batch"""
    ctx.models_clear()
    mids = ctx.modelsh_create([(t, nhdp["alphabet"], nhdp["grid"], nhdp["y"], nhdp["slope"], nhdp["kmer_row"])
                               for t in ts])
    with env(CPECAN_SYSTOLIC_ROWS=rows_env(variant)):
        b = cp.Batch(ctx, make_items(batch, ragged), batch["x_chars"], batch["events"], batch["anchors"], bp,
                     flags=cp.FLAG_EXPECTATIONS | (cp.FLAG_GENERAL_KERNEL if variant == "general" else 0), hdp=True)
    info = b.info()
    runs = []
    for _ in range(2 if twice else 1):
        b.run()
        b.sync()
        runs.append((batch_results(b), info, [b.expectations(m) for m in mids]))
    b.close()
    return runs if twice else runs[0]


def assert_same_assignments(res, reads, what):
    """per read: the assignments and their exponents bit-identical and in the reference's order (the oracle run on
    that read alone); the batch's count the summed oracle's"""
    for i, (g, r) in enumerate(zip(res, reads)):
        assert np.array_equal(g["triples"], r["assign"]), (what, i, len(g["triples"]), len(r["assign"]))
        assert np.array_equal(np.asarray(g["logp"]).view(np.uint64), np.asarray(r["logp"]).view(np.uint64)), (what, i)
    assert sum(len(g["triples"]) for g in res) == sum(len(r["assign"]) for r in reads), what


def check_hdp(key, res, got, batch, models, bp, ragged, what, read_of=read_of):
    assert_same_totals(res, cached(key + ("post",), lambda: hdp_posteriors(batch, models, bp, ragged, read_of)), what)
    reads, ref = cached(key + ("e",), lambda: hdp_oracle(batch, models, bp, ragged, read_of))
    for k, (g, r) in enumerate(zip(got, ref)):
        assert_expectations_match(g, r, (what, k))
    assert_same_assignments(res, reads, what)
    return reads, ref


@pytest.mark.gpu
@pytest.mark.parametrize("case,variant", [(c, v) for c in HDP for v in ["auto", "general"] +
                                          (["rows3", "rows4"] if c["k"] % 4 == 0 else [])], ids=ids)
def test_random_hdp_expectations_and_assignments(ctx, nhdp, case, variant, request):
    tr = request.getfixturevalue("trained") if "trained" in case["tsets"] else None
    ts = [transitions_named(name, tr) for name in case["tsets"]]
    batch = hdp_case_batch(case, nhdp)
    bp = bp_of(case)
    res, info, got = run_hdp(ctx, nhdp, batch, ts, bp, case["ragged"], variant)
    assert_wave_path(info, variant, signal_width(batch, case["e"]), W4)
    models = [o.HdpModel(nhdp, transitions=t) for t in ts]
    _, ref = check_hdp((case_id(case),), res, got, batch, models, bp, case["ragged"], variant)
    assert_sane(ref, case_id(case))


# -------------------------------------------------------- DNA --------------------------------------------------------


def dna_cases(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        c = dict(machine="d", k=k, seed=9500 + k, length=int(rng.integers(20, 701)), thr=0.01)
        out.append(geometry(rng, c, [0, 2, 10, 20, 50, 84, 120]))
    return out


DNA = dna_cases(N_CASES * SCALE, 1)


def dna_models(two, k=0):
    """the tables as uploaded, (transitions[17], match[16], gx[4], gy[4]) per model: the reference's defaults and,
    where `two` (the cases of even k), a second model whose emission tables (k % 4 == 0) or transitions
    (k % 4 == 2) differ"""
    d = o.Sm5Model()
    first = (list(d.c.t), d.match.copy(), d.gx.copy(), d.gy.copy())
    if not two:
        return [first]
    if k % 4 == 0:
        ts, tv = 0.04, 0.025  # a base pair matches with probability 0.64, 4 transitions, 8 transversions
        m = np.log([[0.16, tv, ts, tv], [tv, 0.16, tv, ts], [ts, tv, 0.16, tv], [tv, ts, tv, 0.16]]).reshape(-1)
        return [first, (first[0], m, np.log([0.3, 0.2, 0.2, 0.3]), np.log([0.2, 0.3, 0.3, 0.2]))]
    t = np.array(first[0]) + np.log(np.where(np.arange(17) % 2 == 0, 0.9, 1.1))
    return [first, ([float(v) for v in t], first[1], first[2], first[3])]


def dna_seqs(c):
    rng = np.random.default_rng(c["seed"])
    seqs = []
    for _ in range(c["n"]):
        f = float(np.clip(rng.lognormal(0.0, c["sigma"]), 0.25, 1.5)) if c["sigma"] > 0 else 1.0
        x, y, pairs = evolve(rng, min(700, max(12, int(c["length"] * f))))
        seqs.append((x, y, pairs[3::c["every"]] if c["every"] < 10 ** 6 else NO_ANCHORS))
    return seqs


def dna_width(seqs, e):
    return widest([(a, len(x), len(y)) for x, y, a in seqs], e)


def dna_oracle(seqs, tables, model_of, bp, raggeds):
    """per-model vectors [25 transitions | 80 emission bins | likelihood]"""
    p = orc_params(bp, split=1 << 60)
    models = [o.Sm5Model(*t) for t in tables]
    hmms = [o.OrcExpectations5() for _ in tables]
    for (x, y, a), k, rg in zip(seqs, model_of, raggeds):
        o.expectations5_using_anchors(models[k], x, len(x), y, a, p, hmms[k], rg[0], rg[1])
    return [h.as_array() for h in hmms]


def dna_posteriors(seqs, tables, model_of, bp, raggeds):
    p = orc_params(bp, split=1 << 60)
    models = [o.Sm5Model(*t) for t in tables]
    return [posterior_of(models[k], x, len(x), y, a, p, rg) for (x, y, a), k, rg in zip(seqs, model_of, raggeds)]


def run_dna(ctx, seqs, tables, model_of, bp, raggeds, flags, twice=False, pad=""):
    """(per-item results, info(), per-model vectors or None) of one DNA batch; pad: characters past the last sequence"""
    ctx.models_clear()
    mids = ctx.models5_create(tables)
    xs, ys, an = "", "", []
    items = np.zeros(len(seqs), cp.ITEM_DTYPE)
    for i, ((x, y, a), k, rg) in enumerate(zip(seqs, model_of, raggeds)):
        items[i] = (len(xs), len(x), len(ys), len(y), sum(len(q) for q in an), len(a), mids[k], rg[0], rg[1], 0)
        xs += x
        ys += y
        an.append(np.asarray(a, np.int64).reshape(-1, 2))
    b = cp.Batch(ctx, items, xs + pad, None, np.concatenate(an), bp, flags=flags, y_chars=ys + pad)
    info = b.info()
    runs = []
    for _ in range(2 if twice else 1):
        b.run()
        b.sync()
        runs.append((batch_results(b), info,
                     [b.expectations(m) for m in mids] if flags & cp.FLAG_EXPECTATIONS else None))
    b.close()
    return runs if twice else runs[0]


def assert_dna_path(info, width, flags):
    """bands of up to 192 cells on the wave5 kernels (one, two, three cells per lane by the width) unless the general
    kernel is asked for; wider ones on cpecan_k_general5"""
    assert info["kernel"] == "general" and info["max_band_width"] == width, (info, width)
    assert (info.get("family") == "wave (5-state)") == (width <= D3 and not flags & cp.FLAG_GENERAL_KERNEL), info


@pytest.mark.gpu
@pytest.mark.parametrize("form", KERNEL_FORMS, ids=KERNEL_IDS)
@pytest.mark.parametrize("case", DNA, ids=ids)
def test_random_dna_expectations(ctx, case, form, monkeypatch):
    flags = pick_form(monkeypatch, form) | cp.FLAG_EXPECTATIONS
    seqs = dna_seqs(case)
    tables = dna_models(case["two"], case["k"])
    model_of = [i % len(tables) for i in range(len(seqs))]
    raggeds = [case["ragged"]] * len(seqs)
    bp = bp_of(case)
    res, info, got = run_dna(ctx, seqs, tables, model_of, bp, raggeds, flags)
    assert_dna_path(info, dna_width(seqs, case["e"]), flags)
    key = (case_id(case),)
    assert_same_totals(res, cached(key + ("post",), lambda: dna_posteriors(seqs, tables, model_of, bp, raggeds)), form)
    ref = cached(key + ("e",), lambda: dna_oracle(seqs, tables, model_of, bp, raggeds))
    for k, (g, r) in enumerate(zip(got, ref)):
        assert_expectations_match(g, r, (form, k))
    assert_sane(ref, case_id(case))


# ------------------------------------------- the conditions of the sweep -------------------------------------------


def test_sweep_conditions_on_the_oracle(nhdp):
    """(CPU) of each machine's default cases at least three land on each wave build, at least two past the widest one
    (on the general kernel by AUTO), all four ragged pairs occur, the forced builds get a band narrower than their
    own; and the oracle's vectors are finite with a negative likelihood and a third of their sums in use.  (An HDP
    case with the trained transition set is held to the last part on the GPU only: the set comes from a GPU E-step.)"""
    def classes(widths, bounds):
        return [sum(lo < w <= hi for w in widths) for lo, hi in zip([0] + bounds, bounds + [10 ** 9])]

    batches = [vanilla_batch(c) for c in VANILLA[:N_CASES]]
    wv = [signal_width(b, c["e"]) for (b, _), c in zip(batches, VANILLA)]
    assert min(classes(wv, [W2, W3])[:2]) >= 3 and classes(wv, [W2, W3])[2] >= 2, wv
    assert sum(w <= W2 for w in wv[::4]) >= 2, wv[::4]
    for (b, models), c in zip(batches, VANILLA):
        assert_sane(cached((case_id(c), "e"), lambda: vanilla_oracle(b, models, bp_of(c), c["ragged"])), case_id(c))

    hb = [hdp_case_batch(c, nhdp) for c in HDP[:N_CASES]]
    wh = [signal_width(b, c["e"]) for b, c in zip(hb, HDP)]
    assert min(classes(wh, [W2, W3, W4])[:3]) >= 3 and classes(wh, [W2, W3, W4])[3] >= 2, wh
    assert sum(w <= W2 for w in wh[::4]) >= 1 and sum(w <= W3 for w in wh[::4]) >= 2, wh[::4]
    assert {t for c in HDP[:N_CASES] for t in c["tsets"]} == set(TSETS)
    for b, c in zip(hb, HDP):
        if "trained" not in c["tsets"]:
            models = [o.HdpModel(nhdp, transitions=transitions_named(t)) for t in c["tsets"]]
            _, ref = cached((case_id(c), "e"), lambda: hdp_oracle(b, models, bp_of(c), c["ragged"]))
            assert_sane(ref, case_id(c))

    seqs = [dna_seqs(c) for c in DNA[:N_CASES]]
    wd = [dna_width(s, c["e"]) for s, c in zip(seqs, DNA)]
    assert min(classes(wd, [D1, D2, D3])[:3]) >= 3 and classes(wd, [D1, D2, D3])[3] >= 2, wd
    union = np.zeros(80, bool)
    for s, c in zip(seqs, DNA):
        tables = dna_models(c["two"], c["k"])
        model_of = [i % len(tables) for i in range(len(s))]
        ref = cached((case_id(c), "e"), lambda: dna_oracle(s, tables, model_of, bp_of(c), [c["ragged"]] * len(s)))
        assert_sane(ref, case_id(c))
        union |= np.any([v[25:105] != 0 for v in ref], axis=0)
    assert np.count_nonzero(union) >= 60  # most emission bins are hit

    for cs in (VANILLA, HDP, DNA):
        assert {c["ragged"] for c in cs[:N_CASES]} == set(RAGGED)
        assert {c["sigma"] for c in cs[:N_CASES]} == {0.0, 0.3} and min(c["tb"] for c in cs[:N_CASES]) < 10


# ------------------------------------- 2. degenerate items in an E-step batch -------------------------------------

DEG_BP = (0.01, 100, 40, 40)


def vanilla_degenerate():
    """test_fuzz_expectations_gpu.degenerate_batch as a vanilla batch: the two reads' models with skip bins of their
    own, every degenerate item a model of its own with the first read's tables"""
    batch = degenerate_batch()
    return batch, [o.VanillaModel(m, skip_bins(k if k < 2 else 0), gy) for k, (m, _, gy) in enumerate(batch["models"])]


def test_vanilla_degenerate_items_on_the_oracle():
    """(CPU) what the device has to reproduce: 0 x 0 nothing at all; 0 x 5 zero sums and a NaN likelihood; 5 x 0 one or
    three skip bins and a finite likelihood; 1 x 1 three NaN, the likelihood among them; 3 x 4 finite"""
    batch, models = vanilla_degenerate()
    for ragged in RAGGED:
        ref = cached(("v-degenerate", ragged, "e"), lambda: vanilla_oracle(batch, models, band_params(*DEG_BP), ragged))
        v = dict(zip(DEGENERATE, ref[2:]))
        assert not np.any(v[(0, 0)])
        assert np.array_equal(np.flatnonzero(np.isnan(v[(0, 5)])), [60]) and not np.any(v[(0, 5)][:60])
        assert np.all(np.isfinite(v[(5, 0)])) and 2 <= np.count_nonzero(v[(5, 0)]) <= 3 and v[(5, 0)][60] < -50
        assert np.isnan(v[(1, 1)][60]) and np.count_nonzero(np.isnan(v[(1, 1)])) == 3
        assert np.all(np.isfinite(v[(3, 4)])) and v[(3, 4)][60] < 0
        for k in (0, 1):
            assert np.all(np.isfinite(ref[k])) and ref[k][60] < 0


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["auto", "general"])
@pytest.mark.parametrize("ragged", RAGGED, ids=["r%d%d" % r for r in RAGGED])
def test_vanilla_degenerate_items_expectations(ctx, ragged, variant):
    """the oracle's answers, NaN included (a NaN for a NaN: same_doubles).  An item of no or one k-mer reads the
    k-mer that runs into its string's terminator, which the reference scores NaN: the batch runs on cpecan_k_generalv
    with or without the flag"""
    batch, models = vanilla_degenerate()
    bp = band_params(*DEG_BP)
    res, info, got = run_vanilla(ctx, batch, models, bp, ragged, variant)
    assert_wave_path(info, "general", signal_width(batch, bp.diagonalExpansion), W3)
    check_vanilla(("v-degenerate", ragged), res, got, batch, models, bp, ragged, variant)


# the degenerate items no rule sends to the general kernel: no events, a few of both, and the shortest item the
# register-resident kernels take (two k-mers: the k-mer sequence_getKmer2 looks ahead to is the item's last)
SHORT = [(5, 0), (3, 4), (2, 6)]


def vanilla_short_items():
    """two 300 x 600 reads, then items of SHORT's shapes on the first read's bytes and events, each with a model of
    its own (degenerate_batch's layout)"""
    batch = synth.make_batch(302, 2, 300, 600, anchor_every=50)
    base, m0 = batch["items"][0], batch["models"][0]
    items, tables = list(batch["items"]), list(batch["models"])
    for lX, lY in SHORT:
        items.append(dict(base, lX=lX, lY=lY, n_anchors=0, model=len(tables)))
        tables.append(m0)
    batch = dict(batch, items=items, models=tables)
    return batch, [o.VanillaModel(m, skip_bins(k if k < 2 else 0), gy) for k, (m, _, gy) in enumerate(tables)]


def test_vanilla_short_items_on_the_oracle():
    """(CPU) every item of two or more k-mers has finite sums, a finite negative likelihood and finite totals on the
    oracle, under all four ragged pairs; the 5 x 0 item's are those of the degenerate batch"""
    batch, models = vanilla_short_items()
    bp = band_params(*DEG_BP)
    for ragged in RAGGED:
        ref = cached(("v-short", ragged, "e"), lambda: vanilla_oracle(batch, models, bp, ragged))
        post = cached(("v-short", ragged, "post"), lambda: vanilla_posteriors(batch, models, bp, ragged))
        for v, r in zip(ref, post):
            assert np.all(np.isfinite(v)) and v[60] < 0 and np.all(np.isfinite(r["totals"])), ragged
        v = dict(zip(SHORT, ref[2:]))
        assert np.isclose(v[(5, 0)][:60].sum(), 5.0, rtol=1e-12) and np.count_nonzero(v[(5, 0)][:60]) <= 2
        assert np.count_nonzero(v[(2, 6)][:60]) >= 1 and np.count_nonzero(v[(3, 4)][:60]) >= 1
        deg = cached(("v-degenerate", ragged, "e"), lambda: vanilla_oracle(*vanilla_degenerate(), bp, ragged))
        assert np.array_equal(v[(5, 0)], deg[2 + DEGENERATE.index((5, 0))])


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["auto", "general"])
@pytest.mark.parametrize("ragged", RAGGED, ids=["r%d%d" % r for r in RAGGED])
def test_vanilla_short_items_expectations(ctx, ragged, variant):
    """the degenerate items the wave builds can be given (5 x 0, 3 x 4, 2 x 6) inside a batch of ordinary reads, on
    the wave build v2 (AUTO) and on cpecan_k_generalv, against the oracle.  The 0 x 0, 0 x 5 and 1 x 1 items of
    test_vanilla_degenerate_items_expectations can only run on the general kernel: an item of fewer than two k-mers
    sends its batch there"""
    batch, models = vanilla_short_items()
    bp = band_params(*DEG_BP)
    res, info, got = run_vanilla(ctx, batch, models, bp, ragged, variant)
    assert_wave_path(info, variant, signal_width(batch, bp.diagonalExpansion), W3)
    assert variant == "general" or info["cells_per_lane"] == 2, info
    check_vanilla(("v-short", ragged), res, got, batch, models, bp, ragged, variant)


def hdp_degenerate(nhdp):
    batch = degenerate_batch()
    return batch, [o.HdpModel(nhdp) for _ in batch["models"]]


def read_with_first_kmer(batch, it):
    """read_of, an item without k-mers with the six characters at its offset (one past its own five)"""
    x, ev, an = read_of(batch, it)
    return (batch["x_chars"][it["x_offset"]: it["x_offset"] + 6] if it["lX"] == 0 else x), ev, an


def test_hdp_degenerate_items_on_the_oracle(nhdp):
    """(CPU) 0 x 0 nothing at all; 0 x 5 NaN in the two transitions into gap Y and in the likelihood, no assignment;
    5 x 0 five gap-X terms, finite; 1 x 1 and 3 x 4 finite with one to nine assignments.  The 0 x 5 item's NaN is the
    oracle's answer to a k-mer that is none (the item's five characters and their terminator), where the reference exits
    (kmer_to_word, impl/nanopore_hdp.c:358-373); given the six characters at the item's offset the oracle's answer
    is finite, and that is what the device is held to (test_hdp_degenerate_items_expectations)"""
    batch, models = hdp_degenerate(nhdp)
    bp = band_params(*DEG_BP)
    for ragged in RAGGED:
        reads, ref = hdp_oracle(batch, models, bp, ragged)
        v = dict(zip(DEGENERATE, ref[2:]))
        n = dict(zip(DEGENERATE, [len(r["assign"]) for r in reads[2:]]))
        assert not np.any(v[(0, 0)]) and n[(0, 0)] == 0
        assert np.array_equal(np.flatnonzero(np.isnan(v[(0, 5)])), [2, 8, 9]) and n[(0, 5)] == 0
        assert np.all(np.isfinite(v[(5, 0)])) and np.isclose(v[(5, 0)][[1, 4, 7]].sum(), 5.0, rtol=1e-12)
        for shape in ((1, 1), (3, 4)):
            assert np.all(np.isfinite(v[shape])) and 1 <= n[shape] <= 9, (ragged, shape, n[shape])
        for k in (0, 1):
            assert np.all(np.isfinite(ref[k])) and len(reads[k]["assign"]) > 50
        reads6, ref6 = cached(("h-degenerate", ragged, "e"),
                              lambda: hdp_oracle(batch, models, bp, ragged, read_with_first_kmer))
        w = dict(zip(DEGENERATE, ref6[2:]))
        assert np.all(np.isfinite(w[(0, 5)])) and w[(0, 5)][9] < 0
        assert np.isclose(w[(0, 5)][[2, 8]].sum(), 5.0, rtol=1e-12)
        for shape in DEGENERATE:  # (the other shapes are as they were)
            if shape != (0, 5):
                assert np.array_equal(w[shape], v[shape], equal_nan=True), (ragged, shape)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["auto", "general"])
@pytest.mark.parametrize("ragged", RAGGED, ids=["r%d%d" % r for r in RAGGED])
def test_hdp_degenerate_items_expectations(ctx, nhdp, ragged, variant):
    """Every shape against the oracle.  An item without k-mers (0 x 5) is an input the reference cannot be given: its
    sequence_getKmer3 hands the emission the item's five characters and their terminator, and kmer_to_word exits on a
    character outside the alphabet.  Both paths score such an item with the k-mer that starts at its offset (six
    characters, one past its own five), so both are held, at the usual bars, to the oracle given those six
    characters: five gap-Y terms, a finite likelihood, no assignment lost.  See DESIGN.md."""
    batch, models = hdp_degenerate(nhdp)
    bp = band_params(*DEG_BP)
    res, info, got = run_hdp(ctx, nhdp, batch, [cp.NANOPORE_TRANSITIONS] * len(models), bp, ragged, variant)
    assert_wave_path(info, variant, signal_width(batch, bp.diagonalExpansion), W4)
    check_hdp(("h-degenerate", ragged), res, got, batch, models, bp, ragged, variant, read_with_first_kmer)


# test_dna5_gpu.test_degenerate_shapes_agree_between_the_kernels' shapes and a 3 x 4 one; item i's ragged ends are
# (i % 2, i // 2 % 2)
DNA_DEGENERATE = [("", "ACGT"), ("ACGTAC", ""), ("A", "A"), ("A", "C"), ("G", "ACGTACGTAC"), ("ACGTACGTACGT", "T"),
                  ("ACGTACGTTGCA", "ACGTCGTTGCA"), ("ACG", "ACTG")]
DNA_DEG_BP = (0.01, 4, 1, 2)


def dna_degenerate():
    seqs = [(x, y, NO_ANCHORS) for x, y in DNA_DEGENERATE]
    return seqs, dna_models(False) * len(seqs), list(range(len(seqs))), [(i % 2, i // 2 % 2) for i in range(len(seqs))]


def oracle_runs(x, y):
    """the shapes the reference's entry points take as far as the DP (both sequences non-empty)"""
    return len(x) > 0 and len(y) > 0


def test_dna_degenerate_items_on_the_oracle():
    """(CPU) the shapes with two non-empty sequences have finite sums and a negative likelihood on the oracle"""
    seqs, tables, model_of, raggeds = dna_degenerate()
    for i, (x, y, a) in enumerate(seqs):
        if oracle_runs(x, y):
            v = cached(("d-degenerate", i), lambda: dna_oracle([seqs[i]], [tables[i]], [0], band_params(*DNA_DEG_BP),
                                                              [raggeds[i]]))[0]
            assert np.all(np.isfinite(v)) and v[-1] < 0 and np.count_nonzero(v[:25]) >= 1, (i, v[-1])


@pytest.mark.gpu
def test_dna_degenerate_items_expectations(ctx, monkeypatch):
    """the reference's entry points return before the DP for an empty sequence, so for those shapes the three forms
    are held to each other (sums to 1e-9, totals bit for bit); the shapes the oracle runs are compared with it too"""
    seqs, tables, model_of, raggeds = dna_degenerate()
    bp = band_params(*DNA_DEG_BP)
    out = []
    for form in KERNEL_FORMS:
        flags = pick_form(monkeypatch, form) | cp.FLAG_EXPECTATIONS
        res, info, got = run_dna(ctx, seqs, tables, model_of, bp, raggeds, flags, pad="A")
        assert_dna_path(info, 12, flags)
        out.append((res, got))
    for res, got in out[:2]:
        assert_same_totals(res, out[2][0], "forms")
        for k, (g, r) in enumerate(zip(got, out[2][1])):
            assert_expectations_match(g, r, ("forms", k))
    for form, (res, got) in zip(KERNEL_IDS, out):
        for i, (x, y, a) in enumerate(seqs):
            if oracle_runs(x, y):
                ref = cached(("d-degenerate", i), lambda: dna_oracle([seqs[i]], [tables[i]], [0], bp, [raggeds[i]]))[0]
                assert_expectations_match(got[i], ref, (form, i))
                post = cached(("d-degenerate", i, "post"),
                              lambda: dna_posteriors([seqs[i]], [tables[i]], [0], bp, [raggeds[i]]))
                assert_same_totals([res[i]], post, (form, i))


# ------------------------------------------- 3. bytes other than ACGT -------------------------------------------


def vanilla_non_acgt(pos, ch):
    batch = non_acgt_batch(301, 3, 300, 600, 1, pos, ch)
    return batch, vanilla_models(batch)


NON_ACGT_BP = (0.01, 100, 40, 40)


def test_vanilla_non_acgt_on_the_oracle():
    """(CPU) what the device has to reproduce.  E-step: the bad read's model is NaN in all 61 entries (59 of them with
    the byte in the last character); the other reads' models stay finite.  Posterior decode: some of the bad read's
    totals are NaN, none -inf; with the byte inside the first k-mer every total is NaN and no pair comes out, elsewhere
    pairs still do -- a NaN exponent beside finite ones is what the decode's candidate selection has to cope with"""
    bp = band_params(*NON_ACGT_BP)
    for name, pos, ch in NON_ACGT:
        batch, models = vanilla_non_acgt(pos, ch)
        ref = cached(("v-acgt", name, "e"), lambda: vanilla_oracle(batch, models, bp, (1, 1)))
        assert np.count_nonzero(np.isnan(ref[1])) == (59 if name == "last" else 61), name
        assert np.all(np.isfinite(ref[0])) and np.all(np.isfinite(ref[2])), name
        post = cached(("v-acgt", name, "post"), lambda: vanilla_posteriors(batch, models, bp, (1, 1)))
        tot = post[1]["totals"]
        assert np.any(np.isnan(tot)) and not np.any(np.isinf(tot)), name
        if name == "first-kmer":
            assert np.all(np.isnan(tot)) and len(post[1]["triples"]) == 0
        else:
            assert not np.all(np.isnan(tot)) and len(post[1]["triples"]) > 100, name
        for k in (0, 2):
            assert np.all(np.isfinite(post[k]["totals"])) and len(post[k]["triples"]) > 100


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["auto", "general"])
@pytest.mark.parametrize("name,pos,ch", NON_ACGT, ids=[n for n, _, _ in NON_ACGT])
def test_vanilla_non_acgt_expectations(ctx, name, pos, ch, variant):
    """the bad read's model NaN where the oracle's is, the other reads' models finite and the oracle's.  A batch with a
    k-mer that is none runs on cpecan_k_generalv: 'auto' proves that route, 'general' is the same kernel asked for
    (kept so that the route, not the flag, is what the pair shows: both must give the same answers)"""
    batch, models = vanilla_non_acgt(pos, ch)
    bp = band_params(*NON_ACGT_BP)
    res, info, got = run_vanilla(ctx, batch, models, bp, (1, 1), variant)
    assert_wave_path(info, "general", signal_width(batch, bp.diagonalExpansion), W3)
    ref = check_vanilla(("v-acgt", name), res, got, batch, models, bp, (1, 1), variant)
    assert np.all(np.isfinite(ref[0])) and np.all(np.isfinite(ref[2]))


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["auto", "general"])
@pytest.mark.parametrize("name,pos,ch", NON_ACGT, ids=[n for n, _, _ in NON_ACGT])
def test_vanilla_non_acgt_posteriors(ctx, name, pos, ch, variant):
    """cells, totals (bit for bit, a NaN for a NaN) and pairs identical to the oracle's: NaN exponents beside finite
    ones in cpecan_k_generalv's decode, with or without the flag ('auto' proves the route).  The register-resident
    decode, the one that selects candidates by exponent alone, never sees a NaN exponent under this machine: such a
    batch does not reach it"""
    batch, models = vanilla_non_acgt(pos, ch)
    bp = band_params(*NON_ACGT_BP)
    res, info, _ = run_vanilla(ctx, batch, models, bp, (1, 1), variant, flags=0)
    assert_wave_path(info, "general", signal_width(batch, bp.diagonalExpansion), W3)
    post = cached(("v-acgt", name, "post"), lambda: vanilla_posteriors(batch, models, bp, (1, 1)))
    for i in range(3):
        assert_same_posterior(res[i], post[i], (name, variant, i))


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [4, 6])
def test_vanilla_non_acgt_posteriors_on_the_workgroup_builds(ctx, rows):
    """an N in the middle of the first read of a four-wave and of a six-wave workgroup shape under
    CPECAN_FLAG_WIDE_BANDS: the batch leaves the workgroup build for cpecan_k_generalv and equals the oracle; without
    the byte it runs on the build (test_vanilla_workgroup_gpu.py).  No workgroup build runs here: this pins the route
    and the general kernel at bands of 185-376 k-mers with NaN totals"""
    shape = [s for s in VANILLA_WIDE_SHAPES if s["rows"] == rows][0]
    batch = shape_batch(shape)
    x = bytearray(batch["x_chars"])
    x[batch["items"][0]["x_offset"] + batch["items"][0]["lX"] // 2] = ord("N")
    batch = dict(batch, x_chars=bytes(x))
    models = vanilla_models(batch)
    bp = band_params(0.01, shape["md"], shape["tb"], shape["e"])
    res, info, _ = run_vanilla(ctx, batch, models, bp, shape["ragged"], "auto", flags=cp.FLAG_WIDE_BANDS)
    assert info["kernel"] == "general" and build_of(info["max_band_width"]) == rows, info
    post = cached(("v-acgt-wide", rows), lambda: vanilla_posteriors(batch, models, bp, shape["ragged"]))
    assert np.any(np.isnan(post[0]["totals"]))
    for i in range(len(batch["items"])):
        assert_same_posterior(res[i], post[i], (rows, i))


# (name, sequence, place, byte): place 0 the first character, 1 the middle, 2 the last
DNA_NON_ACGT = [("%s-%s%d" % (ch, s, p), s, p, ch) for ch in "Na" for s, p in (("x", 0), ("x", 1), ("x", 2), ("y", 1))]


def dna_non_acgt(s, place, ch):
    """three sequence pairs of about 150 bases, anchored; the second with `ch` in x or in y"""
    rng = np.random.default_rng(4300)
    seqs = []
    for i in range(3):
        x, y, pairs = evolve(rng, 150 + 20 * i)
        seqs.append((x, y, pairs[3::20]))
    x, y, a = seqs[1]
    t = x if s == "x" else y
    at = (0, len(t) // 2, len(t) - 1)[place]
    t = t[:at] + ch + t[at + 1:]
    seqs[1] = (t, y, a) if s == "x" else (x, t, a)
    return seqs, dna_models(False) * 3, [0, 1, 2], [(1, 1)] * 3


DNA_ACGT_BP = (0.01, 60, 10, 20)


def test_dna_non_acgt_on_the_oracle():
    """(CPU) what the three forms are held to.  A base outside ACGT scores log 0 as a match and in both gaps (quirk
    Q3), so no path crosses it: the totals of the windows over it are -inf, never NaN (all 37 with the base in the
    first character, and then no pair; 21 in the middle, 5 in the last character, and pairs still come out of the
    windows before it); the bad pair's E-step divides by such a total: a likelihood of -inf, NaN in the 13
    transitions the machine takes and in all 80 emission bins, zero in the 12 transitions never taken.  The other
    pairs' totals and sums stay finite"""
    bp = band_params(*DNA_ACGT_BP)
    for name, s, place, ch in DNA_NON_ACGT:
        seqs, tables, model_of, raggeds = dna_non_acgt(s, place, ch)
        ref = cached(("d-acgt", name, "e"), lambda: dna_oracle(seqs, tables, model_of, bp, raggeds))
        post = cached(("d-acgt", name, "post"), lambda: dna_posteriors(seqs, tables, model_of, bp, raggeds))
        tot, v = post[1]["totals"], ref[1]
        assert len(tot) == 37 and not np.any(np.isnan(tot)), name
        assert np.count_nonzero(np.isneginf(tot)) == (37, 21, 5)[place], name
        assert (len(post[1]["triples"]) == 0) == (place == 0) and (place == 0 or len(post[1]["triples"]) > 100), name
        assert v[-1] == -np.inf and np.all(np.isnan(v[25:105])), name
        assert np.count_nonzero(np.isnan(v[:25])) == 13 and np.count_nonzero(v[:25] == 0) == 12, name
        for k in (0, 2):
            assert np.all(np.isfinite(ref[k])) and np.all(np.isfinite(post[k]["totals"])), (name, k)


@pytest.mark.gpu
@pytest.mark.parametrize("form", KERNEL_FORMS, ids=KERNEL_IDS)
@pytest.mark.parametrize("name,s,place,ch", DNA_NON_ACGT, ids=[c[0] for c in DNA_NON_ACGT])
def test_dna_non_acgt_posteriors_and_expectations(ctx, name, s, place, ch, form, monkeypatch):
    seqs, tables, model_of, raggeds = dna_non_acgt(s, place, ch)
    bp = band_params(*DNA_ACGT_BP)
    flags = pick_form(monkeypatch, form)
    width = dna_width(seqs, bp.diagonalExpansion)
    post = cached(("d-acgt", name, "post"), lambda: dna_posteriors(seqs, tables, model_of, bp, raggeds))
    res, info, _ = run_dna(ctx, seqs, tables, model_of, bp, raggeds, flags)
    assert_dna_path(info, width, flags)
    for i in range(3):
        assert_same_posterior(res[i], post[i], (name, "posterior", i))
    res, info, got = run_dna(ctx, seqs, tables, model_of, bp, raggeds, flags | cp.FLAG_EXPECTATIONS)
    assert_dna_path(info, width, flags)
    assert_same_totals(res, post, name)
    ref = cached(("d-acgt", name, "e"), lambda: dna_oracle(seqs, tables, model_of, bp, raggeds))
    for k, (g, r) in enumerate(zip(got, ref)):
        assert_expectations_match(g, r, (name, k))


# ------------------------------------------------ 4. a batch run twice ------------------------------------------------


def assert_second_run(first, second):
    """the sums are added with atomics into buffers a second run has to have cleared: the second run's vectors equal
    the first's to rtol 1e-11, its per-item results bit for bit"""
    for f, s in zip(first[2], second[2]):
        assert np.allclose(s, f, rtol=1e-11, atol=0), np.flatnonzero(~np.isclose(s, f, rtol=1e-11, atol=0))[:20]
    for f, s in zip(first[0], second[0]):
        for key in ("triples", "totals_xay"):
            assert np.array_equal(f[key], s[key]), key
        for key in ("logp", "totals"):
            assert np.array_equal(np.asarray(f[key]).view(np.uint64), np.asarray(s[key]).view(np.uint64)), key


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["auto", "general"])
def test_vanilla_expectations_run_twice(ctx, variant):
    batch = synth.make_batch(58, 3, 150, 310, anchor_every=30)
    models = vanilla_models(batch)
    bp = band_params(0.01, 60, 10, 20)
    first, second = run_vanilla(ctx, batch, models, bp, (1, 1), variant, twice=True)
    assert_wave_path(first[1], variant, signal_width(batch, 20), W3)
    assert first[1]["max_band_width"] <= W2
    assert_second_run(first, second)
    for res, _, got in (first, second):
        check_vanilla(("v-twice",), res, got, batch, models, bp, (1, 1), variant)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["auto", "general"])
def test_hdp_expectations_run_twice(ctx, nhdp, variant):
    batch, model = hdp_batch(67, 3, 120, 25, nhdp)
    batch = dict(batch, items=[dict(it, model=0) for it in batch["items"]])
    bp = band_params(0.05, 60, 10, 20)
    first, second = run_hdp(ctx, nhdp, batch, [cp.NANOPORE_TRANSITIONS], bp, (1, 1), variant, twice=True)
    assert_wave_path(first[1], variant, signal_width(batch, 20), W4)
    assert first[1]["max_band_width"] <= W2
    assert_second_run(first, second)
    for res, _, got in (first, second):
        reads, _ = check_hdp(("h-twice",), res, got, batch, [model], bp, (1, 1), variant)
    assert sum(len(r["assign"]) for r in reads) > 50


@pytest.mark.gpu
@pytest.mark.parametrize("form", KERNEL_FORMS, ids=KERNEL_IDS)
def test_dna_expectations_run_twice(ctx, form, monkeypatch):
    flags = pick_form(monkeypatch, form) | cp.FLAG_EXPECTATIONS
    rng = np.random.default_rng(4400)
    seqs = []
    for i in range(3):
        x, y, pairs = evolve(rng, 140 + 30 * i)
        seqs.append((x, y, pairs[5::12]))
    tables, model_of, raggeds = dna_models(True), [0, 1, 0], [(1, 1)] * 3
    bp = band_params(0.01, 40, 8, 10)
    first, second = run_dna(ctx, seqs, tables, model_of, bp, raggeds, flags, twice=True)
    assert_dna_path(first[1], dna_width(seqs, 10), flags)
    assert_second_run(first, second)
    ref = cached(("d-twice", "e"), lambda: dna_oracle(seqs, tables, model_of, bp, raggeds))
    post = cached(("d-twice", "post"), lambda: dna_posteriors(seqs, tables, model_of, bp, raggeds))
    for res, _, got in (first, second):
        assert_same_totals(res, post, form)
        for k, (g, r) in enumerate(zip(got, ref)):
            assert_expectations_match(g, r, (form, k))

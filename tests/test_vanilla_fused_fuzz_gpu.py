"""The vanilla E-step summed inside the wave kernels' sweep back (CPECAN_FLAG_VANILLA_FUSED_ESTEP:
cpecan_k_wv_backward_fx_vf2 / _vf3, the post kernel's finish, the re-sweep of the windows the estimate cannot carry) on what every other E-step path is
run on and these builds were not: the seeded sweep of test_fuzz_expectations_machines_gpu.py, reads on the band's edges,
the A-record cases (a slot that changes column inside one refresh segment with sums to hand over), a batch whose band
holds such records before one that has none, degenerate, short and non-ACGT items, a batch run twice -- and, on every
vanilla E-step path, models whose skip bins are zero.

The inputs are held to what this file relies on by test_vanilla_fused_cases_cpu.py (CPU, the oracle alone), which shares
its oracle vectors with this file through test_band_edges_machines_gpu.cached; the sweep's cases share theirs with
test_fuzz_expectations_machines_gpu.py (the same case_id keys).

Bars, all the project's own: against the oracle, per item the totals bit-identical to its posterior run (a NaN for a NaN:
same_doubles), per model the 60 bins to rtol 1e-9 / atol 1e-12, a finite likelihood to rtol 1e-12 and the same non-finite
entries (assert_expectations_match); fused against the ring build of the same batch 1e-11 on the bins and 1e-12 on the
likelihood (test_vanilla_fused_expectations_gpu.py derives it).  Every case asserts its route: kernel, family, cells per
lane and fused_expectations, or the kernel a batch that must leave the fused builds lands on.

CPECAN_FUZZ_SCALE=N runs N times as many sweep cases (the first ones are the default run's)."""
import numpy as np
import pytest

import pyoracle as o
from harness import band_params, batch_results, cp, make_items
from test_band_edges_machines_gpu import cached
from test_fuzz_expectations_gpu import NON_ACGT, RAGGED, assert_expectations_match, env
from test_fuzz_expectations_machines_gpu import (DEG_BP, NON_ACGT_BP, VANILLA, W2, W3, assert_same_totals,
                                                 assert_sane, assert_second_run, bp_of, case_id, check_vanilla,
                                                 run_vanilla, signal_width, vanilla_batch,
                                                 vanilla_degenerate, vanilla_models, vanilla_non_acgt,
                                                 vanilla_short_items)
from test_vanilla_fused_cases_cpu import (EDGE_FAMILIES, ZERO_CASES, family_case, oracle_posteriors, oracle_sums,
                                          zero_bin_case)
from test_vanilla_workgroup_gpu import check_workgroup

pytestmark = pytest.mark.gpu

FUSED = getattr(cp, "FLAG_VANILLA_FUSED_ESTEP", 0)  # (0 before the flag existed: every route assertion then fails)
EXP = cp.FLAG_EXPECTATIONS
# CPECAN_EXPECT_RESWEEP: unset, the estimate decides; 1 every window swept back once more against the exact totals; 2
# every other one (items and windows alternate), so that a model's sums come from both paths
RESWEEP = {"fused": None, "every-window": "1", "every-other-window": "2"}


@pytest.fixture(scope="module")
def ctx():
    c = cp.Context(0)
    yield c
    c.close()


def run_fused(ctx, batch, models, bp, ragged, variant="auto", resweep="fused", flags=EXP | FUSED, twice=False):
    with env(CPECAN_EXPECT_RESWEEP=RESWEEP[resweep]):
        return run_vanilla(ctx, batch, models, bp, ragged, variant, flags=flags, twice=twice)


def assert_route(info, width, variant="auto", fused=1, general=False):
    """the fused build of the fewest cells per lane that holds the band (of at least three with 'rows3'); a band past
    184 k-mers, and a batch with a k-mer that is none (general), on cpecan_k_generalv, which has no fused form"""
    assert info["max_band_width"] == width, (info, width)
    if general or variant == "general" or width > W3:
        assert info["kernel"] == "general" and info["fused_expectations"] == 0, info
        return
    rows = max(2 + (width > W2), 3 if variant == "rows3" else 2)
    assert info["kernel"] == "systolic" and info["family"] == "wave" and info["cells_per_lane"] == rows, (info, rows)
    assert info["fused_expectations"] == fused, info


def assert_close_to_ring(fused, ring, what):
    for k, (f, r) in enumerate(zip(fused, ring)):
        err = np.abs(f[:60] - r[:60]) / np.maximum(np.abs(r[:60]), 1e-300)
        print("%s model %d: largest relative difference to the ring of the bins %.3g, of the likelihood %.3g" % (
            what, k, err[r[:60] != 0].max(initial=0.0), abs(f[60] - r[60]) / abs(r[60])))
        assert np.allclose(f[:60], r[:60], rtol=1e-11, atol=1e-300), (what, k)
        assert np.isclose(f[60], r[60], rtol=1e-12, atol=0), (what, k)


def check_case(case, res, got, what):
    """check_vanilla on a case of test_vanilla_fused_cases_cpu: totals and sums against the oracle, and the cells"""
    key, batch, models, bp, ragged = case
    ref = check_vanilla(key, res, got, batch, models, bp, ragged, what)
    for i, (g, r) in enumerate(zip(res, oracle_posteriors(key, batch, models, bp, ragged))):
        assert g["cells"] == r["cells"], (what, i)
    return ref


def print_errors(got, ref, what):
    for k, (g, r) in enumerate(zip(got, ref)):
        ok = np.isfinite(r[:60]) & (r[:60] != 0)
        err = np.abs(g[:60][ok] - r[:60][ok]) / np.abs(r[:60][ok])
        print("%s model %d: largest relative error of the bins %.3g" % (what, k, err.max(initial=0.0)))


def ring_of(ctx, case):
    """the same batch on the ring of backward cells (no fused flag), once per session"""
    key, batch, models, bp, ragged = case

    def run():
        res, info, got = run_vanilla(ctx, batch, models, bp, ragged, "auto")
        assert info["fused_expectations"] == 0, info
        return res, got
    return cached(key + ("ring-gpu",), run)


# ------------------------------------------------------- the sweep -------------------------------------------------------

SWEEP = [(c, "auto", "fused") for c in VANILLA] + [(c, "rows3", "fused") for c in VANILLA if c["k"] % 4 == 0] + \
        [(c, "auto", "every-other-window") for c in VANILLA if c["k"] % 2 == 1]


@pytest.mark.parametrize("case,variant,resweep", SWEEP, ids=["%s-%s-%s" % (case_id(c), v, r) for c, v, r in SWEEP])
def test_random_vanilla_fused_expectations(ctx, case, variant, resweep):
    batch, models = vanilla_batch(case)
    bp = bp_of(case)
    res, info, got = run_fused(ctx, batch, models, bp, case["ragged"], variant, resweep)
    assert_route(info, signal_width(batch, case["e"]), variant)
    ref = check_vanilla((case_id(case),), res, got, batch, models, bp, case["ragged"], (variant, resweep))
    print_errors(got, ref, case_id(case))
    assert_sane(ref, case_id(case))


# ------------------------------------------------------ band edges ------------------------------------------------------


def run_family(ctx, name, resweep, cells, centred=False):
    case = family_case(name, centred)
    key, batch, models, bp, ragged = case
    res, info, got = run_fused(ctx, batch, models, bp, ragged, resweep=resweep)
    width = signal_width(batch, batch["e"])
    assert_route(info, width)
    assert cells is None or (width <= W3 and info["cells_per_lane"] == cells), info
    print_errors(got, oracle_sums(key, batch, models, bp, ragged), "%s %s%s" % (name, resweep, " centred" * centred))
    check_case(case, res, got, (name, resweep))
    return case, res, got


@pytest.mark.parametrize("resweep", list(RESWEEP))
@pytest.mark.parametrize("name", EDGE_FAMILIES)
def test_fused_edge_expectations(ctx, name, resweep):
    """reads whose mass runs on the band's edge (w185: one k-mer past the three-cell build, on the general kernel)"""
    case, res, got = run_family(ctx, name, resweep, None)
    ring_res, ring = ring_of(ctx, case)
    assert_close_to_ring(got, ring, "%s %s" % (name, resweep))
    assert_same_totals(res, ring_res, name)


# ------------------------------------------------------- A records -------------------------------------------------------

AREC = [("arec120", 2), ("arec184", 3)]


@pytest.mark.parametrize("resweep", list(RESWEEP))
@pytest.mark.parametrize("name,cells", AREC, ids=[n for n, _ in AREC])
def test_fused_a_records(ctx, name, cells, resweep):
    """a slot hands the sums of the column it leaves to the segment's A record: the store, the post kernel's read of it
    and, on the re-sweep, the same against the exact totals"""
    case, res, got = run_family(ctx, name, resweep, cells)
    _, ring = ring_of(ctx, case)
    assert_close_to_ring(got, ring, "%s %s" % (name, resweep))


@pytest.mark.parametrize("name,cells", AREC, ids=[n for n, _ in AREC])
def test_no_stale_a_records_on_one_context(ctx, name, cells):
    """the A-record batch, then the batch with the same band and its mass down the middle (no A record), then the first
    again: a record of the first that the second's sweep did not reset would be added to the second's sums"""
    for centred in (False, True, False):
        run_family(ctx, name, "fused", cells, centred)


def test_no_stale_a_records_down_a_chain_of_two_contexts():
    """the A-record batch as leader and the centred batch as follower (run(after=...)) on two contexts, two rounds"""
    cases = [family_case("arec184"), family_case("arec184", centred=True)]
    ctxs = [cp.Context(0), cp.Context(0)]
    made = []
    for c, (_, batch, models, bp, ragged) in zip(ctxs, cases):
        mids = c.modelsv_create([(m.scalars, m.match, m.skip, m.gap_y) for m in models])
        b = cp.Batch(c, make_items(batch, ragged), batch["x_chars"], batch["events"], batch["anchors"], bp,
                     flags=EXP | FUSED, vanilla=True)
        assert_route(b.info(), signal_width(batch, batch["e"]))
        assert b.info()["cells_per_lane"] == 3
        made.append((b, mids))
    for round_ in range(2):
        made[0][0].run()
        made[1][0].run(after=made[0][0])
        for (b, mids), case in zip(made, cases):
            b.sync()
            check_case(case, batch_results(b), [b.expectations(m) for m in mids], "round %d" % round_)
    for b, _ in made:
        b.close()
    for c in ctxs:
        c.close()


# ------------------------------------------ degenerate, short and non-ACGT items ------------------------------------------


@pytest.mark.parametrize("ragged", RAGGED, ids=["r%d%d" % r for r in RAGGED])
def test_degenerate_items_leave_the_fused_builds(ctx, ragged):
    """an item of no or one k-mer reads a k-mer that is none: the batch runs on cpecan_k_generalv with the flag too"""
    batch, models = vanilla_degenerate()
    bp = band_params(*DEG_BP)
    res, info, got = run_fused(ctx, batch, models, bp, ragged)
    assert_route(info, signal_width(batch, bp.diagonalExpansion), general=True)
    check_vanilla(("v-degenerate", ragged), res, got, batch, models, bp, ragged, "fused flag")


@pytest.mark.parametrize("resweep", ["fused", "every-window"])
@pytest.mark.parametrize("ragged", RAGGED, ids=["r%d%d" % r for r in RAGGED])
def test_short_items_on_the_fused_build(ctx, ragged, resweep):
    """items of 5 x 0, 3 x 4 and 2 x 6 beside two ordinary reads on the two-cell fused build"""
    batch, models = vanilla_short_items()
    bp = band_params(*DEG_BP)
    res, info, got = run_fused(ctx, batch, models, bp, ragged, resweep=resweep)
    assert_route(info, signal_width(batch, bp.diagonalExpansion))
    assert info["cells_per_lane"] == 2, info
    check_vanilla(("v-short", ragged), res, got, batch, models, bp, ragged, resweep)


@pytest.mark.parametrize("ragged", RAGGED, ids=["r%d%d" % r for r in RAGGED])
@pytest.mark.parametrize("name,pos,ch", NON_ACGT, ids=[n for n, _, _ in NON_ACGT])
def test_non_acgt_reads_leave_the_fused_builds(ctx, name, pos, ch, ragged):
    batch, models = vanilla_non_acgt(pos, ch)
    bp = band_params(*NON_ACGT_BP)
    res, info, got = run_fused(ctx, batch, models, bp, ragged)
    assert_route(info, signal_width(batch, bp.diagonalExpansion), general=True)
    key = ("v-acgt", name) if ragged == (1, 1) else ("v-acgt", name, ragged)
    ref = check_vanilla(key, res, got, batch, models, bp, ragged, name)
    assert np.any(np.isnan(ref[1])) and np.all(np.isfinite(ref[0])) and np.all(np.isfinite(ref[2]))


# ---------------------------------------------------- a batch run twice ----------------------------------------------------


@pytest.mark.parametrize("variant", ["auto", "rows3"])
def test_fused_expectations_run_twice(ctx, variant):
    import synth
    batch = synth.make_batch(58, 3, 150, 310, anchor_every=30)
    models = vanilla_models(batch)
    bp = band_params(0.01, 60, 10, 20)
    first, second = run_fused(ctx, batch, models, bp, (1, 1), variant, twice=True)
    assert_route(first[1], signal_width(batch, 20), variant)
    assert_second_run(first, second)  # the same counts, pairs and totals; the sums not doubled
    for res, _, got in (first, second):
        check_vanilla(("v-twice",), res, got, batch, models, bp, (1, 1), variant)


# ---------------------------------------------------- zero skip bins ----------------------------------------------------

# path -> (run_vanilla's variant, flags, fused_expectations)
PATHS = {"general": ("general", EXP, 0), "ring-v2": ("auto", EXP, 0), "ring-v3": ("rows3", EXP, 0),
         "fused-vf2": ("auto", EXP | FUSED, 1), "fused-vf3": ("rows3", EXP | FUSED, 1)}


def check_zero_bins(case, ragged, res, got, what):
    key, batch, models, bp = case
    return check_case((key + (ragged,), batch, models, bp, ragged), res, got, what)


@pytest.mark.parametrize("ragged", [(1, 1), (0, 0)], ids=["r11", "r00"])
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", ZERO_CASES)
def test_zero_skip_bins(ctx, name, path, ragged):
    """models with skip bins of probability zero on every vanilla E-step path of narrow bands: the oracle's NaN bins and
    its likelihood of -inf where every alignment needs a skip ('nan', 'mixed' -- there the ordinary model's sums are
    untouched), 60 exact zeros where none does, exact zeros in the zeroed bins of 'partial'.  On the fused builds the
    first is the one input that enters the fallback without CPECAN_EXPECT_RESWEEP: the estimate is not finite"""
    case = zero_bin_case(name)
    _, batch, models, bp = case
    variant, flags, fused = PATHS[path]
    res, info, got = run_vanilla(ctx, batch, models, bp, ragged, variant, flags=flags)
    assert_route(info, signal_width(batch, bp.diagonalExpansion), variant, fused)
    ref = check_zero_bins(case, ragged, res, got, (name, path))
    if name == "mixed":
        assert np.all(np.isfinite(ref[1])) and np.any(np.isnan(ref[0]))


@pytest.mark.parametrize("fused", [0, 1], ids=["ve4", "vf4"])
def test_zero_skip_bins_on_the_workgroup_builds(ctx, fused):
    """a read of 700 k-mers and fewer events under models without skips, band 218: the four-wave workgroup build through
    the ring (_ve4) and summed inside the sweep back (_vf4)"""
    case = zero_bin_case("wide-nan")
    _, batch, models, bp = case
    flags = cp.FLAG_WIDE_BANDS_VANILLA_ESTEP | (cp.FLAG_WIDE_BANDS_VANILLA_FUSED_ESTEP if fused else 0)
    res, info, got = run_vanilla(ctx, batch, models, bp, (1, 1), "auto", flags=EXP | flags)
    assert info["fused_expectations"] == fused, info
    check_workgroup(dict(info, fused_expectations=0), 4)
    check_zero_bins(case, (1, 1), res, got, "wide")


@pytest.mark.parametrize("path", ["general", "ring-v2", "fused-vf2"])
def test_zeros_written_in_place(ctx, path):
    """ctx.modelsv_set_skip_probs with 60 zeros between two runs of one batch (what em.PersistentVanillaEStep does with
    the bins the M-step hands it): the second run's sums are the oracle's under models without skips"""
    key, batch, _, bp = zero_bin_case("nan")
    models = vanilla_models(batch)
    variant, flags, fused = PATHS[path]
    ctx.models_clear()
    mids = ctx.modelsv_create([(m.scalars, m.match, m.skip, m.gap_y) for m in models])
    b = cp.Batch(ctx, make_items(batch, (1, 1)), batch["x_chars"], batch["events"], batch["anchors"], bp,
                 flags=flags | (cp.FLAG_GENERAL_KERNEL if variant == "general" else 0), vanilla=True)
    assert_route(b.info(), signal_width(batch, bp.diagonalExpansion), variant, fused)
    b.run()
    b.sync()
    check_vanilla(key + ("own bins",), batch_results(b), [b.expectations(m) for m in mids], batch, models, bp, (1, 1),
                  path)
    ctx.modelsv_set_skip_probs(np.zeros(60))
    b.run()
    b.sync()
    res, got = batch_results(b), [b.expectations(m) for m in mids]
    b.close()
    rezeroed = [o.VanillaModel(m.match, np.zeros(60), m.gap_y, float(m.c.t[0]), float(m.c.t[1])) for m in models]
    ref = check_vanilla(key + ("zeroed in place",), res, got, batch, rezeroed, bp, (1, 1), path)
    assert all(np.any(np.isnan(r)) for r in ref)

"""CPECAN_FLAG_HDP_FUSED_ESTEP on the device: the HDP machine's E-step summed inside the wave kernels' sweep back (builds
_hf2 / _hf3: no ring of backward cells, no expectation kernel), against the CPU oracle at the bars the ring path is held
to -- totals bit-identical, the nine transitions to rtol 1e-9 and the likelihood to 1e-12 (assert_expectations_match),
each read's assignments and their exponents bit-identical and in the reference's order (check_hdp of
test_fuzz_expectations_machines_gpu.py, unchanged).

What the cases are for:
  fuzz          the sixteen HDP cases of the fuzz file with the flag: three thresholds, the three transition sets (the
                gap Y -> gap X switch and the trained one among them: the _sw kernels), two models per batch, ragged ends,
                no anchors; every fourth case also forced onto three cells per lane.  A band past 184 k-mers keeps its
                ring (fused_expectations 0) and its results.
  resweep       a third of them with every window (CPECAN_EXPECT_RESWEEP=1) or every other one (=2) swept once more:
                the re-sweep's sums and its assignments, and items whose windows alternate between the two paths.
  overflow      a threshold so low that one window's candidates outgrow the list (its capacity: 4 x cells per lane x
                ring diagonals): the window has to be swept again, and the assignments outgrow the first pair capacity too.
  capacity      more assignments than 16 x (lX + lY) + 64, the pair capacity of the first run: the batch is run again.
  boundary      bands of exactly 120, 121, 184, 185 k-mers; alignments that hug the band's upper and lower edge and cross
                from one to the other; the degenerate items (0 x 0, 0 x 5, 5 x 0, 1 x 1, 3 x 4).
  twice         nothing accumulates from run to run.
  host          CPECAN_HDP_FUSED_ESTEP=1 through libcpecan_host.so, in processes of their own.
  unflagged     without the flag an HDP batch of expectations keeps the ring.
The CPU twins hold the cases to what they are there for, on the oracle alone."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import edge_reads as er
import pyoracle as o
from harness import band_params, batch_results, cp, hdp_batch, make_items
from test_band_edges_machines_gpu import cached, seed_of
from test_fuzz_expectations_gpu import RAGGED, env
from test_fuzz_expectations_machines_gpu import (HDP, W2, W3, W4, assert_second_run, assert_wave_path, bp_of, case_id,
                                                 check_hdp, ctx, hdp_case_batch, hdp_degenerate, hdp_oracle, nhdp,
                                                 read_with_first_kmer, rows_env, signal_width, trained, transitions_named)

__all__ = ["ctx", "nhdp", "trained"]  # (the fuzz file's fixtures)

FUSED = 65536
HERE = os.path.dirname(os.path.abspath(__file__))
FUZZ = [(c, v) for c in HDP for v in ["auto"] + (["rows3"] if c["k"] % 4 == 0 else [])]
RESWEEP = [(c, v, r) for c, v in FUZZ if c["k"] % 3 == 0 for r in ("1", "2")]


def ids(x):
    return case_id(x) if isinstance(x, dict) else str(x)


def cells_of(width, variant):
    """cells per lane of the wave build an HDP batch of that widest band runs on (0: none of them)"""
    if width > W4:
        return 0
    return max(2 + (width > W2) + (width > W3), int(variant[4:]) if variant.startswith("rows") else 2)


def run_fused(ctx, nhdp, batch, ts, bp, ragged, variant="auto", flags=FUSED, runs=1, resweep=None):
    """(per-item results: the assignments as pairs; info(); per-model vectors) of each run of one HDP E-step batch"""
    ctx.models_clear()
    mids = ctx.modelsh_create([(t, nhdp["alphabet"], nhdp["grid"], nhdp["y"], nhdp["slope"], nhdp["kmer_row"])
                               for t in ts])
    with env(CPECAN_SYSTOLIC_ROWS=rows_env(variant), CPECAN_EXPECT_RESWEEP=resweep):
        b = cp.Batch(ctx, make_items(batch, ragged), batch["x_chars"], batch["events"], batch["anchors"], bp,
                     flags=cp.FLAG_EXPECTATIONS | flags, hdp=True)
    info = b.info()
    out = []
    for _ in range(runs):
        b.run()
        b.sync()
        out.append((batch_results(b), info, [b.expectations(m) for m in mids]))
    b.close()
    return out if runs > 1 else out[0]


def assert_fused_path(info, variant, width):
    """the flag serves two and three cells per lane; what is past them runs what it runs without it"""
    assert_wave_path(info, variant, width, W4)
    cells = cells_of(width, variant)
    if cells in (2, 3):
        assert info["fused_expectations"] == 1 and info["kernel"] == "systolic" and info["family"] == "wave", info
    else:
        assert info["fused_expectations"] == 0, info
    return cells


def fuzz_case(case, nhdp, request):
    tr = request.getfixturevalue("trained") if "trained" in case["tsets"] else None
    ts = [transitions_named(name, tr) for name in case["tsets"]]
    return hdp_case_batch(case, nhdp), ts, [o.HdpModel(nhdp, transitions=t) for t in ts], bp_of(case)


# ------------------------------------------------------- fuzz -------------------------------------------------------


def test_the_selection_reaches_both_builds_with_and_without_the_switch(nhdp):
    """(CPU) at least four fuzz cases on each of _hf2 and _hf3, on each at least one whose batch has a model with the
    gap Y -> gap X transition (the _sw kernels; the kernels without it run the low-threshold, boundary, degenerate and
    run-twice cases, all with the default transitions); some cases past 184 k-mers; re-sweep cases on both builds"""
    on = {0: [], 2: [], 3: [], 4: []}
    for c, v in FUZZ:
        on[cells_of(signal_width(hdp_case_batch(c, nhdp), c["e"]), v)].append(c)
    for cells in (2, 3):
        assert len(on[cells]) >= 4, (cells, len(on[cells]))
        assert any(t != "defaults" for c in on[cells] for t in c["tsets"])  # (a trained set has a tiny finite switch)
        assert len(set(c["thr"] for c in on[cells])) >= 2
    assert on[4] and on[0]
    swept = set(cells_of(signal_width(hdp_case_batch(c, nhdp), c["e"]), v) for c, v, _ in RESWEEP)
    assert {2, 3} <= swept, swept


@pytest.mark.gpu
@pytest.mark.parametrize("case,variant", FUZZ, ids=ids)
def test_random_hdp_fused_expectations_and_assignments(ctx, nhdp, case, variant, request):
    batch, ts, models, bp = fuzz_case(case, nhdp, request)
    res, info, got = run_fused(ctx, nhdp, batch, ts, bp, case["ragged"], variant)
    assert_fused_path(info, variant, signal_width(batch, case["e"]))
    check_hdp((case_id(case),), res, got, batch, models, bp, case["ragged"], variant)


@pytest.mark.gpu
@pytest.mark.parametrize("case,variant,resweep", RESWEEP, ids=ids)
def test_every_window_down_the_resweep(ctx, nhdp, case, variant, resweep, request):
    batch, ts, models, bp = fuzz_case(case, nhdp, request)
    res, info, got = run_fused(ctx, nhdp, batch, ts, bp, case["ragged"], variant, resweep=resweep)
    assert_fused_path(info, variant, signal_width(batch, case["e"]))
    check_hdp((case_id(case),), res, got, batch, models, bp, case["ragged"], (variant, resweep))


# ------------------------------------------------ the lists' capacities ------------------------------------------------

# two reads of about 100 x 130 in one window each (no traceback before the end), a band of 71 k-mers: with a threshold
# this low nearly every transition into match of the band is an assignment
LOW = dict(overflow=(401, 1e-30), capacity=(403, 1e-100))


def low_case(name, nhdp):
    seed, thr = LOW[name]
    batch, model = hdp_batch(seed, 2, 100, 30, nhdp)
    return dict(batch, items=[dict(it, model=0) for it in batch["items"]]), model, band_params(thr, 1000, 40, 40)


def ring_diagonals(batch):
    """the ring of a batch whose reads are one window each: the power of two that holds the longest and four more"""
    d = 64
    while d < max(it["lX"] + it["lY"] for it in batch["items"]) + 4:
        d *= 2
    return d


def test_the_low_threshold_cases_on_the_oracle(nhdp):
    """(CPU) overflow: on average over a read more than 4 L assignments per diagonal, and -- the list's capacity is
    4 L records per diagonal of the ring, the read is one window -- more than the list holds, at L = 2 and 3; capacity:
    more than 16 (lX + lY) + 64 for some read.  Both stay on the two-cell build unless forced."""
    for name in LOW:
        batch, model, bp = low_case(name, nhdp)
        assert signal_width(batch, 40) <= W2
        reads, _ = cached(("hf-low", name, "e"), lambda: hdp_oracle(batch, [model], bp, (1, 1)))
        counts = [len(r["assign"]) for r in reads]
        for it, n in zip(batch["items"], counts):
            assert it["lX"] + it["lY"] < bp.minDiagsBetweenTraceBack  # one window
            if name == "overflow":
                for L in (2, 3):
                    assert n > 4 * L * (it["lX"] + it["lY"]) and n > 4 * L * ring_diagonals(batch), (n, L)
        assert any(n > 16 * (it["lX"] + it["lY"]) + 64 for it, n in zip(batch["items"], counts)), counts


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["auto", "rows3"])
def test_a_candidate_list_that_overflows(ctx, nhdp, variant):
    batch, model, bp = low_case("overflow", nhdp)
    res, info, got = run_fused(ctx, nhdp, batch, [cp.NANOPORE_TRANSITIONS], bp, (1, 1), variant)
    assert assert_fused_path(info, variant, signal_width(batch, 40)) == (3 if variant == "rows3" else 2)
    check_hdp(("hf-low", "overflow"), res, got, batch, [model], bp, (1, 1), variant)


@pytest.mark.gpu
def test_more_assignments_than_the_first_capacity(ctx, nhdp):
    batch, model, bp = low_case("capacity", nhdp)
    res, info, got = run_fused(ctx, nhdp, batch, [cp.NANOPORE_TRANSITIONS], bp, (1, 1))
    assert assert_fused_path(info, "auto", signal_width(batch, 40)) == 2
    reads, _ = check_hdp(("hf-low", "capacity"), res, got, batch, [model], bp, (1, 1), "capacity")
    assert max(len(g["triples"]) for g in res) == max(len(r["assign"]) for r in reads) > 16 * 250


# ------------------------------------------------ degenerate and boundary ------------------------------------------------

DEG_BP = (0.01, 100, 40, 40)


@pytest.mark.gpu
@pytest.mark.parametrize("ragged", RAGGED, ids=["r%d%d" % r for r in RAGGED])
def test_degenerate_items(ctx, nhdp, ragged):
    """as test_hdp_degenerate_items_expectations: every shape beside two ordinary reads, an item without k-mers held to
    the oracle given the six characters at its offset"""
    batch, models = hdp_degenerate(nhdp)
    bp = band_params(*DEG_BP)
    res, info, got = run_fused(ctx, nhdp, batch, [cp.NANOPORE_TRANSITIONS] * len(models), bp, ragged)
    assert assert_fused_path(info, "auto", signal_width(batch, bp.diagonalExpansion)) == 2
    check_hdp(("h-degenerate", ragged), res, got, batch, models, bp, ragged, "fused", read_with_first_kmer)


EDGES = ("upper", "lower", "cross", "w120", "w121", "w184", "w185")


@pytest.mark.gpu
@pytest.mark.parametrize("name", EDGES)
def test_band_edges_and_build_boundaries(ctx, nhdp, name):
    """the band-edge reads of test_band_edges_machines_gpu.py for the HDP machine (the alignment on the band's upper
    edge, on its lower edge, crossing from one to the other) and bands of exactly 120, 121, 184 and 185 k-mers: the
    last k-mer of _hf2, the first and the last of _hf3, and the first that keeps its ring"""
    f = er.FAMILIES[name]
    model = o.HdpModel(nhdp)
    batch = cached(("hdp", name, 0), lambda: er.family_batch(name, seed=seed_of(f, 0), hdp=(nhdp, model)))
    bp = band_params(0.05, f["md"], f["tb"], batch["e"])
    res, info, got = run_fused(ctx, nhdp, batch, [cp.NANOPORE_TRANSITIONS], bp, f["ragged"])
    cells = assert_fused_path(info, "auto", signal_width(batch, batch["e"]))
    if name[0] == "w":
        width = int(name[1:])
        assert info["max_band_width"] == width and cells == 2 + (width > W2) + (width > W3)
        assert info["fused_expectations"] == (1 if width <= W3 else 0)
    reads, _ = check_hdp(("hf-edge", name), res, got, batch, [model], bp, f["ragged"], name)
    assert sum(len(r["assign"]) for r in reads) > 50


# ------------------------------------------------------- twice -------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("resweep", [None, "2"])
def test_run_twice(ctx, nhdp, resweep):
    batch, model = hdp_batch(67, 3, 120, 25, nhdp)
    batch = dict(batch, items=[dict(it, model=0) for it in batch["items"]])
    bp = band_params(0.05, 60, 10, 20)
    first, second = run_fused(ctx, nhdp, batch, [cp.NANOPORE_TRANSITIONS], bp, (1, 1), runs=2, resweep=resweep)
    assert assert_fused_path(first[1], "auto", signal_width(batch, 20)) == 2
    assert_second_run(first, second)
    for res, _, got in (first, second):
        reads, _ = check_hdp(("h-twice",), res, got, batch, [model], bp, (1, 1), "fused")
    assert sum(len(r["assign"]) for r in reads) > 50


# ------------------------------------------------------- host -------------------------------------------------------


@pytest.mark.gpu
def test_host_library_reaches_the_builds_through_the_variable(tmp_path):
    """cpecan_getHdpExpectationsUsingAnchors (libcpecan_host.so) on the read of test_hdp_machine_through_host_api, in a
    process with CPECAN_HDP_FUSED_ESTEP=1 and in one without: the same assignment list, the transitions and the
    likelihood within the bars.  (The batch is the library's own: that the flag routes it is the dispatch tests' to
    show; the variable is read per call, hdp_fused_host_child.py makes two.)"""
    out = {}
    for name, value in (("off", None), ("on", "1")):
        path = os.path.join(str(tmp_path), name + ".json")
        e = dict(os.environ)
        e.pop("CPECAN_HDP_FUSED_ESTEP", None)
        if value is not None:
            e["CPECAN_HDP_FUSED_ESTEP"] = value
        r = subprocess.run([sys.executable, os.path.join(HERE, "hdp_fused_host_child.py"), path], env=e,
                           stderr=subprocess.PIPE, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        out[name] = json.load(open(path))
    on, off = out["on"], out["off"]
    assert on["n"] == off["n"] > 20
    assert on["kmers"] == off["kmers"] and on["events"] == off["events"]
    assert np.allclose(on["t"], off["t"], rtol=1e-9, atol=1e-12)
    assert np.isclose(on["lik"], off["lik"], rtol=1e-12, atol=0) and off["lik"] != 0.0
    assert on["second"] == on["first"]  # (two calls into hmm structures of their own: nothing is left behind)


# ----------------------------------------------------- unflagged -----------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["auto", "rows3"])
def test_without_the_flag_the_ring(ctx, nhdp, variant):
    batch, model = hdp_batch(67, 3, 120, 25, nhdp)
    batch = dict(batch, items=[dict(it, model=0) for it in batch["items"]])
    bp = band_params(0.05, 60, 10, 20)
    res, info, got = run_fused(ctx, nhdp, batch, [cp.NANOPORE_TRANSITIONS], bp, (1, 1), variant, flags=0)
    assert_wave_path(info, variant, signal_width(batch, 20), W4)
    assert info["cells_per_lane"] == (3 if variant == "rows3" else 2) and info["fused_expectations"] == 0, info
    check_hdp(("h-twice",), res, got, batch, [model], bp, (1, 1), variant)

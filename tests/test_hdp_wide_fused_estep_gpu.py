"""CPECAN_FLAG_WIDE_BANDS_HDP_FUSED_ESTEP on the device: the HDP machine's E-step summed inside the workgroup kernels'
sweep back (builds _hf6 / _hf8 in the place of _he6 / _he8: no ring of backward cells, no expectation kernel), against
the CPU oracle at the bars the ring path is held to -- totals bit-identical, the nine transitions to rtol 1e-9 / atol
1e-12 and the likelihood to rtol 1e-12 and non-zero (assert_expectations_match), each read's assignments and their
exponents bit-identical and in the reference's order (assert_same_assignments).  Threshold 0.05 unless a case says
otherwise.  Every case asserts its route: with the flags fused_expectations 1 on the workgroup family at six or eight
waves, without the new flag 0 -- most cases would pass on _he or on the general kernel otherwise.

What the cases are for:
  shapes        the six shapes of test_hdp_workgroup_gpu.py (three or more traceback windows, ragged ends); the same batch
                on _he<n> and on the general kernel gives the same lists bit for bit.
  fuzz          the first dozen of test_hdp_workgroup_gpu.fuzz_cases() with the default, the strong-switch and the trained
                transitions in turn (the gap Y -> gap X term both ways) and two models in every fourth; one of them
                without anchors.  A band outside 249..504 keeps what it ran (fused_expectations 0) and its results.
  resweep       a third of them with every window (CPECAN_EXPECT_RESWEEP=1) or every other one (=2) down the second
                sweep: its sums and the assignments it emits, and items whose windows alternate between the two paths.
  boundary      bands of exactly 248, 249, 376, 377, 504, 505 k-mers on the band's upper and lower edge, a read that
                crosses from one edge to the other, the degenerate items beside a wide read.
  threshold 0   no log-threshold: every window goes down the second sweep, and the pair capacity is outgrown.
  overflow      a threshold so low that one wave's parked assignments outgrow its list (4 records per ring diagonal).
  capacity      more assignments than 16 x (lX + lY) + 64, the pair capacity of the first run: the batch is run again.
  twice         nothing accumulates from run to run.
  host          CPECAN_WIDE_BANDS_HDP_FUSED_ESTEP=1 through libcpecan_host.so, in processes of their own.
  unflagged     CPECAN_FLAG_WIDE_BANDS_HDP_ESTEP alone, and with 65536, keeps the ring.
The CPU twins hold the cases to what they are there for, on the oracle and the band table alone."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import edge_reads as er
import pyoracle as o
from harness import band_params, batch_results, cp, make_items, with_gap_switch
from test_band_edges_machines_gpu import cached, read_of
from test_fuzz_expectations_gpu import RAGGED, assert_expectations_match, env
from test_fuzz_expectations_machines_gpu import (assert_same_assignments, assert_same_totals, assert_second_run,
                                                 hdp_oracle, hdp_posteriors, read_with_first_kmer, signal_width, trained)
from test_hdp_workgroup_estep_gpu import ctx, degenerate_beside_a_wide_read, nhdp, same_lists, same_sums
from test_hdp_workgroup_gpu import (SHAPES, W6, W8, WV, build_of, exact_width_batch, fuzz_batch, fuzz_cases, shape_batch,
                                    shape_bp, shape_id, shape_of, threshold_zero_read)

__all__ = ["ctx", "nhdp", "trained"]  # (the fixtures of the files the helpers come from)

ESTEP = cp.FLAG_WIDE_BANDS_HDP_ESTEP
FUSED = getattr(cp, "FLAG_WIDE_BANDS_HDP_FUSED_ESTEP", 0)  # (0 before the flag existed: every route assertion then fails)
THR = 0.05
HERE = os.path.dirname(os.path.abspath(__file__))
STRONG = with_gap_switch(cp.NANOPORE_TRANSITIONS, 0.1)
TSETS = (("defaults",), ("strong",), ("trained",), ("defaults", "strong"))


def run_fused(ctx, nhdp, batch, ts, bp, ragged, flags=None, runs=1, resweep=None):
    """(per-item results: the assignments as pairs; info(); per-model vectors) of each run of one HDP E-step batch"""
    ctx.models_clear()
    mids = ctx.modelsh_create([(t, nhdp["alphabet"], nhdp["grid"], nhdp["y"], nhdp["slope"], nhdp["kmer_row"])
                               for t in ts])
    with env(CPECAN_EXPECT_RESWEEP=resweep):
        b = cp.Batch(ctx, make_items(batch, ragged), batch["x_chars"], batch["events"], batch["anchors"], bp,
                     flags=cp.FLAG_EXPECTATIONS | (ESTEP | FUSED if flags is None else flags), hdp=True)
    info = b.info()
    out = []
    for _ in range(runs):
        b.run()
        b.sync()
        out.append((batch_results(b), info, [b.expectations(m) for m in mids]))
    b.close()
    return out if runs > 1 else out[0]


def assert_route(info, rows, fused=1):
    """a workgroup build of `rows` waves (None: whatever a band outside 249..504 runs on, and never a fused pass)"""
    if rows is None:
        assert build_of(info["max_band_width"]) is None and info["fused_expectations"] == 0, info
        return
    assert info["kernel"] == "systolic" and info["family"] == "workgroup", info
    assert info["waves_per_workgroup"] == rows and build_of(info["max_band_width"]) == rows, info
    assert info["fused_expectations"] == fused, info


def check(key, res, got, batch, models, bp, ragged, what, read_of=read_of):
    """every model's ten sums, every read's totals and its assignments against the oracle's of each read alone"""
    assert_same_totals(res, cached(("hwf-post",) + key, lambda: hdp_posteriors(batch, models, bp, ragged, read_of)), what)
    reads, ref = cached(("he",) + key, lambda: hdp_oracle(batch, models, bp, ragged, read_of))
    assert len(got) == len(ref)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert_expectations_match(g, r, (what, k))
    assert_same_assignments(res, reads, what)
    return reads, ref


DEFAULTS = [cp.NANOPORE_TRANSITIONS]

# ------------------------------------------------------- shapes -------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_shapes_match_the_oracle(ctx, nhdp, shape):
    batch = shape_batch(shape, nhdp)
    bp = shape_bp(shape, THR)
    res, info, got = run_fused(ctx, nhdp, batch, DEFAULTS, bp, shape["ragged"])
    assert_route(info, shape["rows"])
    for it in batch["items"]:
        assert (it["lX"] + it["lY"]) // shape["md"] >= 3  # several traceback windows
    reads, ref = check(("shape", shape["seed"]), res, got, batch, [o.HdpModel(nhdp)], bp, shape["ragged"], shape_id(shape))
    assert ref[0][9] != 0.0 and sum(len(r["assign"]) for r in reads) > 50


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [6, 8])
def test_same_batch_on_the_ring_build_and_on_the_general_kernel(ctx, nhdp, rows):
    shape = shape_of(rows, 1)
    batch = shape_batch(shape, nhdp)
    bp = shape_bp(shape, THR)
    fx, info, fsum = run_fused(ctx, nhdp, batch, DEFAULTS, bp, shape["ragged"])
    assert_route(info, rows)
    ring, info, rsum = run_fused(ctx, nhdp, batch, DEFAULTS, bp, shape["ragged"], flags=ESTEP)
    assert_route(info, rows, fused=0)
    gen, info, gsum = run_fused(ctx, nhdp, batch, DEFAULTS, bp, shape["ragged"], flags=0)
    assert info["kernel"] == "general" and info["fused_expectations"] == 0, info
    for other, sums in ((ring, rsum), (gen, gsum)):
        same_lists(other, fx)
        same_sums(sums, fsum)
    assert sum(len(r["triples"]) for r in fx) > 50


# ------------------------------------------------------- fuzz -------------------------------------------------------

FUZZ = fuzz_cases(12)
RESWEEP = [(k, r) for k in range(len(FUZZ)) if k % 3 == 0 for r in ("1", "2")]
NO_ANCHORS = 2  # the case run without its anchors: its band is then the whole matrix, 378 k-mers wide (eight waves)


def fuzz_case(k, nhdp, request=None):
    """(batch, the transition sets' names, band parameters) of case k: a threshold of 0.0 replaced by 0.05, the models
    dealt to the reads in turn, case NO_ANCHORS without anchors"""
    c = FUZZ[k]
    names = TSETS[k % 4]
    batch = fuzz_batch(c, nhdp)
    items = [dict(it, model=i % len(names), **(dict(n_anchors=0) if k == NO_ANCHORS else {}))
             for i, it in enumerate(batch["items"])]
    return dict(batch, items=items), names, band_params(c["thr"] if c["thr"] > 0.0 else THR, c["md"], c["tb"], c["e"])


def transitions_of(names, request):
    return [{"defaults": cp.NANOPORE_TRANSITIONS, "strong": STRONG,
             "trained": request.getfixturevalue("trained") if n == "trained" else None}[n] for n in names]


def test_the_fuzz_cases_reach_both_builds_and_leave_them(nhdp):
    """(CPU) from the band table alone: at least four cases on each of six and eight waves, some outside 249..504; every
    transition set on a served case, two models among them, and re-sweep cases on both builds"""
    on = {6: [], 8: [], None: []}
    for k in range(len(FUZZ)):
        batch, names, bp = fuzz_case(k, nhdp)
        on[build_of(signal_width(batch, bp.diagonalExpansion))].append(k)
    print("fuzz cases by build:", on)
    assert len(on[6]) >= 4 and len(on[8]) >= 4 and on[None], on
    served = on[6] + on[8]
    assert set(TSETS[k % 4] for k in served) == set(TSETS)
    assert {6, 8} <= set(b for b in (6, 8) for k, _ in RESWEEP if k in on[b])


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(FUZZ)), ids=lambda k: "seed%d" % FUZZ[k]["seed"])
def test_fuzz(ctx, nhdp, k, request):
    batch, names, bp = fuzz_case(k, nhdp)
    ts = transitions_of(names, request)
    ragged = FUZZ[k]["ragged"]
    res, info, got = run_fused(ctx, nhdp, batch, ts, bp, ragged)
    print("fuzz case", FUZZ[k]["seed"], names, info)
    assert_route(info, build_of(signal_width(batch, bp.diagonalExpansion)))
    check(("hwf-fuzz", k), res, got, batch, [o.HdpModel(nhdp, transitions=t) for t in ts], bp, ragged, k)
    if info["fused_expectations"] == 0:  # unchanged results: those of the same batch without the flag
        ring, rinfo, rsum = run_fused(ctx, nhdp, batch, ts, bp, ragged, flags=ESTEP)
        assert rinfo == info
        same_lists(ring, res)


@pytest.mark.gpu
@pytest.mark.parametrize("k,resweep", RESWEEP, ids=lambda v: str(v))
def test_every_window_down_the_second_sweep(ctx, nhdp, k, resweep, request):
    batch, names, bp = fuzz_case(k, nhdp)
    ts = transitions_of(names, request)
    ragged = FUZZ[k]["ragged"]
    res, info, got = run_fused(ctx, nhdp, batch, ts, bp, ragged, resweep=resweep)
    assert_route(info, build_of(signal_width(batch, bp.diagonalExpansion)))
    check(("hwf-fuzz", k), res, got, batch, [o.HdpModel(nhdp, transitions=t) for t in ts], bp, ragged, (k, resweep))


# ------------------------------------------------------ boundary ------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("place", ["upper", "lower"])
@pytest.mark.parametrize("width", [248, 249, 376, 377, 504, 505])
def test_bands_at_the_edges_of_the_builds(ctx, nhdp, width, place):
    model = o.HdpModel(nhdp)
    batch, _ = exact_width_batch(width, place, (nhdp, model))
    bp = band_params(THR, 150, 40, batch["e"])
    ragged = (width % 2, 1)
    res, info, got = run_fused(ctx, nhdp, batch, DEFAULTS, bp, ragged)
    assert info["max_band_width"] == width
    assert_route(info, {249: 6, 376: 6, 377: 8, 504: 8}.get(width))
    if width == WV:
        assert info["kernel"] == "systolic" and info["family"] == "wave" and info["cells_per_lane"] == 4, info
    if width > W8:
        assert info["kernel"] == "general", info
    reads, _ = check(("edge", width, place), res, got, batch, [model], bp, ragged, (width, place))
    assert sum(len(r["assign"]) for r in reads) > 50


CROSS = dict(lX=700, lY=1050, width=320, cross=(0.45, 0.5), md=150, tb=40, ragged=(1, 1))


@pytest.mark.gpu
def test_a_read_that_crosses_the_band(ctx, nhdp):
    """edge_reads' crossing read (the band's lower edge up to 45 % of the diagonals, its upper edge from 50 %) at a band
    of 320 k-mers"""
    model = o.HdpModel(nhdp)
    f = CROSS
    batch = cached(("hwf-cross",), lambda: er.edge_batch(7, 1, f["lX"], f["lY"], "cross", every=1, e=40, width=f["width"],
                                                         cross=f["cross"], hdp=(nhdp, model)))
    bp = band_params(THR, f["md"], f["tb"], batch["e"])
    res, info, got = run_fused(ctx, nhdp, batch, DEFAULTS, bp, f["ragged"])
    assert info["max_band_width"] == f["width"]
    assert_route(info, 6)
    reads, _ = check(("hwf-cross",), res, got, batch, [model], bp, f["ragged"], "cross")
    assert sum(len(r["assign"]) for r in reads) > 50


@pytest.mark.gpu
@pytest.mark.parametrize("ragged", RAGGED, ids=["r%d%d" % r for r in RAGGED])
@pytest.mark.parametrize("rows", [6, 8])
def test_degenerate_items_beside_a_wide_read(ctx, nhdp, rows, ragged):
    """items of 0 x 0, 0 x 5, 5 x 0, 1 x 1 and 3 x 4 and a read that ends inside its first traceback window beside a read
    whose band asks for the build; an item without k-mers is scored with the k-mer that starts at its offset"""
    batch, bp = degenerate_beside_a_wide_read(rows, nhdp)
    models = [o.HdpModel(nhdp) for _ in batch["items"]]
    res, info, got = run_fused(ctx, nhdp, batch, DEFAULTS * len(models), bp, ragged)
    assert_route(info, rows)
    reads, ref = check(("degenerate", rows, ragged), res, got, batch, models, bp, ragged, (rows, ragged),
                       read_with_first_kmer)
    assert len(reads[-1]["assign"]) > 5 and len(reads[-2]["assign"]) > 50
    assert all(np.all(np.isfinite(v)) for v in ref)


# ---------------------------------------------- threshold 0 and the lists ----------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [6, 8])
def test_threshold_zero(ctx, nhdp, rows):
    """no log-threshold: every window goes down the second sweep, which emits a pair for every cell of the band whose
    lower-left neighbour two diagonals down is in the band, one of exponent -inf too; far more than the first pair
    allocation, so the batch is run again.  Lists and sums are _he<n>'s and the oracle's."""
    batch, model, bp = threshold_zero_read(rows, nhdp)
    res, info, got = run_fused(ctx, nhdp, batch, DEFAULTS, bp, (1, 1))
    assert_route(info, rows)
    it = batch["items"][0]
    assert len(res[0]["triples"]) > 16 * (it["lX"] + it["lY"]) + 64
    check(("hwf-thr0", rows), res, got, batch, [model], bp, (1, 1), rows)
    ring, info, rsum = run_fused(ctx, nhdp, batch, DEFAULTS, bp, (1, 1), flags=ESTEP)
    assert_route(info, rows, fused=0)
    same_lists(ring, res)
    same_sums(rsum, got)


def low_read(nhdp):
    """threshold_zero_read(6)'s read (300 k-mers, a single anchor: the band is the whole matrix, 300 k-mers wide) in one
    window, at a threshold so low that nearly every transition into match of the band is an assignment"""
    batch, model, bp0 = threshold_zero_read(6, nhdp)
    return batch, model, band_params(1e-30, 1000, 40, bp0.diagonalExpansion)


def ring_diagonals(batch):
    """the ring of a workgroup batch whose reads are one window each: the power of two that holds the longest and four
    more diagonals (sweep_storage, cpecan_hip.hip)"""
    d = 64
    while d < max(it["lX"] + it["lY"] for it in batch["items"]) + 4:
        d *= 2
    return d


def parked_per_wave(reads, rows, log_thr):
    """per wave of a build of `rows` waves, the oracle's assignments of a one-window read whose exponent reaches log_thr:
    a lower bound of what the sweep parks there (a wave owns the matrix columns x + 1 of its 64 slots modulo 64 x rows)"""
    n = np.zeros(rows, np.int64)
    for r in reads:
        a, e = np.asarray(r["assign"]).reshape(-1, 3), np.asarray(r["logp"])
        np.add.at(n, ((a[:, 1] + 1) % (64 * rows)) // 64, e >= log_thr)
    return n


def test_the_low_threshold_read_on_the_oracle(nhdp):
    """(CPU) one window; at 1e-30 some wave's assignments alone outgrow its list (4 records per ring diagonal), at 0.05
    every wave's stay far below it"""
    batch, model, bp = low_read(nhdp)
    it = batch["items"][0]
    assert it["lX"] + it["lY"] < bp.minDiagsBetweenTraceBack and build_of(signal_width(batch, bp.diagonalExpansion)) == 6
    cap = 4 * ring_diagonals(batch)
    reads, _ = cached(("he", "hwf-low"), lambda: hdp_oracle(batch, [model], bp, (1, 1)))
    low = parked_per_wave(reads, 6, np.log(1e-30))
    usual = parked_per_wave(reads, 6, np.log(THR) - 0.25 - 1e-3)  # (what the sweep parks at 0.05: within the slack)
    print("capacity", cap, "assignments per wave at 1e-30", low, "within the slack of 0.05", usual)
    assert low.max() > cap and usual.max() < cap // 4


@pytest.mark.gpu
def test_a_list_of_parked_assignments_that_overflows(ctx, nhdp):
    batch, model, bp = low_read(nhdp)
    res, info, got = run_fused(ctx, nhdp, batch, DEFAULTS, bp, (1, 1))
    assert_route(info, 6)
    check(("hwf-low",), res, got, batch, [model], bp, (1, 1), "overflow")


@pytest.mark.parametrize("rows", [6, 8])
def test_the_capacity_case_on_the_oracle(nhdp, rows):
    """(CPU) more assignments than the first pair allocation, 16 per element of lX + lY plus 64"""
    batch, model, bp0 = threshold_zero_read(rows, nhdp)
    bp = band_params(1e-4, 200, 40, bp0.diagonalExpansion)
    it = batch["items"][0]
    reads, _ = cached(("he", "overflow", rows), lambda: hdp_oracle(batch, [model], bp, (1, 1)))
    assert len(reads[0]["assign"]) > 16 * (it["lX"] + it["lY"]) + 64


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [6, 8])
def test_more_assignments_than_the_first_capacity(ctx, nhdp, rows):
    batch, model, bp0 = threshold_zero_read(rows, nhdp)
    bp = band_params(1e-4, 200, 40, bp0.diagonalExpansion)
    res, info, got = run_fused(ctx, nhdp, batch, DEFAULTS, bp, (1, 1))
    assert_route(info, rows)
    it = batch["items"][0]
    reads, _ = check(("overflow", rows), res, got, batch, [model], bp, (1, 1), rows)
    assert len(res[0]["triples"]) == len(reads[0]["assign"]) > 16 * (it["lX"] + it["lY"]) + 64


# ------------------------------------------------------- twice -------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("resweep", [None, "2"])
@pytest.mark.parametrize("rows", [6, 8])
def test_run_twice(ctx, nhdp, rows, resweep):
    shape = shape_of(rows, 1)
    batch = shape_batch(shape, nhdp)
    bp = shape_bp(shape, THR)
    first, second = run_fused(ctx, nhdp, batch, DEFAULTS, bp, shape["ragged"], runs=2, resweep=resweep)
    assert_route(first[1], rows)
    assert_second_run(first, second)
    for res, _, got in (first, second):
        check(("shape", shape["seed"]), res, got, batch, [o.HdpModel(nhdp)], bp, shape["ragged"], (rows, resweep))


# ------------------------------------------------------- host -------------------------------------------------------


@pytest.mark.gpu
def test_host_library_reaches_the_builds_through_the_variable(tmp_path):
    """cpecan_getHdpExpectationsUsingAnchors (libcpecan_host.so) on a read whose band is 300 k-mers wide, in processes
    with CPECAN_WIDE_BANDS_HDP_ESTEP=1, one of them with CPECAN_WIDE_BANDS_HDP_FUSED_ESTEP=1 too: the same assignment
    list, the transitions and the likelihood within the bars.  (The batch is the library's own: that the flag routes it
    is the dispatch tests' to show; the variable is read per call, the child makes two.)"""
    out = {}
    for name, value in (("off", None), ("on", "1")):
        path = os.path.join(str(tmp_path), name + ".json")
        e = dict(os.environ, CPECAN_WIDE_BANDS_HDP_ESTEP="1")
        e.pop("CPECAN_WIDE_BANDS_HDP_FUSED_ESTEP", None)
        if value is not None:
            e["CPECAN_WIDE_BANDS_HDP_FUSED_ESTEP"] = value
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(HERE, "hdp_wide_fused_host_child.py"),
                            path], env=e, stderr=subprocess.PIPE, text=True, timeout=400)
        assert r.returncode == 0, r.stderr[-2000:]
        out[name] = json.load(open(path))
    on, off = out["on"], out["off"]
    assert on["n"] == off["n"] > 50
    assert on["kmers"] == off["kmers"] and on["events"] == off["events"]
    assert np.allclose(on["t"], off["t"], rtol=1e-9, atol=1e-12)
    assert np.isclose(on["lik"], off["lik"], rtol=1e-12, atol=0) and off["lik"] != 0.0
    assert on["second"] == on["first"]  # (two calls into hmm structures of their own: nothing is left behind)


# ----------------------------------------------------- unflagged -----------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, 65536], ids=["alone", "with65536"])
@pytest.mark.parametrize("rows", [6, 8])
def test_without_the_flag_the_ring(ctx, nhdp, rows, flags):
    shape = shape_of(rows, 0)
    batch = shape_batch(shape, nhdp)
    bp = shape_bp(shape, THR)
    res, info, got = run_fused(ctx, nhdp, batch, DEFAULTS, bp, shape["ragged"], flags=ESTEP | flags)
    assert_route(info, rows, fused=0)
    check(("shape", shape["seed"]), res, got, batch, [o.HdpModel(nhdp)], bp, shape["ragged"], (rows, flags))
    assert FUSED == 131072 and W6 == 376

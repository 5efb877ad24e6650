"""CPECAN_FLAG_HDP_FOUR_CELLS_FUSED_ESTEP on the device: the HDP machine's E-step summed inside the sweep back of the
four-cell wave build _hf4 (bands of 185..248 k-mers, or a narrower band under CPECAN_SYSTOLIC_ROWS=4: no ring of
backward cells, no expectation kernel), against the CPU oracle at the bars the ring path is held to -- totals
bit-identical, the nine transitions to rtol 1e-9 and the likelihood to 1e-12 (assert_expectations_match), each read's
assignments and their exponents bit-identical and in the reference's order (check_hdp of
test_fuzz_expectations_machines_gpu.py, unchanged).  Every fused case asserts fused_expectations == 1, four cells per
lane and the wave family.

What the cases are for:
  fuzz          the HDP fuzz cases whose widest band is 185..248 k-mers as they are (three thresholds, the gap Y -> gap X
                switch and the trained transitions among them: the plain and the _sw kernels), and two narrower ones
                forced onto four cells.
  resweep       three of them with every window (CPECAN_EXPECT_RESWEEP=1) or every other one (=2) swept once more.
  overflow      a threshold so low that one window's candidates outgrow the four-cell list (4 x 4 x ring diagonals).
  capacity      more assignments than 16 x (lX + lY) + 64, the pair capacity of the first run: the batch is run again.
  boundary      bands of exactly 185 and 248 k-mers (the first and the last of the build), 184 (three cells: this flag
                means nothing) and 249 (the general kernel); alignments on the band's edges forced onto four cells; the
                degenerate items.
  twice         nothing accumulates from run to run.
  both          65536 | 262144 on one context: a narrow batch on _hf2, then one of 185..248 k-mers on _hf4.
  unflagged     without the flag a batch at four cells keeps the ring (with 65536 too).
  host          CPECAN_HDP_FOUR_CELLS_FUSED_ESTEP=1 through libcpecan_host.so, in processes of their own.
tests/test_hdp_four_cells_fused_cases_cpu.py holds the cases to what they are there for, on the oracle alone."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import edge_reads as er
import pyoracle as o
from harness import band_params, cp, hdp_batch
from test_band_edges_machines_gpu import cached, seed_of
from test_fuzz_expectations_gpu import RAGGED
from test_fuzz_expectations_machines_gpu import (HDP, W2, W3, W4, assert_second_run, assert_wave_path, case_id, check_hdp,
                                                 ctx, hdp_degenerate, nhdp, read_with_first_kmer, signal_width,
                                                 trained)
from test_hdp_fused_estep_gpu import DEG_BP, fuzz_case, low_case, run_fused

__all__ = ["ctx", "nhdp", "trained"]  # (the fuzz file's fixtures)

FOUR = 262144
NARROW = 65536
HERE = os.path.dirname(os.path.abspath(__file__))
BY_K = dict((c["k"], c) for c in HDP)
# the fuzz cases whose widest band is 185..248 k-mers (190, 221, 196, 199, 193: the CPU twin checks them on the oracle),
# and two narrower ones forced onto four cells
OWN = [2, 3, 4, 12, 14]
FORCED = [0, 8]
FUZZ = [(BY_K[k], "auto") for k in OWN] + [(BY_K[k], "rows4") for k in FORCED]
RESWEEP = [(BY_K[k], v, r) for k, v in ((2, "auto"), (3, "auto"), (12, "auto"), (8, "rows4")) for r in ("1", "2")]
HOST_READ = (91, 299, 100, 130)  # seed, k-mers, an anchor every so many, diagonalExpansion: a band of 231 k-mers


def ids(x):
    return case_id(x) if isinstance(x, dict) else str(x)


def assert_four_cells_fused(info, variant, width):
    assert_wave_path(info, variant, width, W4)
    assert info["fused_expectations"] == 1 and info["cells_per_lane"] == 4, info
    assert info["kernel"] == "systolic" and info["family"] == "wave", info


# ------------------------------------------------------- fuzz -------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("case,variant", FUZZ, ids=ids)
def test_random_hdp_fused_expectations_and_assignments(ctx, nhdp, case, variant, request):
    batch, ts, models, bp = fuzz_case(case, nhdp, request)
    res, info, got = run_fused(ctx, nhdp, batch, ts, bp, case["ragged"], variant, flags=FOUR)
    assert_four_cells_fused(info, variant, signal_width(batch, case["e"]))
    check_hdp((case_id(case),), res, got, batch, models, bp, case["ragged"], variant)


@pytest.mark.gpu
@pytest.mark.parametrize("case,variant,resweep", RESWEEP, ids=ids)
def test_every_window_down_the_resweep(ctx, nhdp, case, variant, resweep, request):
    batch, ts, models, bp = fuzz_case(case, nhdp, request)
    res, info, got = run_fused(ctx, nhdp, batch, ts, bp, case["ragged"], variant, flags=FOUR, resweep=resweep)
    assert_four_cells_fused(info, variant, signal_width(batch, case["e"]))
    check_hdp((case_id(case),), res, got, batch, models, bp, case["ragged"], (variant, resweep))


# ------------------------------------------------ the lists' capacities ------------------------------------------------


@pytest.mark.gpu
def test_a_candidate_list_that_overflows(ctx, nhdp):
    """the window's candidates outgrow 4 x 4 x 256 records: it is swept again, and the results are the oracle's"""
    batch, model, bp = low_case("overflow", nhdp)
    res, info, got = run_fused(ctx, nhdp, batch, [cp.NANOPORE_TRANSITIONS], bp, (1, 1), "rows4", flags=FOUR)
    assert_four_cells_fused(info, "rows4", signal_width(batch, 40))
    check_hdp(("hf-low", "overflow"), res, got, batch, [model], bp, (1, 1), "rows4")


@pytest.mark.gpu
def test_more_assignments_than_the_first_capacity(ctx, nhdp):
    batch, model, bp = low_case("capacity", nhdp)
    res, info, got = run_fused(ctx, nhdp, batch, [cp.NANOPORE_TRANSITIONS], bp, (1, 1), "rows4", flags=FOUR)
    assert_four_cells_fused(info, "rows4", signal_width(batch, 40))
    reads, _ = check_hdp(("hf-low", "capacity"), res, got, batch, [model], bp, (1, 1), "capacity4")
    assert max(len(g["triples"]) for g in res) == max(len(r["assign"]) for r in reads) > 16 * 250


# ------------------------------------------------ degenerate and boundary ------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("ragged", RAGGED, ids=["r%d%d" % r for r in RAGGED])
def test_degenerate_items(ctx, nhdp, ragged):
    """every shape (0 x 0, 0 x 5, 5 x 0, 1 x 1, 3 x 4) beside two ordinary reads, an item without k-mers held to the
    oracle given the six characters at its offset"""
    batch, models = hdp_degenerate(nhdp)
    bp = band_params(*DEG_BP)
    res, info, got = run_fused(ctx, nhdp, batch, [cp.NANOPORE_TRANSITIONS] * len(models), bp, ragged, "rows4",
                               flags=FOUR)
    assert_four_cells_fused(info, "rows4", signal_width(batch, bp.diagonalExpansion))
    check_hdp(("h-degenerate", ragged), res, got, batch, models, bp, ragged, "fused4", read_with_first_kmer)


EDGES = ("upper", "lower", "cross", "w184", "w185", "w248", "w249")


@pytest.mark.gpu
@pytest.mark.parametrize("name", EDGES)
def test_band_edges_and_build_boundaries(ctx, nhdp, name):
    """the band-edge reads of test_band_edges_machines_gpu.py for the HDP machine forced onto four cells, and bands of
    exactly 185 and 248 k-mers -- the first and the last k-mer of the build -- with 184 (three cells, the ring: this
    flag alone means nothing there) and 249 (the general kernel) beside them"""
    f = er.FAMILIES[name]
    model = o.HdpModel(nhdp)
    batch = cached(("hdp", name, 0), lambda: er.family_batch(name, seed=seed_of(f, 0), hdp=(nhdp, model)))
    bp = band_params(0.05, f["md"], f["tb"], batch["e"])
    variant = "auto" if name[0] == "w" else "rows4"
    res, info, got = run_fused(ctx, nhdp, batch, [cp.NANOPORE_TRANSITIONS], bp, f["ragged"], variant, flags=FOUR)
    width = signal_width(batch, batch["e"])
    if name == "w184":
        assert_wave_path(info, "auto", width, W4)
        assert info["max_band_width"] == 184 == W3 and info["cells_per_lane"] == 3 and info["fused_expectations"] == 0
    elif name == "w249":
        assert info["max_band_width"] == 249 == W4 + 1 and info["kernel"] == "general", info
        assert info["fused_expectations"] == 0, info
    else:
        assert_four_cells_fused(info, variant, width)
        if name[0] == "w":
            assert info["max_band_width"] == int(name[1:])
        else:
            assert width <= W3   # (four cells are forced)
    reads, _ = check_hdp(("hf-edge", name), res, got, batch, [model], bp, f["ragged"], name)
    assert sum(len(r["assign"]) for r in reads) > 50


# ------------------------------------------------------- twice -------------------------------------------------------


def small_batch(nhdp):
    batch, model = hdp_batch(67, 3, 120, 25, nhdp)
    return dict(batch, items=[dict(it, model=0) for it in batch["items"]]), model, band_params(0.05, 60, 10, 20)


@pytest.mark.gpu
@pytest.mark.parametrize("resweep", [None, "2"])
def test_run_twice(ctx, nhdp, resweep):
    batch, model, bp = small_batch(nhdp)
    first, second = run_fused(ctx, nhdp, batch, [cp.NANOPORE_TRANSITIONS], bp, (1, 1), "rows4", flags=FOUR, runs=2,
                              resweep=resweep)
    assert_four_cells_fused(first[1], "rows4", signal_width(batch, 20))
    assert_second_run(first, second)
    for res, _, got in (first, second):
        reads, _ = check_hdp(("h-twice",), res, got, batch, [model], bp, (1, 1), "fused4")
    assert sum(len(r["assign"]) for r in reads) > 50


# ------------------------------------------------------- both -------------------------------------------------------


@pytest.mark.gpu
def test_both_flags_on_one_context(ctx, nhdp, request):
    """a batch that carries 65536 | 262144 is fused at two, three and four cells: one of at most 120 k-mers on _hf2,
    then one of 185..248 on _hf4, on the same context, each on its own build"""
    batch, model, bp = small_batch(nhdp)
    res, info, got = run_fused(ctx, nhdp, batch, [cp.NANOPORE_TRANSITIONS], bp, (1, 1), flags=NARROW | FOUR)
    assert_wave_path(info, "auto", signal_width(batch, 20), W4)
    assert signal_width(batch, 20) <= W2 and info["cells_per_lane"] == 2 and info["fused_expectations"] == 1, info
    check_hdp(("h-twice",), res, got, batch, [model], bp, (1, 1), "both2")
    case = BY_K[4]
    batch, ts, models, bp = fuzz_case(case, nhdp, request)
    res, info, got = run_fused(ctx, nhdp, batch, ts, bp, case["ragged"], flags=NARROW | FOUR)
    assert_four_cells_fused(info, "auto", signal_width(batch, case["e"]))
    check_hdp((case_id(case),), res, got, batch, models, bp, case["ragged"], "both4")


# ----------------------------------------------------- unflagged -----------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, NARROW], ids=["alone", "with65536"])
@pytest.mark.parametrize("which", ["own", "forced"])
def test_without_the_flag_the_ring(ctx, nhdp, which, flags, request):
    """the feature is opt-in: at four cells an HDP batch of expectations without 262144 keeps the ring and its results"""
    case, variant = (BY_K[2], "auto") if which == "own" else (BY_K[0], "rows4")
    batch, ts, models, bp = fuzz_case(case, nhdp, request)
    res, info, got = run_fused(ctx, nhdp, batch, ts, bp, case["ragged"], variant, flags=flags)
    assert_wave_path(info, variant, signal_width(batch, case["e"]), W4)
    assert info["cells_per_lane"] == 4 and info["fused_expectations"] == 0, info
    check_hdp((case_id(case),), res, got, batch, models, bp, case["ragged"], (variant, flags))


# ------------------------------------------------------- host -------------------------------------------------------


@pytest.mark.gpu
def test_host_library_reaches_the_build_through_the_variable(nhdp, tmp_path):
    """cpecan_getHdpExpectationsUsingAnchors (libcpecan_host.so) on a read whose band comes out in 185..248 k-mers, in a
    process with CPECAN_HDP_FOUR_CELLS_FUSED_ESTEP=1 and in one without: the same assignment list, the transitions and
    the likelihood within the bars.  (The batch is the library's own: the width is checked here, on the C-ABI's band
    and plan calls; that the flag routes such a batch is the dispatch tests' to show; the variable is read per call,
    the child makes two.)"""
    seed, lX, every, e = HOST_READ
    batch, _ = hdp_batch(seed, 1, lX, every, nhdp)
    it = batch["items"][0]
    bl, br = cp.band_construct(batch["anchors"], it["lX"], it["lY"], e)
    width = int(((br - bl) // 2 + 1).max())
    assert W3 < width <= W4 and width == 231, width
    q = (cp.MACHINE_HDP, cp.MODE_EXPECTATIONS, cp.KERNEL_AUTO)
    assert cp.plan_dispatch(*q, FOUR, width, True) == dict(kernel=cp.KERNEL_SYSTOLIC, wave=1, rows=4, build_max_width=248)
    assert cp.plan_expectation_pass(*q, FOUR, width, True) == 1 and cp.plan_expectation_pass(*q, 0, width, True) == 0
    out = {}
    for name, value in (("off", None), ("on", "1")):
        path = os.path.join(str(tmp_path), name + ".json")
        env = dict(os.environ)
        for k in ("CPECAN_HDP_FOUR_CELLS_FUSED_ESTEP", "CPECAN_HDP_FUSED_ESTEP", "CPECAN_SYSTOLIC_ROWS"):
            env.pop(k, None)
        if value is not None:
            env["CPECAN_HDP_FOUR_CELLS_FUSED_ESTEP"] = value
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable,
                            os.path.join(HERE, "hdp_four_cells_fused_host_child.py"), path, str(seed), str(lX), str(every),
                            str(e), str(width)], env=env, stderr=subprocess.PIPE, text=True, timeout=400)
        assert r.returncode == 0, r.stderr[-2000:]
        out[name] = json.load(open(path))
    on, off = out["on"], out["off"]
    assert on["n"] == off["n"] > 50
    assert on["kmers"] == off["kmers"] and on["events"] == off["events"]
    assert np.allclose(on["t"], off["t"], rtol=1e-9, atol=1e-12)
    assert np.isclose(on["lik"], off["lik"], rtol=1e-12, atol=0) and off["lik"] != 0.0
    assert on["second"] == on["first"]  # (two calls into hmm structures of their own: nothing is left behind)

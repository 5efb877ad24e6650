"""The vanilla machine's E-step with its expectations summed inside the workgroup kernels' sweep back
(CPECAN_FLAG_WIDE_BANDS_VANILLA_FUSED_ESTEP beside CPECAN_FLAG_WIDE_BANDS_VANILLA_ESTEP: cpecan_k_sy_backward_vf4 / _vf6 /
_vf8 -- the terms, the segment records, the finish through 60 bins of LDS, the second sweep of the windows the estimate
cannot carry) against the oracle's vanilla E-step and against the _ve builds' path through the ring of backward cells and
cpecan_k_sy_expect.  The shapes are those of test_vanilla_workgroup_estep_gpu.py, whose oracle vectors
test_vanilla_workgroup_estep_cases_cpu.py computes once for both files and holds to what the bars need (all 60 bins in
use, a finite negative likelihood).

Bars: against the oracle the project's for every E-step -- the 60 bins to rtol 1e-9 / atol 1e-12 (the same terms added
in another order, the device's exp), the likelihood to rtol 1e-12, the same non-finite entries
(assert_expectations_match); every item's totals and cell count bit-identical to the oracle's posterior run.  Fused
against the ring 1e-11 on the bins (a term exp(a - estimate) * exp(estimate - total) in place of exp(a - total): the
estimate lies within 30 nats of the total, so the two differ by a few ulp of an argument of that size, as
test_vanilla_fused_expectations_gpu.py reasons for the wave builds) and 1e-12 on the likelihood; a run with the skip bins
rewritten in place against a fresh batch 1e-12 (the same kernels on the same tables: only the order of the atomic
additions differs).  Every case asserts its route -- the workgroup family with the build's waves (check_workgroup, which
pins fused_expectations == 0 for the _ve builds: it is asked with that one entry set aside) and fused_expectations == 1:
without that each would pass on the ring path."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pyoracle as o
from cpecan_load import em
from harness import band_params, batch_results, cp
from test_fuzz_expectations_gpu import assert_expectations_match, env
from test_fuzz_expectations_machines_gpu import same_doubles, signal_width, vanilla_oracle
from test_vanilla_fused_cases_cpu import family_case
from test_vanilla_fused_expectations_gpu import FUDGE
from test_vanilla_scaled_models_gpu import as_tuple, host_scaled, two_strand_batch
from test_vanilla_workgroup_estep_cases_cpu import EDGE_WIDTHS, edge_case, oracle_sums, shape_case
from test_vanilla_workgroup_estep_gpu import (NEW_BINS, WIDE_FAMILIES, check_oracle, ebatch, run_estep,
                                              short_items_beside_a_wide_read, upload)
from test_vanilla_workgroup_gpu import (SHAPES, W8, WV, build_of, check_workgroup, shape_batch, shape_id, shape_of,
                                        vanilla_models)

pytestmark = pytest.mark.gpu

WIDE_FUSED = getattr(cp, "FLAG_WIDE_BANDS_VANILLA_FUSED_ESTEP", 0)  # (0 before the flag existed: every route assertion then fails)
ESTEP = cp.FLAG_WIDE_BANDS_VANILLA_ESTEP
EXP = cp.FLAG_EXPECTATIONS
FUSED = ESTEP | WIDE_FUSED
HOST_SHAPE = shape_of(4, 2)  # (vanilla_wide_fused_host_child.py runs the same one)


@pytest.fixture(scope="module")
def ctx():
    c = cp.Context(0)
    yield c
    c.close()


def check_fused(info, rows):
    """the route: a workgroup build of `rows` waves whose E-step sums inside the sweep back"""
    assert info["fused_expectations"] == 1, info
    check_workgroup(dict(info, fused_expectations=0), rows)


def test_the_flag_exists():
    assert WIDE_FUSED == 32768


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_fused_batches_match_the_oracle(ctx, shape):
    case = shape_case(shape)
    _, batch, models, bp, ragged = case
    res, info, got = run_estep(ctx, batch, models, bp, ragged, FUSED)
    check_fused(info, shape["rows"])
    check_oracle(case, res, got, shape_id(shape))


@pytest.mark.parametrize("width", EDGE_WIDTHS)
def test_bands_at_the_edges_of_the_builds(ctx, width):
    case = edge_case(width)
    _, batch, models, bp, ragged = case
    res, info, got = run_estep(ctx, batch, models, bp, ragged, FUSED)
    assert info["max_band_width"] == width
    if width <= WV:    # the wave builds, where this flag means nothing (and the wave builds' own flag was not given)
        assert info["kernel"] == "systolic" and info["family"] == "wave" and info["cells_per_lane"] == 3, info
        assert info["fused_expectations"] == 0, info
    elif width > W8:
        assert info["kernel"] == "general" and info["fused_expectations"] == 0, info
    else:
        check_fused(info, build_of(width))
    check_oracle(case, res, got, width)


@pytest.mark.parametrize("rows", [4, 6, 8])
def test_fused_against_the_ring_of_backward_cells(ctx, rows):
    case = shape_case(shape_of(rows, 1))
    _, batch, models, bp, ragged = case
    res_r, info, ring = run_estep(ctx, batch, models, bp, ragged, ESTEP)
    check_workgroup(info, rows)
    res_f, info, fused = run_estep(ctx, batch, models, bp, ragged, FUSED)
    check_fused(info, rows)
    for k, (f, r) in enumerate(zip(fused, ring)):
        err = np.abs(f[:60] - r[:60]) / np.abs(r[:60])
        print("rows %d model %d: largest relative difference of the bins %.3g, of the likelihood %.3g" % (
            rows, k, err.max(), abs(f[60] - r[60]) / abs(r[60])))
        assert np.count_nonzero(r[:60]) == 60
        assert np.allclose(f[:60], r[:60], rtol=1e-11, atol=1e-300)
        assert np.isclose(f[60], r[60], rtol=1e-12, atol=0)
    for a, b in zip(res_f, res_r):
        assert same_doubles(a["totals"], b["totals"]) and a["cells"] == b["cells"]


@pytest.mark.parametrize("rows", [4, 6, 8])
@pytest.mark.parametrize("resweep", [1, 2], ids=["every-window", "every-other-window"])
def test_windows_down_the_second_sweep(ctx, rows, resweep, monkeypatch):
    """CPECAN_EXPECT_RESWEEP=1: every window swept back once more against the exact totals; 2: every other one (items
    and windows alternate), so that a model's sums come from both paths"""
    monkeypatch.setenv("CPECAN_EXPECT_RESWEEP", str(resweep))
    case = shape_case(shape_of(rows))
    _, batch, models, bp, ragged = case
    res, info, got = run_estep(ctx, batch, models, bp, ragged, FUSED)
    check_fused(info, rows)
    check_oracle(case, res, got, "rows %d resweep %d" % (rows, resweep))


def run_wide_family(ctx, name, rows, resweep=None, centred=False):
    """an edge_reads.VANILLA_FAMILIES batch on the fused build of `rows` waves, against the oracle at check_oracle's
    bars (sums, totals, cell counts); CPECAN_EXPECT_RESWEEP as test_windows_down_the_second_sweep sets it"""
    case = family_case(name, centred)
    _, batch, models, bp, ragged = case
    with env(CPECAN_EXPECT_RESWEEP=resweep):
        res, info, got = run_estep(ctx, batch, models, bp, ragged, FUSED)
    check_fused(info, rows)
    assert info["max_band_width"] == signal_width(batch, batch["e"])
    for k, (g, r) in enumerate(zip(got, oracle_sums(*case))):
        print("%s resweep %s%s model %d: largest relative error of the bins %.3g" % (
            name, resweep, " centred" * centred, k,
            (np.abs(g[:60] - r[:60])[r[:60] != 0] / np.abs(r[:60][r[:60] != 0])).max(initial=0.0)))
    check_oracle(case, res, got, (name, resweep, centred))
    return case, res, got


@pytest.mark.parametrize("resweep", [None, "1", "2"], ids=["fused", "every-window", "every-other-window"])
@pytest.mark.parametrize("name,rows", WIDE_FAMILIES, ids=[n for n, _ in WIDE_FAMILIES])
def test_a_records_and_lower_edges(ctx, name, rows, resweep):
    """varec...: a slot hands the sums of the column it leaves to the segment's A record (`x + 1 != gCol`): the store,
    the post kernel's read of it and, on the second sweep, the same against the exact totals -- against the oracle and
    against the _ve build's path through the ring.  vlower...: the path on the band's lower edge"""
    case, res_f, fused = run_wide_family(ctx, name, rows, resweep)
    _, batch, models, bp, ragged = case
    res_r, info, ring = run_estep(ctx, batch, models, bp, ragged, ESTEP)
    check_workgroup(info, rows)
    for k, (f, r) in enumerate(zip(fused, ring)):
        assert np.allclose(f[:60], r[:60], rtol=1e-11, atol=1e-300), (name, k)
        assert np.isclose(f[60], r[60], rtol=1e-12, atol=0), (name, k)
    for a, b in zip(res_f, res_r):
        assert same_doubles(a["totals"], b["totals"]) and a["cells"] == b["cells"]


@pytest.mark.parametrize("width", [248, 376, 504])
def test_no_stale_a_records(ctx, width):
    """the A-record batch, then the batch with the same band and its mass down the middle (no A record), then the first
    again, on one context: a record of the first that the second's sweep did not reset would be added to the second's
    sums"""
    for centred in (False, True, False):
        run_wide_family(ctx, "varec%d" % width, build_of(width), centred=centred)


@pytest.mark.parametrize("rows", [4, 6, 8])
def test_run_twice(ctx, rows):
    case = shape_case(shape_of(rows, 1))
    _, batch, models, bp, ragged = case
    mids = upload(ctx, models)
    b = ebatch(ctx, batch, bp, ragged, FUSED)
    check_fused(b.info(), rows)
    runs = []
    for _ in range(2):
        b.run()
        b.sync()
        runs.append((batch_results(b), [b.expectations(m) for m in mids], b.counts()))
    b.close()
    for first, second in zip(runs[0][2], runs[1][2]):
        assert np.array_equal(first, second)
    for res, got, _ in runs:     # ... and not doubled
        check_oracle(case, res, got, rows)


def test_chained_rounds_and_two_contexts():
    """a four-wave and an eight-wave batch of two contexts, the second run behind the first (run(after=...)), three
    rounds: the segment records in scratch are reused from round to round"""
    cases = [shape_case(shape_of(4)), shape_case(shape_of(8))]
    ctxs = [cp.Context(0), cp.Context(0)]
    made = []
    for c, (_, batch, models, bp, ragged), rows in zip(ctxs, cases, (4, 8)):
        mids = upload(c, models)
        b = ebatch(c, batch, bp, ragged, FUSED)
        check_fused(b.info(), rows)
        made.append((b, mids))
    for round_ in range(3):
        made[0][0].run()
        made[1][0].run(after=made[0][0])
        for (b, mids), case in zip(made, cases):
            b.sync()
            check_oracle(case, batch_results(b), [b.expectations(m) for m in mids], "round %d" % round_)
    for b, _ in made:
        b.close()
    for c in ctxs:
        c.close()


def test_two_items_share_one_model(ctx):
    """both reads of a four-wave shape on the first read's model: the atomics of two workgroups hit the same 61
    doubles"""
    _, batch, models, bp, ragged = shape_case(shape_of(4, 2))
    assert len(batch["items"]) == 2
    batch = dict(batch, items=[dict(it, model=0) for it in batch["items"]])
    models = models[:1]
    res, info, got = run_estep(ctx, batch, models, bp, ragged, FUSED)
    check_fused(info, 4)
    ref = check_oracle((("ve-shared", 4), batch, models, bp, ragged), res, got, "shared")
    assert np.all(np.isfinite(ref[0])) and np.count_nonzero(ref[0][:60]) == 60


@pytest.mark.parametrize("ragged", [(1, 1), (0, 0)], ids=["r11", "r00"])
def test_short_items_beside_a_wide_read(ctx, ragged):
    """items of no events, of a few of both and of two k-mers ride on the six-wave fused build beside a read that needs
    it"""
    batch, models, bp = short_items_beside_a_wide_read()
    res, info, got = run_estep(ctx, batch, models, bp, ragged, FUSED)
    check_fused(info, 6)
    assert info["max_band_width"] == signal_width(batch, bp.diagonalExpansion)
    ref = check_oracle((("ve-short", ragged), batch, models, bp, ragged), res, got, ragged)
    assert all(np.all(np.isfinite(r)) and r[60] < 0 for r in ref)
    assert np.isclose(ref[2][:60].sum(), 5.0, rtol=1e-12)  # the 5 x 0 item: five gap-X steps


def test_skip_bins_rewritten_between_two_runs(ctx):
    """ctx.modelsv_set_skip_probs between two runs of one fused batch: the second run's sums are the oracle's with the
    new bins in every model, and equal to 1e-12 those of a fresh fused batch on tables built with the new bins"""
    shape = shape_of(6, 1)
    case = shape_case(shape)
    _, batch, models, bp, ragged = case
    mids = upload(ctx, models)
    b = ebatch(ctx, batch, bp, ragged, FUSED)
    check_fused(b.info(), 6)
    b.run()
    b.sync()
    check_oracle(case, batch_results(b), [b.expectations(m) for m in mids], "own bins")
    ctx.modelsv_set_skip_probs(NEW_BINS)
    b.run()
    b.sync()
    res, got = batch_results(b), [b.expectations(m) for m in mids]
    b.close()
    rebinned = [o.VanillaModel(m.match, NEW_BINS, m.gap_y, float(m.c.t[0]), float(m.c.t[1])) for m in models]
    new = check_oracle((("ve-rebinned", shape["seed"]), batch, rebinned, bp, ragged), res, got, "new bins")
    old = oracle_sums(*case)
    assert not np.allclose(new[0][:60], old[0][:60], rtol=1e-3, atol=0)  # the new bins are other bins
    _, info, fresh = run_estep(ctx, batch, rebinned, bp, ragged, FUSED)
    check_fused(info, 6)
    for g, f in zip(got, fresh):
        assert np.allclose(g, f, rtol=1e-12, atol=1e-300)


def test_persistent_e_step_after_new_bins_in_place():
    """em.PersistentVanillaEStep with the two flags: an iteration, the skip bins rewritten in place
    (cpecan_hip_modelsv_set_skip_probs), a second iteration -- equal to a fresh fused batch on tables built with the new
    bins"""
    import torch
    sh = shape_of(4, 2)
    batch, bases, strand_of, _ = two_strand_batch(83, 2, sh["lX"], sh["lY"], sh["every"])
    bp = band_params(0.01, sh["md"], sh["tb"], sh["e"])
    n = len(batch["items"])
    ctx = cp.Context(0)
    step = em().PersistentVanillaEStep(cp, [ctx], batch, bp, range(n), [as_tuple(m) for m in bases], strand_of,
                                       flags=FUSED)
    check_fused(step.batches[0][1].info(), 4)
    first = step(bases[0].skip.copy())
    second = step(NEW_BINS)
    fresh = cp.Context(0)
    ids = fresh.modelsv_create([host_scaled(bases[strand_of[i]], batch["scalings"][i], NEW_BINS) for i in range(n)])
    items = np.zeros(n, cp.ITEM_DTYPE)
    for i, it in enumerate(batch["items"]):
        items[i] = (it["x_offset"], it["lX"], it["y_offset"], it["lY"], it["anchor_offset"], it["n_anchors"], ids[i], 1, 1, 0)
    b = cp.Batch(fresh, items, batch["x_chars"], batch["events"], batch["anchors"], bp, flags=EXP | FUSED, vanilla=True)
    check_fused(b.info(), 4)
    b.run()
    b.sync()
    ptr, size = b.expectations_device_ptr()  # added up as the persistent step adds them: one sum on the device
    want = torch.as_tensor(em()._DeviceDoubles(ptr, size), device="cuda:0").view(-1, 61).sum(0).cpu().numpy()
    b.close()
    assert second.shape == (61,) and np.count_nonzero(want[:60]) > 20 and want[60] < 0
    assert np.allclose(second, want, rtol=1e-12, atol=1e-300)
    assert not np.allclose(second, first, rtol=1e-3, atol=0)  # the new bins are other bins
    step.close()
    fresh.close()
    ctx.close()


def test_a_byte_that_is_no_nucleotide_sends_the_batch_to_the_general_kernel(ctx):
    """an N in the middle of the first read of a four-wave shape: with the flags the batch runs where it runs without,
    on cpecan_k_generalv, and gives the same vectors, a NaN for a NaN"""
    _, batch, _, bp, ragged = shape_case(shape_of(4))
    x = bytearray(batch["x_chars"])
    x[batch["items"][0]["x_offset"] + batch["items"][0]["lX"] // 2] = ord("N")
    batch = dict(batch, x_chars=bytes(x))
    models = vanilla_models(batch)
    _, info0, plain = run_estep(ctx, batch, models, bp, ragged, 0)
    _, info1, flagged = run_estep(ctx, batch, models, bp, ragged, FUSED)
    for info in (info0, info1):
        assert info["kernel"] == "general" and info["fused_expectations"] == 0, info
        assert build_of(info["max_band_width"]) == 4, info
    assert np.any(np.isnan(plain[0])) and np.all(np.isfinite(plain[1]))
    for g, r in zip(flagged, plain):
        assert same_doubles(g, r)
    assert WIDE_FUSED == 32768  # (the route above is the parent's too: the case must not pass before the flag exists)


def test_an_item_of_fewer_than_two_kmers_sends_the_batch_to_the_general_kernel(ctx):
    _, batch, _, bp, ragged = shape_case(shape_of(6))
    base = batch["items"][0]
    batch = dict(batch, items=list(batch["items"]) + [dict(base, lX=1, lY=4, n_anchors=0, model=0)])
    upload(ctx, vanilla_models(batch))
    b = ebatch(ctx, batch, bp, ragged, FUSED)
    info = b.info()
    b.close()
    assert info["kernel"] == "general" and info["fused_expectations"] == 0, info
    assert build_of(info["max_band_width"]) == 6, info
    assert WIDE_FUSED == 32768


def test_host_library_in_a_fresh_process(tmp_path, golden_dir):
    """CPECAN_WIDE_BANDS_VANILLA_ESTEP=1 CPECAN_WIDE_BANDS_VANILLA_FUSED_ESTEP=1 in a child process: the reference-shaped
    vanilla E-step call of libcpecan_host.so on the reads of a four-wave shape gives the oracle's sums.  (Which path the
    call took cannot be seen through the reference's interface: results only; the choice itself is covered at the
    C-ABI, and each read alone has a widest band of the four-wave class.)"""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "vanilla_wide_fused_host_child.py")
    path = str(tmp_path / "sums.json")
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, child, path],
                       env=dict(os.environ, CPECAN_WIDE_BANDS_VANILLA_ESTEP="1", CPECAN_WIDE_BANDS_VANILLA_FUSED_ESTEP="1"),
                       capture_output=True, text=True, timeout=150)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.array(json.load(open(path)))
    sh = HOST_SHAPE
    batch = shape_batch(sh)
    for it in batch["items"]:
        assert build_of(signal_width(dict(batch, items=[it]), sh["e"])) == 4
    match, skip, gapy = o.load_pore_model(os.path.join(golden_dir, "template_median68pA.model"))
    model = o.VanillaModel(match, skip, gapy, *FUDGE[0])
    one = dict(batch, items=[dict(it, model=0) for it in batch["items"]])
    ref = vanilla_oracle(one, [model], band_params(0.01, sh["md"], sh["tb"], sh["e"]), sh["ragged"])[0]
    assert np.count_nonzero(ref[:60]) == 60 and np.isfinite(ref[60]) and ref[60] < 0
    assert_expectations_match(got, ref, "host library")
    assert WIDE_FUSED == 32768

"""The vanilla machine's E-step on the workgroup-per-alignment kernels (CPECAN_FLAG_WIDE_BANDS_VANILLA_ESTEP on a
vanilla batch of expectations: four waves per workgroup for bands of 185..248 k-mers, six for 249..376, eight for
377..504) against the oracle's vanilla E-step (o.expectations_v_using_anchors), through the C-ABI.  The bars are the
project's for every E-step: the 60 skip bins to rtol 1e-9 / atol 1e-12 (atomic additions of the same terms in an order
that differs from run to run), the likelihood to rtol 1e-12, the same non-finite entries
(test_fuzz_expectations_gpu.assert_expectations_match); every item's totals and cell count bit-identical to the
oracle's posterior run.  Every case asserts its route: without it most of them would pass on the general kernel.

The inputs are held to what this file relies on by test_vanilla_workgroup_estep_cases_cpu.py (CPU, the oracle alone),
which also computes the oracle's vectors once for both files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pyoracle as o
from harness import batch_results, cp, make_items
from test_fuzz_expectations_gpu import assert_expectations_match
from test_fuzz_expectations_machines_gpu import (assert_same_totals, same_doubles, signal_width, vanilla_oracle,
                                                 vanilla_short_items)
from test_vanilla_fused_cases_cpu import family_case
from test_vanilla_gpu import skip_bins
from test_vanilla_workgroup_estep_cases_cpu import (EDGE_WIDTHS, edge_case, oracle_posteriors, oracle_sums,
                                                    shape_case)
from test_vanilla_workgroup_gpu import (SHAPES, W8, WV, build_of, check_workgroup, exact_width_batch, shape_id,
                                        shape_of, vanilla_models)

pytestmark = pytest.mark.gpu

ESTEP = getattr(cp, "FLAG_WIDE_BANDS_VANILLA_ESTEP", 0)  # (0 before the flag existed: every route assertion then fails)
EXP = cp.FLAG_EXPECTATIONS
NEW_BINS = np.concatenate([skip_bins(7), skip_bins(8) * 0.8])  # beta | alpha, other than any model's own


@pytest.fixture(scope="module")
def ctx():
    c = cp.Context(0)
    yield c
    c.close()


def upload(ctx, models):
    ctx.models_clear()
    return ctx.modelsv_create([(m.scalars, m.match, m.skip, m.gap_y) for m in models])


def ebatch(ctx, batch, bp, ragged, flags):
    return cp.Batch(ctx, make_items(batch, ragged), batch["x_chars"], batch["events"], batch["anchors"], bp,
                    flags=EXP | flags, vanilla=True)


def run_estep(ctx, batch, models, bp, ragged, flags):
    """(per-item results, info(), per-model vectors) of one vanilla batch of expectations"""
    mids = upload(ctx, models)
    b = ebatch(ctx, batch, bp, ragged, flags)
    info = b.info()
    b.run()
    b.sync()
    res, got = batch_results(b), [b.expectations(m) for m in mids]
    b.close()
    return res, info, got


def check_oracle(case, res, got, what):
    """every model's 61 sums within the bar of the oracle's E-step; every item's totals and cells its posterior run's"""
    key, batch, models, bp, ragged = case
    ref = oracle_sums(key, batch, models, bp, ragged)
    assert len(got) == len(ref)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert_expectations_match(g, r, (what, k))
    post = oracle_posteriors(key, batch, models, bp, ragged)
    assert_same_totals(res, post, what)
    for i, (g, r) in enumerate(zip(res, post)):
        assert g["cells"] == r["cells"], (what, i)
    return ref


def same_sums(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.allclose(x[:60], y[:60], rtol=1e-9, atol=1e-12)
        assert np.isclose(x[60], y[60], rtol=1e-12, atol=0) and x[60] != 0.0


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_vanilla_workgroup_estep_matches_oracle(ctx, shape):
    case = shape_case(shape)
    _, batch, models, bp, ragged = case
    res, info, got = run_estep(ctx, batch, models, bp, ragged, ESTEP)
    check_workgroup(info, shape["rows"])
    ref = check_oracle(case, res, got, shape_id(shape))
    assert all(np.count_nonzero(r[:60]) == 60 and r[60] < 0 for r in ref)


@pytest.mark.parametrize("width", EDGE_WIDTHS)
def test_bands_at_the_edges_of_the_builds(ctx, width):
    case = edge_case(width)
    _, batch, models, bp, ragged = case
    res, info, got = run_estep(ctx, batch, models, bp, ragged, ESTEP)
    assert info["max_band_width"] == width
    if width <= WV:
        assert info["kernel"] == "systolic" and info["family"] == "wave" and info["cells_per_lane"] == 3, info
    elif width > W8:
        assert info["kernel"] == "general", info
    else:
        check_workgroup(info, build_of(width))
    check_oracle(case, res, got, width)


# edge_reads.VANILLA_FAMILIES: a band that crosses 30 skipped k-mers within a few k-mers of the build's slot period (on
# the fused builds the A-record cases; here the same reads through the ring), and the path on the band's lower edge
WIDE_FAMILIES = [(name % w, build_of(w)) for w in (248, 376, 504) for name in ("varec%d", "vlower%d")]


@pytest.mark.parametrize("name,rows", WIDE_FAMILIES, ids=[n for n, _ in WIDE_FAMILIES])
def test_fast_bands_and_lower_edges(ctx, name, rows):
    case = family_case(name)
    _, batch, models, bp, ragged = case
    res, info, got = run_estep(ctx, batch, models, bp, ragged, ESTEP)
    check_workgroup(info, rows)
    assert info["max_band_width"] == signal_width(batch, batch["e"])
    check_oracle(case, res, got, name)


@pytest.mark.parametrize("rows", [4, 6, 8])
def test_same_batch_on_the_general_kernel(ctx, rows):
    """without the flag the batch runs what it ran before, cpecan_k_generalv, and CPECAN_FLAG_GENERAL_KERNEL wins over
    the flag: the sums of all three within the bar of one another and of the oracle"""
    case = shape_case(shape_of(rows, 1))
    _, batch, models, bp, ragged = case
    res0, info, plain = run_estep(ctx, batch, models, bp, ragged, 0)
    assert info["kernel"] == "general" and build_of(info["max_band_width"]) == rows, info
    res1, info, asked = run_estep(ctx, batch, models, bp, ragged, ESTEP | cp.FLAG_GENERAL_KERNEL)
    assert info["kernel"] == "general" and build_of(info["max_band_width"]) == rows, info
    res2, info, wg = run_estep(ctx, batch, models, bp, ragged, ESTEP)
    check_workgroup(info, rows)
    same_sums(plain, wg)
    same_sums(asked, wg)
    for res, got in ((res0, plain), (res1, asked), (res2, wg)):
        check_oracle(case, res, got, rows)


def test_a_byte_that_is_no_nucleotide_sends_the_batch_to_the_general_kernel(ctx):
    """an N in the middle of the first read of a four-wave shape: with the flag the batch runs where it runs without,
    on cpecan_k_generalv (the reference scores a k-mer that is none as NaN, which only that kernel reproduces), and
    gives the same vectors, a NaN for a NaN"""
    _, batch, _, bp, ragged = shape_case(shape_of(4))
    x = bytearray(batch["x_chars"])
    x[batch["items"][0]["x_offset"] + batch["items"][0]["lX"] // 2] = ord("N")
    batch = dict(batch, x_chars=bytes(x))
    models = vanilla_models(batch)
    _, info0, plain = run_estep(ctx, batch, models, bp, ragged, 0)
    _, info1, flagged = run_estep(ctx, batch, models, bp, ragged, ESTEP)
    for info in (info0, info1):
        assert info["kernel"] == "general" and build_of(info["max_band_width"]) == 4, info
    assert np.any(np.isnan(plain[0])) and np.all(np.isfinite(plain[1]))
    for g, r in zip(flagged, plain):
        assert same_doubles(g, r)


def test_an_item_of_fewer_than_two_kmers_sends_the_batch_to_the_general_kernel(ctx):
    _, batch, _, bp, ragged = shape_case(shape_of(6))
    base = batch["items"][0]
    batch = dict(batch, items=list(batch["items"]) + [dict(base, lX=1, lY=4, n_anchors=0, model=0)])
    upload(ctx, vanilla_models(batch))
    b = ebatch(ctx, batch, bp, ragged, ESTEP)
    info = b.info()
    b.close()
    assert info["kernel"] == "general" and build_of(info["max_band_width"]) == 6, info


def short_items_beside_a_wide_read():
    """vanilla_short_items' batch (two 300 x 600 reads and items of 5 x 0, 3 x 4 and 2 x 6, a model each) and the first
    read of exact_width_batch(300), with a model of its own: its band of 300 k-mers asks for the six-wave build"""
    batch, models = vanilla_short_items()
    wide, bp = exact_width_batch(300)
    it, (match, _, gap_y) = wide["items"][0], wide["models"][0]
    assert it["x_offset"] == 0 and it["y_offset"] == 0 and it["anchor_offset"] == 0
    items = list(batch["items"]) + [dict(it, x_offset=len(batch["x_chars"]), y_offset=len(batch["events"]),
                                         anchor_offset=len(batch["anchors"]), model=len(models))]
    batch = dict(batch, items=items, x_chars=bytes(batch["x_chars"]) + bytes(wide["x_chars"][:it["lX"] + 5]),
                 events=np.concatenate([batch["events"], wide["events"][:it["lY"]]]),
                 anchors=np.concatenate([np.asarray(batch["anchors"]).reshape(-1, 2),
                                         np.asarray(wide["anchors"][:it["n_anchors"]]).reshape(-1, 2)]),
                 models=list(batch["models"]) + [wide["models"][0]])
    return batch, models + [o.VanillaModel(match, skip_bins(3), gap_y)], bp


@pytest.mark.parametrize("ragged", [(1, 1), (0, 0)], ids=["r11", "r00"])
def test_short_items_beside_a_wide_read(ctx, ragged):
    """items of no events, of a few of both and of two k-mers ride on the six-wave build beside a read that needs it"""
    batch, models, bp = short_items_beside_a_wide_read()
    assert [(it["lX"], it["lY"]) for it in batch["items"][2:5]] == [(5, 0), (3, 4), (2, 6)]
    res, info, got = run_estep(ctx, batch, models, bp, ragged, ESTEP)
    check_workgroup(info, 6)
    assert info["max_band_width"] == signal_width(batch, bp.diagonalExpansion)
    ref = check_oracle((("ve-short", ragged), batch, models, bp, ragged), res, got, ragged)
    assert all(np.all(np.isfinite(r)) and r[60] < 0 for r in ref)
    assert np.isclose(ref[2][:60].sum(), 5.0, rtol=1e-12)  # the 5 x 0 item: five gap-X steps


def test_two_items_share_one_model(ctx):
    """both reads of a four-wave shape on the first read's model: the sums of two alignments' workgroups land in one
    block"""
    _, batch, models, bp, ragged = shape_case(shape_of(4, 2))
    assert len(batch["items"]) == 2
    batch = dict(batch, items=[dict(it, model=0) for it in batch["items"]])
    models = models[:1]
    res, info, got = run_estep(ctx, batch, models, bp, ragged, ESTEP)
    check_workgroup(info, 4)
    ref = check_oracle((("ve-shared", 4), batch, models, bp, ragged), res, got, "shared")
    alone = vanilla_oracle(dict(batch, items=batch["items"][:1]), models, bp, ragged)
    assert np.all(np.isfinite(ref[0])) and not np.isclose(ref[0][60], alone[0][60], rtol=1e-3, atol=0)


@pytest.mark.parametrize("rows", [4, 6, 8])
def test_run_twice(ctx, rows):
    case = shape_case(shape_of(rows, 1))
    _, batch, models, bp, ragged = case
    mids = upload(ctx, models)
    b = ebatch(ctx, batch, bp, ragged, ESTEP)
    check_workgroup(b.info(), rows)
    runs = []
    for _ in range(2):
        b.run()
        b.sync()
        runs.append((batch_results(b), [b.expectations(m) for m in mids], b.counts()))
    b.close()
    same_sums(runs[0][1], runs[1][1])  # ... and not doubled
    for first, second in zip(runs[0][2], runs[1][2]):
        assert np.array_equal(first, second)
    for res, got, _ in runs:
        check_oracle(case, res, got, rows)


def test_chained_batches_of_different_classes(ctx):
    """a four-wave and an eight-wave E-step batch run behind one another for three rounds"""
    cases = [shape_case(shape_of(4)), shape_case(shape_of(8))]
    # one model set for both batches: the second batch's model ids follow the first's
    batches, models = [], []
    for _, bt, own, _, _ in cases:
        batches.append(dict(bt, items=[dict(it, model=it["model"] + len(models)) for it in bt["items"]]))
        models += own
    mids = upload(ctx, models)
    bs = [ebatch(ctx, bt, bp, ragged, ESTEP) for bt, (_, _, _, bp, ragged) in zip(batches, cases)]
    for b, rows in zip(bs, (4, 8)):
        check_workgroup(b.info(), rows)
    prev = None
    for _ in range(3):
        for b in bs:
            b.run(after=prev)
            prev = b
    first = 0
    for b, case in zip(bs, cases):
        b.sync()
        n = len(case[2])
        check_oracle(case, batch_results(b), [b.expectations(m) for m in mids[first:first + n]], "chained")
        first += n
    for b in bs:
        b.close()


def test_skip_bins_rewritten_between_two_runs(ctx):
    """ctx.modelsv_set_skip_probs between two runs of one batch: the second run's sums are the oracle's with the new
    bins in every model"""
    shape = shape_of(6, 1)
    case = shape_case(shape)
    _, batch, models, bp, ragged = case
    mids = upload(ctx, models)
    b = ebatch(ctx, batch, bp, ragged, ESTEP)
    check_workgroup(b.info(), 6)
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


def test_environment_switch_in_a_fresh_process(tmp_path):
    """CPECAN_WIDE_BANDS_VANILLA_ESTEP=1 in a fresh child process: a vanilla batch of expectations created with no other
    flag runs a workgroup build and gives the oracle's sums"""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "vanilla_wide_estep_env_child.py")
    e = dict(os.environ, CPECAN_WIDE_BANDS_VANILLA_ESTEP="1")
    path = str(tmp_path / "on.json")
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, child, path], env=e, capture_output=True,
                       text=True, timeout=400)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.load(open(path))
    shape = shape_of(6)
    check_workgroup(out["info"], shape["rows"])
    case = shape_case(shape)
    ref = oracle_sums(*case)
    assert len(out["sums"]) == len(ref)
    for k, (g, r) in enumerate(zip(out["sums"], ref)):
        assert_expectations_match(np.asarray(g), r, ("child", k))

"""The HDP machine's E-step on the workgroup-per-alignment kernels (CPECAN_FLAG_WIDE_BANDS_HDP_ESTEP on an HDP batch
of expectations: six waves per workgroup for bands of 249..376 k-mers, eight for 377..504) against the oracle's HDP
E-step (o.expectations_h_using_anchors) on the reference's own serialized HDP (tests/golden/testTemplate.nhdp), through
the C-ABI.  The bars are test_hdp_gpu.py's: the nine transition sums to rtol 1e-9 / atol 1e-12 (atomic additions of the
same terms in an order that differs from run to run), the likelihood to rtol 1e-12 and non-zero, every read's
event-to-k-mer assignments and their exponents bit-identical and in the reference's order.  Threshold 0.05 unless a
case says otherwise.  Every case asserts its route: without it most of them would pass on the general kernel."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pyoracle as o
from harness import band_params, batch_results, cp, hdp_batch, make_items, trained_transitions, with_gap_switch
from test_band_edges_machines_gpu import cached, read_of
from test_fuzz_expectations_gpu import RAGGED, assert_expectations_match, env
from test_fuzz_expectations_machines_gpu import (assert_same_assignments, hdp_degenerate, hdp_oracle,
                                                 read_with_first_kmer)
from test_hdp_workgroup_gpu import (SCALE, SHAPES, THRESHOLD_ZERO, W8, WV, build_of, check_workgroup, exact_width_batch,
                                    fuzz_batch, fuzz_cases, shape_batch, shape_bp, shape_id, shape_of,
                                    threshold_zero_read)

pytestmark = pytest.mark.gpu

ESTEP = getattr(cp, "FLAG_WIDE_BANDS_HDP_ESTEP", 0)  # (0 before the flag existed: every route assertion then fails)
THR = 0.05  # the machine's posteriors are flat: a low bar gives a few hundred assignments a read


@pytest.fixture(scope="module")
def ctx():
    c = cp.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def nhdp(golden_dir):
    return o.load_nhdp(os.path.join(golden_dir, "testTemplate.nhdp"))


@pytest.fixture(scope="module")
def switch_sets(ctx):
    """the transition sets of test_gap_switch_gpu.py: a strong gap Y -> gap X switch and a trained (tiny) one"""
    trained, _ = trained_transitions(ctx)
    return dict(strong=with_gap_switch(cp.NANOPORE_TRANSITIONS, 0.1), trained=trained)


def upload(ctx, nhdp, ts):
    ctx.models_clear()
    return ctx.modelsh_create([(t, nhdp["alphabet"], nhdp["grid"], nhdp["y"], nhdp["slope"], nhdp["kmer_row"])
                               for t in ts])


def ebatch(ctx, batch, bp, ragged, flags):
    return cp.Batch(ctx, make_items(batch, ragged), batch["x_chars"], batch["events"], batch["anchors"], bp,
                    flags=cp.FLAG_EXPECTATIONS | flags, hdp=True)


def results(b, mids):
    """(per-item results: the assignments as pairs; per-model vectors of nine sums and the likelihood)"""
    return batch_results(b), [b.expectations(m) for m in mids]


def run_estep(ctx, nhdp, batch, bp, ragged, flags, ts=(cp.NANOPORE_TRANSITIONS,)):
    """(per-item results, info(), per-model vectors) of one HDP batch of expectations"""
    mids = upload(ctx, nhdp, ts)
    b = ebatch(ctx, batch, bp, ragged, flags)
    info = b.info()
    b.run()
    b.sync()
    res, got = results(b, mids)
    b.close()
    return res, info, got


def check_oracle(key, res, got, batch, models, bp, ragged, what, read_of=read_of):
    """every model's ten sums and every read's assignments against the oracle's E-step of each read alone"""
    reads, ref = cached(("he",) + key, lambda: hdp_oracle(batch, models, bp, ragged, read_of))
    assert len(got) == len(ref)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert_expectations_match(g, r, (what, k))
    assert_same_assignments(res, reads, what)
    return reads, ref


def same_lists(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(x["triples"], y["triples"])
        assert np.array_equal(np.asarray(x["logp"]).view(np.uint64), np.asarray(y["logp"]).view(np.uint64))


def same_sums(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.allclose(x[:9], y[:9], rtol=1e-9, atol=1e-12)
        assert np.isclose(x[9], y[9], rtol=1e-12, atol=0) and x[9] != 0.0


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_hdp_workgroup_estep_matches_oracle(ctx, nhdp, shape):
    batch = shape_batch(shape, nhdp)
    bp = shape_bp(shape, THR)
    res, info, got = run_estep(ctx, nhdp, batch, bp, shape["ragged"], ESTEP)
    check_workgroup(info, shape["rows"])
    for it in batch["items"]:
        assert (it["lX"] + it["lY"]) // shape["md"] >= 3  # several traceback windows
    _, ref = check_oracle(("shape", shape["seed"]), res, got, batch, [o.HdpModel(nhdp)], bp, shape["ragged"],
                          shape_id(shape))
    assert ref[0][9] != 0.0
    assert sum(len(r["triples"]) for r in res) > 50


@pytest.mark.parametrize("rows", [6, 8])
def test_same_batch_on_the_general_kernel(ctx, nhdp, rows):
    """without the flag the batch runs what it ran before, cpecan_k_generalh: the same assignments bit for bit, the
    sums within the bound"""
    shape = shape_of(rows, 1)
    batch = shape_batch(shape, nhdp)
    bp = shape_bp(shape, THR)
    gen, info, gsum = run_estep(ctx, nhdp, batch, bp, shape["ragged"], 0)
    assert info["kernel"] == "general" and build_of(info["max_band_width"]) == rows, info
    wg, info, wsum = run_estep(ctx, nhdp, batch, bp, shape["ragged"], ESTEP)
    check_workgroup(info, rows)
    same_lists(gen, wg)
    same_sums(gsum, wsum)
    assert sum(len(r["triples"]) for r in wg) > 50


@pytest.mark.parametrize("place", ["upper", "lower"])
@pytest.mark.parametrize("width", [248, 249, 376, 377, 504, 505])
def test_bands_at_the_edges_of_the_builds(ctx, nhdp, width, place):
    model = o.HdpModel(nhdp)
    batch, _ = exact_width_batch(width, place, (nhdp, model))
    bp = band_params(THR, 150, 40, batch["e"])
    ragged = (width % 2, 1)
    res, info, got = run_estep(ctx, nhdp, batch, bp, ragged, ESTEP)
    assert info["max_band_width"] == width
    if width <= WV:
        assert info["kernel"] == "systolic" and info["family"] == "wave" and info["cells_per_lane"] == 4, info
    elif width > W8:
        assert info["kernel"] == "general", info
    else:
        check_workgroup(info, build_of(width))
    check_oracle(("edge", width, place), res, got, batch, [model], bp, ragged, (width, place))
    assert sum(len(r["triples"]) for r in res) > 50


@pytest.mark.parametrize("name", ["strong", "trained"])
@pytest.mark.parametrize("rows", [6, 8])
def test_switch_transition_matches_oracle(ctx, nhdp, switch_sets, rows, name):
    """a finite gap Y -> gap X switch: the ninth sum is no longer zero"""
    t = switch_sets[name]
    assert np.isfinite(t[7])
    shape = shape_of(rows, 2)
    batch = shape_batch(shape, nhdp)
    bp = shape_bp(shape, THR)
    res, info, got = run_estep(ctx, nhdp, batch, bp, (1, 1), ESTEP, ts=[t])
    check_workgroup(info, rows)
    _, ref = check_oracle(("switch", name, shape["seed"]), res, got, batch, [o.HdpModel(nhdp, transitions=t)], bp,
                          (1, 1), (rows, name))
    assert ref[0][2 * 3 + 1] > 0.0  # gap Y -> gap X is taken
    if name == "strong":  # the switch moves the likelihood far past its bound: a pass that drops the term cannot pass
        _, plain = cached(("he", "switch-plain", shape["seed"]),
                          lambda: hdp_oracle(batch, [o.HdpModel(nhdp)], bp, (1, 1)))
        assert not np.isclose(plain[0][9], ref[0][9], rtol=1e-6, atol=0)


@pytest.mark.parametrize("rows", [6, 8])
def test_two_models_in_one_batch(ctx, nhdp, rows):
    """reads alternate between two models with different transitions: each model's ten sums are the oracle's on that
    model's reads alone"""
    shape = shape_of(rows, 1)
    batch = shape_batch(shape, nhdp)
    batch = dict(batch, items=[dict(it, model=i % 2) for i, it in enumerate(batch["items"])])
    assert len(batch["items"]) == 3
    ts = [cp.NANOPORE_TRANSITIONS, with_gap_switch(cp.NANOPORE_TRANSITIONS, 0.1)]
    bp = shape_bp(shape, THR)
    res, info, got = run_estep(ctx, nhdp, batch, bp, shape["ragged"], ESTEP, ts=ts)
    check_workgroup(info, rows)
    _, ref = check_oracle(("two", shape["seed"]), res, got, batch, [o.HdpModel(nhdp, transitions=t) for t in ts], bp,
                          shape["ragged"], rows)
    assert ref[0][7] == 0.0 and ref[1][7] > 0.0 and ref[0][9] != ref[1][9]


def degenerate_beside_a_wide_read(rows, nhdp):
    """hdp_degenerate's items (two 300 x 600 reads and the five degenerate shapes), one read with a single anchor whose
    band is the whole matrix (THRESHOLD_ZERO's) and a read of 30 k-mers, each with a model of its own"""
    deg, _ = hdp_degenerate(nhdp)
    lX, e = THRESHOLD_ZERO[rows]
    parts = [hdp_batch(70 + rows, 1, lX, lX, nhdp)[0], hdp_batch(170 + rows, 1, 30, 10, nhdp)[0]]
    x = deg["x_chars"].decode() if isinstance(deg["x_chars"], bytes) else deg["x_chars"]
    events, anchors, items = [np.asarray(deg["events"])], [np.asarray(deg["anchors"]).reshape(-1, 2)], list(deg["items"])
    for p in parts:
        items.append(dict(p["items"][0], x_offset=len(x), y_offset=sum(len(v) for v in events),
                          anchor_offset=sum(len(v) for v in anchors), model=len(items)))
        x += p["x_chars"]
        events.append(p["events"])
        anchors.append(p["anchors"])
    batch = dict(x_chars=x, events=np.concatenate(events), anchors=np.concatenate(anchors), items=items)
    return batch, band_params(THR, 100, 40, e)


@pytest.mark.parametrize("ragged", RAGGED, ids=["r%d%d" % r for r in RAGGED])
@pytest.mark.parametrize("rows", [6, 8])
def test_degenerate_items_beside_a_wide_read(ctx, nhdp, rows, ragged):
    """items of 0 x 0, 0 x 5, 5 x 0, 1 x 1 and 3 x 4 and a read that ends inside its first traceback window in a batch
    whose widest band asks for the build, held to the oracle as test_hdp_degenerate_items_expectations holds them (an
    item without k-mers is scored with the k-mer that starts at its offset)"""
    batch, bp = degenerate_beside_a_wide_read(rows, nhdp)
    short = batch["items"][-1]
    assert short["lX"] == 30 and short["lX"] + short["lY"] < bp.minDiagsBetweenTraceBack
    models = [o.HdpModel(nhdp) for _ in batch["items"]]
    res, info, got = run_estep(ctx, nhdp, batch, bp, ragged, ESTEP, ts=[cp.NANOPORE_TRANSITIONS] * len(models))
    check_workgroup(info, rows)
    reads, ref = check_oracle(("degenerate", rows, ragged), res, got, batch, models, bp, ragged, (rows, ragged),
                              read_with_first_kmer)
    assert len(reads[-1]["assign"]) > 5 and len(reads[-2]["assign"]) > 50
    assert all(np.all(np.isfinite(v)) for v in ref)


@pytest.mark.parametrize("rows", [6, 8])
def test_assignment_overflow_reruns(ctx, nhdp, rows):
    """more assignments than the item's first allocation -- pairCapFactor (16 for the HDP machine) per element of
    lX + lY, plus 64 (plan_bands, cpecan_hip.hip) -- so the batch is run once more with the counted sizes: the lists
    are the oracle's and the sums are not doubled.  1e-4 is the largest power of ten at which the oracle's count of
    either read exceeds the allocation (8 367 / 12 483 assignments at 1e-3 / 1e-4 against 10 448 on the six-wave
    read, 13 082 / 19 894 against 14 560 on the eight-wave one)."""
    batch, model, bp0 = threshold_zero_read(rows, nhdp)
    bp = band_params(1e-4, 200, 40, bp0.diagonalExpansion)
    it = batch["items"][0]
    reads, _ = cached(("he", "overflow", rows), lambda: hdp_oracle(batch, [model], bp, (1, 1)))
    assert len(reads[0]["assign"]) > 16 * (it["lX"] + it["lY"]) + 64
    res, info, got = run_estep(ctx, nhdp, batch, bp, (1, 1), ESTEP)
    check_workgroup(info, rows)
    check_oracle(("overflow", rows), res, got, batch, [model], bp, (1, 1), rows)


@pytest.mark.parametrize("rows", [6, 8])
def test_run_twice(ctx, nhdp, rows):
    shape = shape_of(rows, 1)
    batch = shape_batch(shape, nhdp)
    bp = shape_bp(shape, THR)
    mids = upload(ctx, nhdp, [cp.NANOPORE_TRANSITIONS])
    b = ebatch(ctx, batch, bp, shape["ragged"], ESTEP)
    check_workgroup(b.info(), rows)
    runs = []
    for _ in range(2):
        b.run()
        b.sync()
        runs.append(results(b, mids) + (b.counts(),))
    b.close()
    same_lists(runs[0][0], runs[1][0])
    same_sums(runs[0][1], runs[1][1])
    for first, second in zip(runs[0][2], runs[1][2]):
        assert np.array_equal(first, second)
    check_oracle(("shape", shape["seed"]), runs[1][0], runs[1][1], batch, [o.HdpModel(nhdp)], bp, shape["ragged"], rows)


def test_chained_batches_equal_their_stand_alone_results(ctx, nhdp):
    """an E-step batch of each build, on a context each, run behind one another twice"""
    shapes = [shape_of(6, 1), shape_of(8, 1)]
    batches = [shape_batch(s, nhdp) for s in shapes]
    alone = [run_estep(ctx, nhdp, bt, shape_bp(s, THR), s["ragged"], ESTEP) for bt, s in zip(batches, shapes)]
    other = cp.Context(0)
    try:
        ctxs = [ctx, other]
        mids = [upload(c, nhdp, [cp.NANOPORE_TRANSITIONS]) for c in ctxs]
        bs = [ebatch(c, bt, shape_bp(s, THR), s["ragged"], ESTEP) for c, bt, s in zip(ctxs, batches, shapes)]
        for b, s in zip(bs, shapes):
            check_workgroup(b.info(), s["rows"])
        prev = None
        for _ in range(2):
            for b in bs:
                b.run(after=prev)
                prev = b
        for b, m, (res, _, got) in zip(bs, mids, alone):
            b.sync()
            chained, sums = results(b, m)
            same_lists(res, chained)
            same_sums(got, sums)
        for b in bs:
            b.close()
    finally:
        other.close()


@pytest.mark.parametrize("rows", [6, 8])
def test_event_means_off_the_grid_match_oracle(ctx, nhdp, rows):
    """test_hdp_workgroup_gpu.test_event_means_off_the_grid_match_oracle's construction -- means below the grid's
    first point, above its last, and exactly on both -- against the oracle's E-step"""
    shape = shape_of(rows, 2)
    batch = shape_batch(shape, nhdp)
    grid = np.asarray(nhdp["grid"])
    ev = np.array(batch["events"], copy=True)
    rng = np.random.default_rng(500 + rows)
    idx = rng.choice(len(ev), size=len(ev) // 8, replace=False)
    off = np.concatenate([grid[0] - rng.uniform(0.0, 20.0, len(idx) // 2),
                          grid[-1] + rng.uniform(0.0, 20.0, len(idx) - len(idx) // 2)])
    off[0], off[-1] = grid[0], grid[-1]
    ev[idx, 0] = off
    batch = dict(batch, events=ev)
    assert np.count_nonzero(ev[:, 0] <= grid[0]) >= 20 and np.count_nonzero(ev[:, 0] >= grid[-1]) >= 20
    bp = shape_bp(shape, THR)
    res, info, got = run_estep(ctx, nhdp, batch, bp, shape["ragged"], ESTEP)
    check_workgroup(info, rows)
    check_oracle(("offgrid", rows), res, got, batch, [o.HdpModel(nhdp)], bp, shape["ragged"], rows)
    assert sum(len(r["triples"]) for r in res) > 50


@pytest.mark.parametrize("rows", [6, 8])
def test_a_column_that_is_no_kmer(ctx, nhdp, rows):
    """A character outside the alphabet makes the six k-mers that contain it no k-mers.  The oracle answers NaN there
    and is not the reference of that read (test_hdp_workgroup_gpu.test_a_column_that_is_no_kmer_scores_minus_infinity);
    the builds score such a column -inf as match and as gap-Y emission.  What follows and is asserted: the read's ten
    sums stay finite, none of its assignments lies in one of the six columns, there are assignments on both sides of
    them, and the other read of the batch (a model of its own) equals its clean results."""
    shape = shape_of(rows, 2)
    batch = shape_batch(shape, nhdp)
    batch = dict(batch, items=[dict(it, model=i) for i, it in enumerate(batch["items"])])
    it = batch["items"][0]
    p = it["x_offset"] + it["lX"] // 2
    bad = dict(batch, x_chars=batch["x_chars"][:p] + "N" + batch["x_chars"][p + 1:])
    bp = shape_bp(shape, THR)
    ts = [cp.NANOPORE_TRANSITIONS] * len(batch["items"])
    res, info, got = run_estep(ctx, nhdp, bad, bp, shape["ragged"], ESTEP, ts=ts)
    check_workgroup(info, rows)
    k0, k1 = it["lX"] // 2 - 5, it["lX"] // 2  # the k-mers (assignment coordinate x) that contain the character
    assert np.all(np.isfinite(got[0])) and got[0][9] != 0.0
    x = np.asarray(res[0]["triples"])[:, 1]
    assert not np.any((x >= k0) & (x <= k1))
    assert np.any(x < k0) and np.any(x > k1)
    assert np.all(np.isfinite(res[0]["logp"]))
    reads, ref = cached(("he", "clean", rows),
                        lambda: hdp_oracle(batch, [o.HdpModel(nhdp) for _ in ts], bp, shape["ragged"]))
    assert len(res) > 1
    for i in range(1, len(res)):
        assert_expectations_match(got[i], ref[i], (rows, i))
    assert_same_assignments(res[1:], reads[1:], rows)


def test_fuzz_hdp_wide_estep(ctx, nhdp):
    """the posterior fuzz test's cases (test_hdp_workgroup_gpu.fuzz_cases), a threshold of 0.0 replaced by 0.05, every
    item held to the oracle whatever the batch runs on; the counts per build depend on the band table alone, which
    the mode does not change (tests/tools/hdp_wide_shapes.py prints them)"""
    cases = fuzz_cases(24 * SCALE)
    model = o.HdpModel(nhdp)
    ran = {6: 0, 8: 0}
    mids = upload(ctx, nhdp, [cp.NANOPORE_TRANSITIONS])
    for c in cases:
        batch = fuzz_batch(c, nhdp)
        bp = band_params(c["thr"] if c["thr"] > 0.0 else THR, c["md"], c["tb"], c["e"])
        b = ebatch(ctx, batch, bp, c["ragged"], ESTEP)
        b.run()
        b.sync()
        res, got = results(b, mids)
        info = b.info()
        b.close()
        rows = build_of(info["max_band_width"])
        if rows is not None:  # (a case whose band came out narrower or wider is compared all the same)
            check_workgroup(info, rows)
            ran[rows] += 1
        print("fuzz case", c["seed"], info)
        check_oracle(("fuzz", c["seed"]), res, got, batch, [model], bp, c["ragged"], c["seed"])
    # at most a quarter of the cases outside the two builds, at least eight on each
    assert 4 * (len(cases) - sum(ran.values())) <= len(cases), ran
    assert min(ran.values()) >= 8, ran


def test_environment_switch_in_a_fresh_process(tmp_path):
    """CPECAN_WIDE_BANDS_HDP_ESTEP=1 in a fresh child process: an HDP batch of expectations created with no other flag
    runs a workgroup build and returns the assignments it returns without the variable (there on the general kernel)"""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hdp_wide_estep_env_child.py")
    out = {}
    for name, value in (("off", None), ("on", "1")):
        e = {k: v for k, v in os.environ.items() if k != "CPECAN_WIDE_BANDS_HDP_ESTEP"}
        if value is not None:
            e["CPECAN_WIDE_BANDS_HDP_ESTEP"] = value
        path = str(tmp_path / (name + ".json"))
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, child, path], env=e, capture_output=True,
                           text=True, timeout=400)
        assert r.returncode == 0, r.stderr[-2000:]
        out[name] = json.load(open(path))
    rows = build_of(out["off"]["info"]["max_band_width"])
    assert out["off"]["info"]["kernel"] == "general" and rows is not None
    check_workgroup(out["on"]["info"], rows)
    assert len(out["on"]["assign"]) > 50
    assert out["on"]["assign"] == out["off"]["assign"] and out["on"]["logp"] == out["off"]["logp"]
    same_sums([np.asarray(out["off"]["sums"])], [np.asarray(out["on"]["sums"])])


def test_host_library_reaches_the_builds_through_the_variable(golden_dir, nhdp):
    """cpecan_getHdpExpectationsUsingAnchors (libcpecan_host.so) on one read whose diagonalExpansion makes its band 300
    k-mers wide, without and with CPECAN_WIDE_BANDS_HDP_ESTEP=1: the same assignments, the transitions within the
    bound.  The route cannot be observed through that interface (the batch is the library's own); that the variable
    routes such a batch is test_environment_switch_in_a_fresh_process's, and the dispatch tests', to show."""
    import host_api as h
    L = h.lib()
    batch, _ = hdp_batch(91, 1, 299, 299, nhdp)  # a single anchor: the band is the whole matrix
    it = batch["items"][0]
    e = 280
    bl, br = cp.band_construct(batch["anchors"], it["lX"], it["lY"], e)
    assert int(((br - bl) // 2 + 1).max()) == 300
    nh = L.deserialize_nhdp(os.path.join(golden_dir, "testTemplate.nhdp").encode())
    sm = L.getHdpStateMachine3(nh)
    ev = np.ascontiguousarray(np.asarray(batch["events"], np.float64).reshape(-1))
    xbuf = C.create_string_buffer(batch["x_chars"].encode())
    sX = L.sequence_construct2(it["lX"], C.cast(xbuf, C.c_void_p), h.fn_ptr("sequence_getKmer3"),
                               h.fn_ptr("sequence_sliceNucleotideSequence2"))
    sY = L.sequence_construct2(ev.size // 3, ev.ctypes.data_as(C.c_void_p), h.fn_ptr("sequence_getEvent"),
                               h.fn_ptr("sequence_sliceEventSequence2"))
    p = L.pairwiseAlignmentBandingParameters_construct()
    p.contents.minDiagsBetweenTraceBack = 200
    p.contents.diagonalExpansion = e
    lst = h.make_anchor_list([tuple(int(v) for v in a) for a in batch["anchors"]])
    got = {}
    for name, value in (("off", None), ("on", "1")):
        with env(CPECAN_WIDE_BANDS_HDP_ESTEP=value):
            hmm = L.cpecan_hdpExpectations_construct(0.0, THR)
            L.cpecan_getHdpExpectationsUsingAnchors(sm, hmm, sX, sY, lst, p, True, True)
        r = hmm.contents
        n = r.numberOfAssignments
        got[name] = dict(t=np.array(list(r.transitions)), lik=r.likelihood, n=n,
                         kmers=[r.kmerAssignments[i * 7:i * 7 + 6] for i in range(n)],
                         events=[r.eventAssignments[i] for i in range(n)])
        L.cpecan_hdpExpectations_destruct(hmm)
    L.stList_destruct(lst)
    L.sequence_sequenceDestroy(sX)
    L.sequence_sequenceDestroy(sY)
    L.pairwiseAlignmentBandingParameters_destruct(p)
    L.stateMachine_destruct(sm)
    L.destroy_nanopore_hdp(nh)
    assert got["on"]["n"] == got["off"]["n"] and got["on"]["n"] > 50
    assert got["on"]["kmers"] == got["off"]["kmers"] and got["on"]["events"] == got["off"]["events"]
    assert np.allclose(got["on"]["t"], got["off"]["t"], rtol=1e-9, atol=1e-12)
    assert np.isclose(got["on"]["lik"], got["off"]["lik"], rtol=1e-12, atol=0) and got["off"]["lik"] != 0.0
    want = o.expectations_h_using_anchors(o.HdpModel(nhdp), [(batch["x_chars"], it["lX"], batch["events"],
                                                              batch["anchors"])],
                                          o.default_params(minDiagsBetweenTraceBack=200, diagonalExpansion=e), THR,
                                          True, True)
    assert np.allclose(got["on"]["t"], want["transitions"], rtol=1e-9, atol=1e-12)
    assert got["on"]["n"] == len(want["assign"])

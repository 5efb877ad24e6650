"""The HDP signal machine on the workgroup-per-alignment kernels (CPECAN_FLAG_WIDE_BANDS_HDP on an HDP posterior batch:
six waves per workgroup for bands of 249..376 k-mers, eight for 377..504) against the oracle's HDP machine on the
reference's own serialized HDP (tests/golden/testTemplate.nhdp), through the C-ABI: cells, totalProbability refreshes
and posterior exponents bit-identical, pairs in the reference's emission order -- and the dispatch around them: nothing
changes without the flag, with CPECAN_FLAG_WIDE_BANDS, at 248 k-mers and below, past 504, with
CPECAN_FLAG_GENERAL_KERNEL, un-banded, and for the E-step, which stays on the general kernel."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import edge_reads
import pyoracle as o
from harness import (assert_same_pairs, band_params, batch_results, cp, hdp_batch, make_items, orc_params,
                     run_oracle_hdp_item, trained_transitions, with_gap_switch)

pytestmark = pytest.mark.gpu

WIDE = getattr(cp, "FLAG_WIDE_BANDS_HDP", 0)  # (0 before the flag existed: every route assertion below then fails)
# the widest band of the HDP wave builds, then of the six- and eight-wave workgroup builds
WV, W6, W8 = 248, 376, 504
SCALE = max(1, int(os.environ.get("CPECAN_FUZZ_SCALE", "1")))


@pytest.fixture(scope="module")
def ctx():
    c = cp.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def nhdp(golden_dir):
    return o.load_nhdp(os.path.join(golden_dir, "testTemplate.nhdp"))


def build_of(width):
    """waves per workgroup of the HDP workgroup build that takes a band of `width` k-mers (None: not one of them)"""
    return 6 if WV < width <= W6 else 8 if W6 < width <= W8 else None


def upload(ctx, nhdp, transitions=None):
    ctx.models_clear()
    t = cp.NANOPORE_TRANSITIONS if transitions is None else transitions
    return ctx.modelsh_create([(t, nhdp["alphabet"], nhdp["grid"], nhdp["y"], nhdp["slope"], nhdp["kmer_row"])])


def hbatch(ctx, batch, bp, ragged, flags):
    return cp.Batch(ctx, make_items(batch, ragged), batch["x_chars"], batch["events"], batch["anchors"], bp, flags=flags,
                    hdp=True)


def run_hdp(ctx, nhdp, batch, bp, ragged, flags, transitions=None):
    upload(ctx, nhdp, transitions)
    b = hbatch(ctx, batch, bp, ragged, flags)
    b.run()
    b.sync()
    return batch_results(b), b


_ORACLE = {}


def oracle_results(key, batch, bp, model, ragged):
    """the oracle's results of every item of a batch, computed once per (batch, band parameters, ragged ends, model)"""
    key = (key, bp.threshold, bp.minDiagsBetweenTraceBack, bp.traceBackDiagonals, bp.diagonalExpansion, ragged)
    if key not in _ORACLE:
        _ORACLE[key] = [run_oracle_hdp_item(batch, i, bp, model, ragged) for i in range(len(batch["items"]))]
    return _ORACLE[key]


def check_oracle(res, refs):
    assert len(res) == len(refs)
    for i, (g, ref) in enumerate(zip(res, refs)):
        assert g["cells"] == ref["cells"], i
        assert np.array_equal(g["totals_xay"], ref["totals_xay"]), i
        assert np.array_equal(g["totals"], ref["totals"]), i
        assert_same_pairs(g, ref)
        assert len(g["triples"]) > 0


def check_workgroup(info, rows):
    assert info["kernel"] == "systolic" and info["family"] == "workgroup", info
    assert info["waves_per_workgroup"] == rows, info
    assert build_of(info["max_band_width"]) == rows, info  # the inputs are of the class they were chosen for
    assert info["assembly_sweeps"] == 0 and info["fused_expectations"] == 0, info


def same_results(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        for key in ("triples", "logp", "totals_xay", "totals"):
            assert np.array_equal(x[key], y[key]), key
        assert x["cells"] == y["cells"]


# sparse anchors and a wide expansion: every shape spans at least three traceback windows (md diagonals apart); the
# widths were checked with cpecan_band_construct on the CPU (tests/tools/hdp_wide_shapes.py prints them).  ls: the
# reads' k-mers (events follow from hdp_batch: about 1.2 per k-mer), one read or several of different lengths
SHAPES = [
    dict(rows=6, seed=31, ls=(340,), every=340, e=160, md=200, tb=40, ragged=(0, 0)),
    dict(rows=6, seed=32, ls=(600, 450, 520), every=250, e=100, md=300, tb=40, ragged=(1, 1)),
    dict(rows=6, seed=33, ls=(500, 560), every=300, e=120, md=150, tb=30, ragged=(0, 1)),
    dict(rows=8, seed=34, ls=(640,), every=400, e=160, md=300, tb=40, ragged=(1, 0)),
    dict(rows=8, seed=35, ls=(800, 650, 720), every=350, e=120, md=250, tb=20, ragged=(1, 1)),
    dict(rows=8, seed=36, ls=(700, 760), every=400, e=160, md=150, tb=40, ragged=(0, 0)),
]


def reads_batch(seed, ls, every, nhdp):
    """hdp_batch's reads, one call per read length, joined into one batch (model 0 shared)"""
    parts = [hdp_batch(seed * 10 + k, 1, lX, every, nhdp)[0] for k, lX in enumerate(ls)]
    items, xo, yo, ao = [], 0, 0, 0
    for p in parts:
        it = dict(p["items"][0], x_offset=xo, y_offset=yo, anchor_offset=ao)
        items.append(it)
        xo += len(p["x_chars"])
        yo += len(p["events"])
        ao += len(p["anchors"])
    return dict(x_chars="".join(p["x_chars"] for p in parts), events=np.concatenate([p["events"] for p in parts]),
                anchors=np.concatenate([p["anchors"] for p in parts]), items=items)


def shape_batch(s, nhdp):
    return reads_batch(s["seed"], s["ls"], s["every"], nhdp)


def shape_bp(s, thr=0.01):
    return band_params(thr, s["md"], s["tb"], s["e"])


def shape_id(s):
    return "h%d-seed%d" % (s["rows"], s["seed"])


def shape_of(rows, k=0):
    return [s for s in SHAPES if s["rows"] == rows][k]


def shape_refs(s, batch, nhdp):
    return oracle_results(("shape", s["seed"]), batch, shape_bp(s), o.HdpModel(nhdp), s["ragged"])


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_hdp_workgroup_posterior_matches_oracle(ctx, nhdp, shape):
    batch = shape_batch(shape, nhdp)
    res, b = run_hdp(ctx, nhdp, batch, shape_bp(shape), shape["ragged"], WIDE)
    check_workgroup(b.info(), shape["rows"])
    for it in batch["items"]:
        assert (it["lX"] + it["lY"]) // shape["md"] >= 3  # several traceback windows
    check_oracle(res, shape_refs(shape, batch, nhdp))
    b.close()


def test_shapes_cover_what_the_issue_asks():
    """(no device) a single read and several reads of different lengths on each build, every ragged-end pair"""
    for rows in (6, 8):
        own = [s for s in SHAPES if s["rows"] == rows]
        assert len(own) >= 3
        assert any(len(s["ls"]) == 1 for s in own) and any(len(set(s["ls"])) > 1 for s in own)
    assert {s["ragged"] for s in SHAPES} == {(0, 0), (1, 0), (0, 1), (1, 1)}


def exact_width_batch(width, place, hdp):
    """two reads whose path runs on the band's `place` edge, the first one's widest band exactly `width` k-mers (the
    other's at most that), as edge_reads builds its w... families"""
    batch = edge_reads.edge_batch(1, 2, 700, 1050, place, every=1, e=40, width=width, hdp=hdp)
    return batch, band_params(0.01, 150, 40, batch["e"])


@pytest.mark.parametrize("place", ["upper", "lower"])
@pytest.mark.parametrize("width", [248, 249, 376, 377, 504, 505])
def test_bands_at_the_edges_of_the_builds(ctx, nhdp, width, place):
    model = o.HdpModel(nhdp)
    batch, bp = exact_width_batch(width, place, (nhdp, model))
    ragged = (width % 2, 1)
    res, b = run_hdp(ctx, nhdp, batch, bp, ragged, WIDE)
    info = b.info()
    assert info["max_band_width"] == width
    if width <= WV:
        assert info["kernel"] == "systolic" and info["family"] == "wave" and info["cells_per_lane"] == 4, info
    elif width > W8:
        assert info["kernel"] == "general", info
    else:
        check_workgroup(info, build_of(width))
    check_oracle(res, oracle_results(("edge", width, place), batch, bp, model, ragged))
    b.close()


@pytest.mark.parametrize("rows", [6, 8])
def test_general_kernel_flag_wins_and_results_are_bit_equal(ctx, nhdp, rows):
    """CPECAN_FLAG_GENERAL_KERNEL beside the flag runs cpecan_k_generalh; the workgroup build gives the same doubles"""
    shape = shape_of(rows, 1)
    batch = shape_batch(shape, nhdp)
    gen, b0 = run_hdp(ctx, nhdp, batch, shape_bp(shape), shape["ragged"], WIDE | cp.FLAG_GENERAL_KERNEL)
    assert b0.info()["kernel"] == "general", b0.info()
    b0.close()
    wg, b1 = run_hdp(ctx, nhdp, batch, shape_bp(shape), shape["ragged"], WIDE)
    check_workgroup(b1.info(), rows)
    b1.close()
    same_results(gen, wg)


@pytest.fixture(scope="module")
def switch_sets(ctx):
    """the transition sets of test_gap_switch_gpu.py: a strong gap Y -> gap X switch and a trained (tiny) one"""
    trained, _ = trained_transitions(ctx)
    return dict(strong=with_gap_switch(cp.NANOPORE_TRANSITIONS, 0.1), trained=trained)


@pytest.mark.parametrize("name", ["strong", "trained"])
@pytest.mark.parametrize("rows", [6, 8])
def test_switch_transition_matches_oracle(ctx, nhdp, switch_sets, rows, name):
    t = switch_sets[name]
    assert np.isfinite(t[7])
    shape = shape_of(rows, 2)
    batch = shape_batch(shape, nhdp)
    model = o.HdpModel(nhdp, transitions=t)
    res, b = run_hdp(ctx, nhdp, batch, shape_bp(shape), (1, 1), WIDE, transitions=t)
    check_workgroup(b.info(), rows)
    check_oracle(res, oracle_results(("switch", name, shape["seed"]), batch, shape_bp(shape), model, (1, 1)))
    if name == "strong":  # the switch moves every total: a sweep that drops the term cannot pass
        plain = oracle_results(("shape11", shape["seed"]), batch, shape_bp(shape), o.HdpModel(nhdp), (1, 1))
        assert not np.any(np.asarray(plain[0]["totals"]) == np.asarray(res[0]["totals"]))
    b.close()


# one read with a single anchor, (k-mers, expansion): the band is the whole matrix, its k-mers set the class
THRESHOLD_ZERO = {6: (300, 280), 8: (420, 420)}


def threshold_zero_read(rows, nhdp):
    lX, e = THRESHOLD_ZERO[rows]
    batch, model = hdp_batch(70 + rows, 1, lX, lX, nhdp)
    return batch, model, band_params(0.0, 200, 40, e)


@pytest.mark.parametrize("rows", [6, 8])
def test_threshold_zero_overflows_and_reruns(ctx, nhdp, rows):
    # every cell of the band with x, y > 0 is a pair: far more than the first pair allocation (16 per element of
    # lX + lY, plus 64), so the batch is re-run with the counted sizes
    batch, model, bp = threshold_zero_read(rows, nhdp)
    res, b = run_hdp(ctx, nhdp, batch, bp, (1, 1), WIDE)
    check_workgroup(b.info(), rows)
    it = batch["items"][0]
    assert len(res[0]["triples"]) > 16 * (it["lX"] + it["lY"]) + 64
    check_oracle(res, oracle_results(("thr0", rows), batch, bp, model, (1, 1)))
    b.close()


@pytest.mark.parametrize("rows", [6, 8])
def test_run_twice_gives_the_same_arrays(ctx, nhdp, rows):
    shape = shape_of(rows, 1)
    batch = shape_batch(shape, nhdp)
    first, b = run_hdp(ctx, nhdp, batch, shape_bp(shape), shape["ragged"], WIDE)
    check_workgroup(b.info(), rows)
    b.run()
    b.sync()
    same_results(first, batch_results(b))
    check_oracle(first, shape_refs(shape, batch, nhdp))
    b.close()


def test_chained_batches_equal_their_stand_alone_results(ctx, nhdp):
    shapes = [shape_of(6, 1), shape_of(8, 1)]
    batches = [shape_batch(s, nhdp) for s in shapes]
    alone = []
    for s, bt in zip(shapes, batches):
        res, b = run_hdp(ctx, nhdp, bt, shape_bp(s), s["ragged"], WIDE)
        alone.append(res)
        b.close()
    upload(ctx, nhdp)
    bs = [hbatch(ctx, bt, shape_bp(s), s["ragged"], WIDE) for bt, s in zip(batches, shapes)]
    for b, s in zip(bs, shapes):
        check_workgroup(b.info(), s["rows"])
    prev = None
    for _ in range(2):
        for b in bs:
            b.run(after=prev)
            prev = b
    for b, res in zip(bs, alone):
        b.sync()
        same_results(res, batch_results(b))
    for b in bs:
        b.close()


@pytest.mark.parametrize("rows", [6, 8])
def test_what_the_flag_does_not_change(ctx, nhdp, rows):
    """no flag, CPECAN_FLAG_WIDE_BANDS alone and the flag on an un-banded batch: the general kernel, the results of the
    same batch without any flag"""
    shape = shape_of(rows, 0)
    batch = shape_batch(shape, nhdp)
    bp = shape_bp(shape)
    plain, b = run_hdp(ctx, nhdp, batch, bp, shape["ragged"], 0)
    info = b.info()
    assert info["kernel"] == "general" and build_of(info["max_band_width"]) == rows, info
    b.close()
    check_oracle(plain, shape_refs(shape, batch, nhdp))
    other, b = run_hdp(ctx, nhdp, batch, bp, shape["ragged"], cp.FLAG_WIDE_BANDS)
    assert b.info()["kernel"] == "general", b.info()
    b.close()
    same_results(plain, other)
    # un-banded: the full matrix, one total, with and without the flag
    unb0, b = run_hdp(ctx, nhdp, batch, bp, shape["ragged"], cp.FLAG_UNBANDED)
    assert b.info()["kernel"] == "general", b.info()
    b.close()
    unb1, b = run_hdp(ctx, nhdp, batch, bp, shape["ragged"], cp.FLAG_UNBANDED | WIDE)
    assert b.info()["kernel"] == "general", b.info()
    b.close()
    same_results(unb0, unb1)
    assert WIDE == 256


@pytest.mark.parametrize("rows", [6, 8])
def test_expectations_stay_on_the_general_kernel(ctx, nhdp, rows):
    """the HDP E-step past 248 k-mers is out of these builds' scope: with the flag it runs what it runs without it, the
    general kernel.  The assignments are bit-equal; the sums are atomic additions of the same terms in an order that
    differs from run to run, so they are held to the project's bound for that (1e-9 relative, as test_hdp_gpu.py)"""
    shape = shape_of(rows, 0)
    batch = shape_batch(shape, nhdp)
    got = []
    for flags in (cp.FLAG_EXPECTATIONS, cp.FLAG_EXPECTATIONS | WIDE):
        ids = upload(ctx, nhdp)
        b = hbatch(ctx, batch, shape_bp(shape), shape["ragged"], flags)
        info = b.info()
        assert info["kernel"] == "general" and build_of(info["max_band_width"]) == rows, info
        b.run()
        b.sync()
        got.append((b.expectations(ids[0]), batch_results(b)))
        b.close()
    assert WIDE == 256
    assert np.allclose(got[0][0], got[1][0], rtol=1e-9, atol=1e-12)
    assert got[0][0][9] != 0.0 and np.count_nonzero(got[0][0][:9]) >= 7  # (no switch between the gaps by default)
    same_results(got[0][1], got[1][1])  # the assignments
    assert sum(len(r["triples"]) for r in got[0][1]) > 0


def test_environment_switch_in_a_fresh_process(tmp_path):
    """CPECAN_WIDE_BANDS_HDP=1 in a fresh child process: an HDP batch created with no flag runs a workgroup build and
    returns the pairs it returns without the variable (there on the general kernel)"""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hdp_wide_env_child.py")
    out = {}
    for name, value in (("off", None), ("on", "1")):
        env = {k: v for k, v in os.environ.items() if k != "CPECAN_WIDE_BANDS_HDP"}
        if value is not None:
            env["CPECAN_WIDE_BANDS_HDP"] = value
        path = str(tmp_path / (name + ".json"))
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, child, path], env=env, capture_output=True,
                           text=True, timeout=400)
        assert r.returncode == 0, r.stderr[-2000:]
        out[name] = json.load(open(path))
    rows = build_of(out["off"]["info"]["max_band_width"])
    assert out["off"]["info"]["kernel"] == "general" and rows is not None
    check_workgroup(out["on"]["info"], rows)
    assert len(out["on"]["pairs"]) > 100
    assert out["on"]["pairs"] == out["off"]["pairs"] and out["on"]["totals"] == out["off"]["totals"]


def fuzz_cases(n):
    """seeded shapes with sparse anchors (120..330 k-mers apart) and expansions of 60..220: by the band table alone at
    least three quarters land in one of the two classes, at least eight in each (tests/tools/hdp_wide_shapes.py counts
    them on the CPU); the first ones are the default run's"""
    rng = np.random.default_rng(20262)
    out = []
    for k in range(n):
        c = dict(seed=8300 + k, n=int(rng.integers(1, 3)), lX=int(rng.integers(350, 700)),
                 every=int(rng.integers(120, 331)), tb=int(rng.integers(1, 60)),
                 thr=float(rng.choice([0.5, 0.01, 1e-4, 0.0])), ragged=(int(rng.integers(0, 2)), int(rng.integers(0, 2))))
        c["e"] = 2 * int(rng.integers(30, 111))
        c["md"] = c["tb"] + 2 + int(rng.integers(0, 400))
        out.append(c)
    return out


def fuzz_batch(c, nhdp):
    return reads_batch(c["seed"], [c["lX"] - 37 * k for k in range(c["n"])], c["every"], nhdp)


def test_fuzz_hdp_wide_bands(ctx, nhdp):
    cases = fuzz_cases(24 * SCALE)
    model = o.HdpModel(nhdp)
    ran = {6: 0, 8: 0}
    upload(ctx, nhdp)
    for c in cases:
        batch = fuzz_batch(c, nhdp)
        bp = band_params(c["thr"], c["md"], c["tb"], c["e"])
        b = hbatch(ctx, batch, bp, c["ragged"], WIDE)
        b.run()
        b.sync()
        res = batch_results(b)
        info = b.info()
        rows = build_of(info["max_band_width"])
        if rows is not None:  # (a case whose band came out narrower or wider is compared all the same)
            check_workgroup(info, rows)
            ran[rows] += 1
        print("fuzz case", c["seed"], info)
        for i in range(len(batch["items"])):
            ref = run_oracle_hdp_item(batch, i, bp, model, c["ragged"])
            assert res[i]["cells"] == ref["cells"], (c["seed"], i)
            assert np.array_equal(res[i]["totals_xay"], ref["totals_xay"]), (c["seed"], i)
            assert np.array_equal(res[i]["totals"], ref["totals"]), (c["seed"], i)
            assert_same_pairs(res[i], ref)
        b.close()
    # at most a quarter of the cases outside the two builds, at least eight on each
    assert 4 * (len(cases) - sum(ran.values())) <= len(cases), ran
    assert min(ran.values()) >= 8, ran


@pytest.mark.parametrize("rows", [6, 8])
def test_event_means_off_the_grid_match_oracle(ctx, nhdp, rows):
    """hdp_batch draws every mean near its k-mer's mode, inside the sampling grid: here some means lie below the
    grid's first point, above its last, and exactly on both (grid_spline_interp's linear branches, staged as cell
    -1 / -2 with the distance to the grid's end), against the oracle"""
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
    res, b = run_hdp(ctx, nhdp, batch, shape_bp(shape), shape["ragged"], WIDE)
    check_workgroup(b.info(), rows)
    check_oracle(res, oracle_results(("offgrid", rows), batch, shape_bp(shape), o.HdpModel(nhdp), shape["ragged"]))
    b.close()


@pytest.mark.parametrize("rows", [6, 8])
def test_a_column_that_is_no_kmer_scores_minus_infinity(ctx, nhdp, rows):
    """A character outside the alphabet makes the six k-mers that contain it no k-mers (id -1).  The reference exits
    there, the oracle and the general kernel answer NaN, so neither can be the reference of this case; the
    register-resident builds score such a column -inf as match and as gap-Y emission (cpecan_k_wv_forward_h*).  What
    follows from that and is asserted: every total stays finite (the six columns can still be crossed through gap X,
    whose emission is the flat log(0.1)), no aligned pair lies in one of the six columns, pairs exist on both sides of
    them, and the columns away from the character are scored as before: the cells counted are those of the same read
    without the character."""
    shape = shape_of(rows, 2)
    batch = shape_batch(shape, nhdp)
    it = batch["items"][0]
    p = it["x_offset"] + it["lX"] // 2
    bad = dict(batch, x_chars=batch["x_chars"][:p] + "N" + batch["x_chars"][p + 1:])
    res, b = run_hdp(ctx, nhdp, bad, shape_bp(shape), shape["ragged"], WIDE)
    check_workgroup(b.info(), rows)
    b.close()
    clean = shape_refs(shape, batch, nhdp)
    k0, k1 = it["lX"] // 2 - 5, it["lX"] // 2  # the k-mers (pair coordinate x) that contain the character
    g = res[0]
    assert g["cells"] == clean[0]["cells"]
    assert len(g["totals"]) == len(clean[0]["totals"]) and np.all(np.isfinite(g["totals"]))
    x = np.asarray(g["triples"])[:, 1]
    assert not np.any((x >= k0) & (x <= k1))
    assert np.any(x < k0) and np.any(x > k1)
    assert np.all(np.isfinite(g["logp"]))
    # the other reads of the batch do not see the character
    for i in range(1, len(res)):
        assert np.array_equal(res[i]["totals"], clean[i]["totals"])
        assert_same_pairs(res[i], clean[i])

"""The vanilla signal machine on the workgroup-per-alignment kernels (CPECAN_FLAG_WIDE_BANDS on a vanilla posterior
batch: four waves per workgroup for bands of 185..248 k-mers, six for 249..376, eight for 377..504) against the oracle's
vanilla machine, through the C-ABI: cells, totalProbability refreshes and posterior exponents bit-identical, pairs in
the reference's emission order -- and the dispatch around them: nothing changes without the flag, at 184 k-mers and
below, past 504, with CPECAN_FLAG_GENERAL_KERNEL, and for the E-step, which stays on the general kernel."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import edge_reads
import pyoracle as o
import synth
from harness import assert_same_pairs, band_params, batch_results, cp, make_items, orc_params
from test_vanilla_gpu import run as run_plain
from test_vanilla_gpu import skip_bins

pytestmark = pytest.mark.gpu

WIDE = cp.FLAG_WIDE_BANDS
# the widest band of the vanilla wave builds, then of the four-, six- and eight-wave workgroup builds
WV, W4, W6, W8 = 184, 248, 376, 504
SCALE = max(1, int(os.environ.get("CPECAN_FUZZ_SCALE", "1")))


@pytest.fixture(scope="module")
def ctx():
    c = cp.Context(0)
    yield c
    c.close()


def build_of(width):
    """waves per workgroup of the vanilla workgroup build that takes a band of `width` k-mers (None: not one of them)"""
    return 4 if WV < width <= W4 else 6 if W4 < width <= W6 else 8 if W6 < width <= W8 else None


def vanilla_models(batch):
    """one VanillaModel per model of the batch (per-read scaled tables as synth draws them), the strands' fudge
    factors alternating as stateMachine3Vanilla_setStrandTransitionsToDefaults sets them, skip bins of its own each"""
    models = []
    for i, (match, _, gapy) in enumerate(batch["models"]):
        strand = (np.float32(0.17), np.float32(0.55)) if i % 2 == 0 else (np.float32(0.14), np.float32(0.49))
        models.append(o.VanillaModel(match, skip_bins(i), gapy, float(strand[0]), float(strand[1])))
    return models


def upload(ctx, models):
    ctx.models_clear()
    return ctx.modelsv_create([(m.scalars, m.match, m.skip, m.gap_y) for m in models])


def vbatch(ctx, batch, bp, ragged, flags):
    return cp.Batch(ctx, make_items(batch, ragged), batch["x_chars"], batch["events"], batch["anchors"], bp, flags=flags,
                    vanilla=True)


def run_vanilla(ctx, batch, models, bp, ragged, flags):
    upload(ctx, models)
    b = vbatch(ctx, batch, bp, ragged, flags)
    b.run()
    b.sync()
    return batch_results(b), b


def oracle_item(batch, models, i, bp, ragged):
    it = batch["items"][i]
    x = batch["x_chars"][it["x_offset"]: it["x_offset"] + it["lX"] + 5]
    ev = batch["events"][it["y_offset"]: it["y_offset"] + it["lY"]]
    an = batch["anchors"][it["anchor_offset"]: it["anchor_offset"] + it["n_anchors"]]
    ref = o.aligned_pairs_using_anchors(models[it["model"]], x, it["lX"], ev, an, orc_params(bp, split=1 << 60),
                                        ragged[0], ragged[1])
    ref["triples"], ref["logp"] = ref["triples"][::-1], ref["logp"][::-1]  # emission order
    return ref


def check_oracle(batch, models, res, bp, ragged):
    for i in range(len(batch["items"])):
        ref = oracle_item(batch, models, i, bp, ragged)
        assert res[i]["cells"] == ref["cells"], i
        assert np.array_equal(res[i]["totals_xay"], ref["totals_xay"]), i
        assert np.array_equal(res[i]["totals"], ref["totals"]), i
        assert_same_pairs(res[i], ref)
        assert len(res[i]["triples"]) > 0


def check_workgroup(info, rows):
    assert info["kernel"] == "systolic" and info["family"] == "workgroup", info
    assert info["waves_per_workgroup"] == rows, info
    assert build_of(info["max_band_width"]) == rows, info  # the inputs are of the class they were chosen for
    assert info["assembly_sweeps"] == 0 and info["fused_expectations"] == 0, info


def same_results(a, b):
    for x, y in zip(a, b):
        for key in ("triples", "logp", "totals_xay", "totals"):
            assert np.array_equal(x[key], y[key]), key
        assert x["cells"] == y["cells"]


# sparse anchors and a wide expansion: every shape spans several traceback windows (md diagonals apart); the widths were
# checked with cpecan_band_construct on the CPU (tests/tools/vanilla_wide_shapes.py prints them)
SHAPES = [
    dict(rows=4, seed=81, n=3, lX=600, lY=1200, every=150, e=80, md=250, tb=40, ragged=(1, 1), sigma=0.0),
    dict(rows=4, seed=82, n=4, lX=500, lY=1050, every=120, e=100, md=150, tb=30, ragged=(0, 1), sigma=0.4),
    dict(rows=4, seed=83, n=2, lX=450, lY=900, every=150, e=60, md=120, tb=20, ragged=(0, 0), sigma=0.0),
    dict(rows=6, seed=24, n=1, lX=400, lY=800, every=400, e=300, md=200, tb=40, ragged=(0, 0), sigma=0.0),
    dict(rows=6, seed=61, n=3, lX=700, lY=1400, every=250, e=90, md=300, tb=40, ragged=(1, 1), sigma=0.0),
    dict(rows=6, seed=62, n=4, lX=600, lY=1250, every=200, e=140, md=150, tb=30, ragged=(0, 1), sigma=0.4),
    dict(rows=8, seed=63, n=3, lX=800, lY=1600, every=300, e=180, md=300, tb=40, ragged=(1, 1), sigma=0.0),
    dict(rows=8, seed=64, n=4, lX=900, lY=1850, every=300, e=160, md=200, tb=20, ragged=(1, 0), sigma=0.4),
    dict(rows=8, seed=65, n=2, lX=700, lY=1300, every=380, e=100, md=120, tb=40, ragged=(0, 0), sigma=0.0),
]


def shape_batch(s):
    return synth.make_batch(s["seed"], s["n"], s["lX"], s["lY"], anchor_every=s["every"], length_sigma=s["sigma"])


def shape_id(s):
    return "v%d-seed%d" % (s["rows"], s["seed"])


def shape_of(rows, k=0):
    return [s for s in SHAPES if s["rows"] == rows][k]


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_vanilla_workgroup_posterior_matches_oracle(ctx, shape):
    batch = shape_batch(shape)
    models = vanilla_models(batch)
    bp = band_params(0.01, shape["md"], shape["tb"], shape["e"])
    res, b = run_vanilla(ctx, batch, models, bp, shape["ragged"], WIDE)
    check_workgroup(b.info(), shape["rows"])
    assert (shape["lX"] + shape["lY"]) // shape["md"] >= 3  # several traceback windows
    check_oracle(batch, models, res, bp, shape["ragged"])
    b.close()


def exact_width_batch(width):
    """two reads whose path runs on the band's upper edge, the first one's widest band exactly `width` k-mers (the
    other's at most that), as edge_reads builds its w... families"""
    batch = edge_reads.edge_batch(1, 2, 700, 1050, "upper", every=1, e=40, width=width)
    return batch, band_params(0.01, 150, 40, batch["e"])


@pytest.mark.parametrize("width", [185, 248, 249, 376, 377, 504])
def test_bands_at_the_edges_of_the_builds(ctx, width):
    batch, bp = exact_width_batch(width)
    models = vanilla_models(batch)
    ragged = (width % 2, 1)
    res, b = run_vanilla(ctx, batch, models, bp, ragged, WIDE)
    assert b.info()["max_band_width"] == width
    check_workgroup(b.info(), build_of(width))
    check_oracle(batch, models, res, bp, ragged)
    b.close()


@pytest.mark.parametrize("name", ["w185", "w248", "w249"])
def test_edge_families(ctx, name):
    """the w... families of edge_reads (the reads' mass on the band's upper edge), as the other machines run them"""
    f = edge_reads.signal_family(name)
    batch = edge_reads.signal_batch(name)
    models = vanilla_models(batch)
    bp = band_params(0.01, f["md"], f["tb"], batch["e"])
    res, b = run_vanilla(ctx, batch, models, bp, f["ragged"], WIDE)
    assert b.info()["max_band_width"] == f["width"]
    check_workgroup(b.info(), build_of(f["width"]))
    check_oracle(batch, models, res, bp, f["ragged"])
    b.close()


def test_flag_changes_nothing_at_184(ctx):
    f = edge_reads.signal_family("w184")
    batch = edge_reads.signal_batch("w184")
    models = vanilla_models(batch)
    bp = band_params(0.01, f["md"], f["tb"], batch["e"])
    plain, b0 = run_vanilla(ctx, batch, models, bp, f["ragged"], 0)
    info0 = b0.info()
    b0.close()
    flagged, b1 = run_vanilla(ctx, batch, models, bp, f["ragged"], WIDE)
    assert info0["max_band_width"] == 184 and info0["kernel"] == "systolic" and info0["family"] == "wave", info0
    assert b1.info() == info0
    same_results(plain, flagged)
    check_oracle(batch, models, flagged, bp, f["ragged"])
    b1.close()


def test_band_of_505_goes_to_the_general_kernel(ctx):
    batch, bp = exact_width_batch(505)
    models = vanilla_models(batch)
    res, b = run_vanilla(ctx, batch, models, bp, (1, 1), WIDE)
    assert b.info()["max_band_width"] == 505 and b.info()["kernel"] == "general", b.info()
    check_oracle(batch, models, res, bp, (1, 1))
    b.close()


def test_without_the_flag_185_is_as_before(ctx):
    batch, bp = exact_width_batch(185)
    models = vanilla_models(batch)
    res, b = run_vanilla(ctx, batch, models, bp, (1, 1), 0)
    assert b.info()["max_band_width"] == 185 and b.info()["kernel"] == "general", b.info()
    check_oracle(batch, models, res, bp, (1, 1))
    b.close()
    # the existing helper's own route assertions (no flag): the general kernel past 184
    run_plain(ctx, batch, models, bp, (1, 1))


@pytest.mark.parametrize("rows", [4, 6, 8])
def test_general_kernel_flag_wins_and_results_are_bit_equal(ctx, rows):
    """CPECAN_FLAG_GENERAL_KERNEL | WIDE_BANDS runs cpecan_k_generalv; the workgroup build gives the same doubles"""
    shape = shape_of(rows, 1)
    batch = shape_batch(shape)
    models = vanilla_models(batch)
    bp = band_params(0.01, shape["md"], shape["tb"], shape["e"])
    gen, b0 = run_vanilla(ctx, batch, models, bp, shape["ragged"], WIDE | cp.FLAG_GENERAL_KERNEL)
    assert b0.info()["kernel"] == "general", b0.info()
    b0.close()
    wg, b1 = run_vanilla(ctx, batch, models, bp, shape["ragged"], WIDE)
    check_workgroup(b1.info(), rows)
    b1.close()
    same_results(gen, wg)


@pytest.mark.parametrize("rows", [4, 8])
def test_expectations_stay_on_the_general_kernel(ctx, rows):
    """the vanilla E-step past 184 k-mers is out of these builds' scope: MODE_EXPECTATIONS | WIDE_BANDS runs the general
    kernel, its sums within the project's 1e-9 relative of the oracle (per-cell terms added in another order)"""
    shape = shape_of(rows)
    batch = shape_batch(shape)
    models = vanilla_models(batch)
    bp = band_params(0.01, shape["md"], shape["tb"], shape["e"])
    ids = upload(ctx, models)
    b = vbatch(ctx, batch, bp, shape["ragged"], cp.FLAG_EXPECTATIONS | WIDE)
    info = b.info()
    assert info["kernel"] == "general" and build_of(info["max_band_width"]) == rows, info
    b.run()
    b.sync()
    got = [b.expectations(mid) for mid in ids]
    b.close()
    p = orc_params(bp, split=1 << 60)
    hmms = [o.OrcExpectationsV() for _ in models]
    for it in batch["items"]:
        x = batch["x_chars"][it["x_offset"]: it["x_offset"] + it["lX"] + 5]
        ev = batch["events"][it["y_offset"]: it["y_offset"] + it["lY"]]
        an = batch["anchors"][it["anchor_offset"]: it["anchor_offset"] + it["n_anchors"]]
        o.expectations_v_using_anchors(models[it["model"]], x, it["lX"], ev, an, p, hmms[it["model"]],
                                       shape["ragged"][0], shape["ragged"][1])
    seen = 0
    for g, hmm in zip(got, hmms):
        ref = hmm.as_array()
        assert np.allclose(g, ref, rtol=1e-9, atol=1e-12)
        assert ref[-1] < 0
        seen += np.count_nonzero(ref[:60])
    assert seen > 20


@pytest.mark.parametrize("rows", [4, 6, 8])
def test_scan_decode_matches_oracle(ctx, rows):
    shape = shape_of(rows, 1)
    batch = shape_batch(shape)
    models = vanilla_models(batch)
    bp = band_params(0.01, shape["md"], shape["tb"], shape["e"])
    res, b = run_vanilla(ctx, batch, models, bp, shape["ragged"], WIDE | cp.FLAG_SCAN_DECODE)
    check_workgroup(b.info(), shape["rows"])
    check_oracle(batch, models, res, bp, shape["ragged"])
    b.close()


# one read with a single anchor gap of 400 k-mers: the expansion sets the class
THRESHOLD_ZERO_E = {4: 60, 6: 300, 8: 420}


@pytest.mark.parametrize("rows", [4, 6, 8])
def test_threshold_zero_overflows_and_reruns(ctx, rows):
    # every cell of the band with x, y > 0 is a pair: far more than the first pair allocation, so the batch is re-run
    # with the counted sizes
    batch = synth.make_batch(70 + rows, 1, 400, 800, anchor_every=400)
    models = vanilla_models(batch)
    bp = band_params(0.0, 200, 40, THRESHOLD_ZERO_E[rows])
    res, b = run_vanilla(ctx, batch, models, bp, (1, 1), WIDE)
    check_workgroup(b.info(), rows)
    assert len(res[0]["triples"]) > 4 * (400 + 800) + 64
    check_oracle(batch, models, res, bp, (1, 1))
    b.close()


def test_chained_batches_of_different_classes(ctx):
    shapes = [shape_of(4), shape_of(8)]
    batches = [shape_batch(s) for s in shapes]
    bps = [band_params(0.01, s["md"], s["tb"], s["e"]) for s in shapes]
    # one model set for both batches: the second batch's model ids follow the first's
    models = []
    for bt in batches:
        own = vanilla_models(bt)
        for it in bt["items"]:
            it["model"] += len(models)
        models += own
    upload(ctx, models)
    bs = [vbatch(ctx, bt, bp, s["ragged"], WIDE) for bt, s, bp in zip(batches, shapes, bps)]
    for b, s in zip(bs, shapes):
        check_workgroup(b.info(), s["rows"])
    prev = None
    for _ in range(3):
        for b in bs:
            b.run(after=prev)
            prev = b
    for b, bt, s, bp in zip(bs, batches, shapes, bps):
        b.sync()
        check_oracle(bt, models, batch_results(b), bp, s["ragged"])
    for b in bs:
        b.close()


def test_environment_switch_through_the_host_library(tmp_path):
    """CPECAN_WIDE_BANDS=1 in a fresh child process: a vanilla batch created with no flag runs a workgroup build, and
    getSignalStateMachine3Vanilla + getAlignedPairsUsingAnchors of libcpecan_host.so on a wide band return the list they
    return without the variable (there on the general kernel)"""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "vanilla_wide_env_child.py")
    out = {}
    for name, value in (("off", None), ("on", "1")):
        env = {k: v for k, v in os.environ.items() if k != "CPECAN_WIDE_BANDS"}
        if value is not None:
            env["CPECAN_WIDE_BANDS"] = value
        path = str(tmp_path / (name + ".json"))
        r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, child, path], env=env, capture_output=True,
                           text=True, timeout=700)
        assert r.returncode == 0, r.stderr[-2000:]
        out[name] = json.load(open(path))
    rows = build_of(out["off"]["info"]["max_band_width"])
    assert out["off"]["info"]["kernel"] == "general" and rows is not None
    check_workgroup(out["on"]["info"], rows)
    assert build_of(out["on"]["host_band_width"]) is not None  # the host call's band is one of the three classes
    assert len(out["on"]["host_pairs"]) > 100
    assert out["on"]["host_pairs"] == out["off"]["host_pairs"]
    assert out["on"]["batch_pairs"] == out["off"]["batch_pairs"]


def fuzz_cases(n):
    """seeded shapes with sparse anchors (100..400 k-mers apart) and expansions of 80..240: by the band table alone at
    least three quarters land in one of the three classes, and every class is hit (tests/tools/vanilla_wide_shapes.py
    counts them on the CPU); the first ones are the default run's"""
    rng = np.random.default_rng(20261)
    out = []
    for k in range(n):
        lX = int(rng.integers(350, 1000))
        c = dict(seed=7300 + k, n=int(rng.integers(1, 4)), lX=lX, lY=int(lX * rng.uniform(1.6, 2.4)),
                 every=int(rng.integers(100, 401)), e=0, tb=int(rng.integers(1, 60)),
                 thr=float(rng.choice([0.5, 0.01, 1e-4, 0.0])), ragged=(int(rng.integers(0, 2)), int(rng.integers(0, 2))),
                 sigma=float(rng.choice([0.0, 0.3])))
        # (the band is about the expansion plus the drift between two anchors wide: the sparser the anchors, the smaller
        # the expansions drawn, so that most cases stay within 504 k-mers)
        c["e"] = 2 * int(rng.integers(40, 121 - (c["every"] - 100) // 5))
        c["md"] = c["tb"] + 2 + int(rng.integers(0, 400))
        out.append(c)
    return out


def fuzz_batch(c):
    return synth.make_batch(c["seed"], c["n"], c["lX"], c["lY"], anchor_every=c["every"], length_sigma=c["sigma"])


def test_fuzz_vanilla_wide_bands(ctx):
    cases = fuzz_cases(24 * SCALE)
    ran = {4: 0, 6: 0, 8: 0}
    for c in cases:
        batch = fuzz_batch(c)
        models = vanilla_models(batch)
        bp = band_params(c["thr"], c["md"], c["tb"], c["e"])
        upload(ctx, models)
        b = vbatch(ctx, batch, bp, c["ragged"], WIDE)
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
            ref = oracle_item(batch, models, i, bp, c["ragged"])
            assert res[i]["cells"] == ref["cells"], (c["seed"], i)
            assert np.array_equal(res[i]["totals_xay"], ref["totals_xay"]), (c["seed"], i)
            assert np.array_equal(res[i]["totals"], ref["totals"]), (c["seed"], i)
            assert_same_pairs(res[i], ref)
        b.close()
    assert min(ran.values()) >= 1 and 4 * sum(ran.values()) >= 3 * len(cases), ran

"""The six- and eight-wave builds of the workgroup-per-alignment kernels (bands of 249..376 and 377..504 k-mers,
CPECAN_FLAG_WIDE_BANDS) against the oracle, through the C-ABI: the same bar as the narrower builds -- totals and
posterior exponents bit-identical, pairs in the reference's emission order -- and the dispatch around them: the flag
changes nothing for a band the four-wave builds hold, and a band past 504 k-mers still goes to the general kernel."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import edge_reads
import synth
from harness import assert_same_pairs, band_params, cp, make_items, run_gpu, run_oracle_item

pytestmark = pytest.mark.gpu

WIDE = cp.FLAG_WIDE_BANDS
# the widest band of the four-wave builds, of the six-wave and of the eight-wave build
W4, W6, W8 = 248, 376, 504
SCALE = max(1, int(os.environ.get("CPECAN_FUZZ_SCALE", "1")))


@pytest.fixture(scope="module")
def ctx():
    c = cp.Context(0)
    yield c
    c.close()


def build_of(width):
    """waves per workgroup of the wide build that takes a band of `width` k-mers (None: not a wide build's)"""
    return 6 if W4 < width <= W6 else 8 if W6 < width <= W8 else None


def check_wide(info, rows):
    assert info["kernel"] == "systolic" and info["family"] == "workgroup", info
    assert info["waves_per_workgroup"] == rows, info
    assert build_of(info["max_band_width"]) == rows, info  # the inputs are of the class they were chosen for
    assert info["assembly_sweeps"] == 0 and info["fused_expectations"] == 0, info


def check_oracle(batch, res, bp, ragged=(0, 0)):
    for i in range(len(batch["items"])):
        ref = run_oracle_item(batch, i, bp, ragged)
        assert res[i]["cells"] == ref["cells"], i
        assert np.array_equal(res[i]["totals_xay"], ref["totals_xay"]), i
        assert np.array_equal(res[i]["totals"], ref["totals"]), i
        assert_same_pairs(res[i], ref)


# sparse anchors and a wide expansion: every shape spans several traceback windows (md diagonals apart); widths were
# checked with cpecan_band_construct on the CPU (tests/tools/wide_band_shapes.py prints them)
SHAPES = [
    dict(rows=6, seed=24, n=1, lX=400, lY=800, every=400, e=300, md=200, tb=40, ragged=(0, 0), sigma=0.0),
    dict(rows=6, seed=61, n=3, lX=700, lY=1400, every=250, e=90, md=300, tb=40, ragged=(1, 1), sigma=0.0),
    dict(rows=6, seed=62, n=4, lX=600, lY=1250, every=200, e=140, md=150, tb=30, ragged=(0, 1), sigma=0.4),
    dict(rows=8, seed=63, n=3, lX=800, lY=1600, every=300, e=180, md=300, tb=40, ragged=(1, 1), sigma=0.0),
    dict(rows=8, seed=64, n=4, lX=900, lY=1850, every=300, e=160, md=200, tb=20, ragged=(1, 0), sigma=0.4),
    dict(rows=8, seed=65, n=2, lX=700, lY=1300, every=380, e=100, md=120, tb=40, ragged=(0, 0), sigma=0.0),
]


def shape_batch(s):
    return synth.make_batch(s["seed"], s["n"], s["lX"], s["lY"], anchor_every=s["every"], length_sigma=s["sigma"])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "r%d-seed%d" % (s["rows"], s["seed"]))
def test_wide_posterior_matches_oracle(ctx, shape):
    batch = shape_batch(shape)
    bp = band_params(0.01, shape["md"], shape["tb"], shape["e"])
    res, b = run_gpu(ctx, batch, bp, kernel=cp.KERNEL_AUTO, flags=WIDE, ragged=shape["ragged"])
    check_wide(b.info(), shape["rows"])
    assert (shape["lX"] + shape["lY"]) // shape["md"] >= 3  # several traceback windows
    check_oracle(batch, res, bp, shape["ragged"])
    b.close()


@pytest.mark.parametrize("family", [0, cp.FLAG_WORKGROUP_KERNELS], ids=["wave-default", "workgroup-default"])
def test_wide_build_whichever_family_is_the_default(ctx, family):
    shape = SHAPES[1]
    batch = shape_batch(shape)
    bp = band_params(0.01, shape["md"], shape["tb"], shape["e"])
    res, b = run_gpu(ctx, batch, bp, kernel=cp.KERNEL_AUTO, flags=WIDE | family, ragged=shape["ragged"])
    check_wide(b.info(), shape["rows"])
    check_oracle(batch, res, bp, shape["ragged"])
    b.close()


def exact_width_batch(width):
    """two reads whose path runs on the band's upper edge, the first one's widest band exactly `width` k-mers (the
    other's at most that), as edge_reads builds w248 / w249"""
    batch = edge_reads.edge_batch(1, 2, 700, 1050, "upper", every=1, e=40, width=width)
    return batch, band_params(0.01, 150, 40, batch["e"])


@pytest.mark.parametrize("width", [249, 376, 377, 504])
def test_bands_at_the_edges_of_the_wide_builds(ctx, width):
    batch, bp = exact_width_batch(width)
    ragged = (width % 2, 1)
    res, b = run_gpu(ctx, batch, bp, kernel=cp.KERNEL_AUTO, flags=WIDE, ragged=ragged)
    assert b.info()["max_band_width"] == width
    check_wide(b.info(), build_of(width))
    check_oracle(batch, res, bp, ragged)
    b.close()


def test_band_of_505_goes_to_the_general_kernel_or_is_refused(ctx):
    batch, bp = exact_width_batch(505)
    res, b = run_gpu(ctx, batch, bp, kernel=cp.KERNEL_AUTO, flags=WIDE, ragged=(1, 1))
    assert b.info()["max_band_width"] == 505 and b.info()["kernel"] == "general"
    check_oracle(batch, res, bp, (1, 1))
    b.close()
    with pytest.raises(cp.CpecanError) as ei:
        run_gpu(ctx, batch, bp, kernel=cp.KERNEL_SYSTOLIC, flags=WIDE, ragged=(1, 1))
    assert ei.value.code == cp.EINVAL and "504" in str(ei.value)


@pytest.mark.parametrize("family", [0, cp.FLAG_WORKGROUP_KERNELS], ids=["wave", "workgroup"])
@pytest.mark.parametrize("mode", [cp.MODE_POSTERIOR, cp.MODE_EXPECTATIONS], ids=["posterior", "expectations"])
def test_flag_changes_nothing_at_248(ctx, family, mode):
    batch = edge_reads.family_batch("w248")
    f = edge_reads.FAMILIES["w248"]
    bp = band_params(0.01, f["md"], f["tb"], batch["e"])
    plain, b0 = run_gpu(ctx, batch, bp, mode=mode, kernel=cp.KERNEL_AUTO, flags=family, ragged=f["ragged"])
    info0, exp0 = b0.info(), b0.expectations(0) if mode else None
    b0.close()
    flagged, b1 = run_gpu(ctx, batch, bp, mode=mode, kernel=cp.KERNEL_AUTO, flags=family | WIDE, ragged=f["ragged"])
    assert info0["max_band_width"] == 248 and b1.info() == info0
    for x, y in zip(plain, flagged):
        for key in ("triples", "logp", "totals_xay", "totals"):
            assert np.array_equal(x[key], y[key]), key
        assert x["cells"] == y["cells"]
    if mode:
        # the same kernels both times (info() equal, totals bit-equal above); the expectation sums themselves are
        # accumulated with floating-point atomics, whose order differs between two runs of one and the same batch:
        # the project's tolerance for them (test_systolic_gpu.py), 1e-9 relative
        assert np.allclose(exp0, b1.expectations(0), rtol=1e-9, atol=1e-12)
    b1.close()


def test_without_the_flag_a_wide_band_is_as_before(ctx):
    batch, bp = exact_width_batch(249)
    with pytest.raises(cp.CpecanError) as ei:
        run_gpu(ctx, batch, bp, kernel=cp.KERNEL_SYSTOLIC, ragged=(1, 1))
    assert ei.value.code == cp.EINVAL and "248" in str(ei.value)
    _, b = run_gpu(ctx, batch, bp, kernel=cp.KERNEL_AUTO, ragged=(1, 1))
    assert b.info()["kernel"] == "general"
    b.close()


def test_explicit_request_with_the_flag(ctx):
    # the batch test_systolic_gpu.py's refusal test uses: one anchor gap of 400
    batch = synth.make_batch(24, 1, 400, 800, anchor_every=400)
    bp = band_params(0.01, 200, 40, 300)
    res, b = run_gpu(ctx, batch, bp, kernel=cp.KERNEL_SYSTOLIC, flags=WIDE)
    check_wide(b.info(), build_of(b.info()["max_band_width"]))
    check_oracle(batch, res, bp)
    b.close()


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]], ids=["r6", "r8"])
def test_wide_expectations_match_oracle(ctx, shape):
    import pyoracle as o
    batch = synth.make_batch(shape["seed"], shape["n"], shape["lX"], shape["lY"], anchor_every=shape["every"],
                             distinct_models=False)
    bp = band_params(0.01, shape["md"], shape["tb"], shape["e"])
    res, b = run_gpu(ctx, batch, bp, mode=cp.MODE_EXPECTATIONS, kernel=cp.KERNEL_AUTO, flags=WIDE,
                     ragged=shape["ragged"])
    check_wide(b.info(), shape["rows"])
    got = b.expectations(0)
    hmm = o.OrcExpectations()
    for i in range(shape["n"]):
        ref = run_oracle_item(batch, i, bp, shape["ragged"], expectations=hmm)
        assert np.array_equal(res[i]["totals"], ref["totals"])
    # tolerance: the device sums in a different order and uses its own exp(): 1e-9 relative
    assert np.allclose(got[:9], np.array(hmm.transitions[:]), rtol=1e-9, atol=1e-12)
    assert np.allclose(got[9:9 + 4096], np.array(hmm.kmerGap[:]), rtol=1e-9, atol=1e-12)  # the gap-X bins
    assert np.isclose(got[-1], hmm.likelihood, rtol=1e-12)
    b.close()


@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[4]], ids=["r6", "r8"])
def test_wide_scan_decode_matches_oracle(ctx, shape):
    batch = shape_batch(shape)
    bp = band_params(0.01, shape["md"], shape["tb"], shape["e"])
    res, b = run_gpu(ctx, batch, bp, kernel=cp.KERNEL_AUTO, flags=WIDE | cp.FLAG_SCAN_DECODE, ragged=shape["ragged"])
    check_wide(b.info(), shape["rows"])
    check_oracle(batch, res, bp, shape["ragged"])
    b.close()


@pytest.mark.parametrize("rows", [6, 8])
def test_threshold_zero_overflows_and_reruns(ctx, rows):
    # every cell of the band with x, y > 0 is a pair: far more than the first pair allocation, so the batch is re-run
    # with the counted sizes
    batch = synth.make_batch(70 + rows, 1, 400, 800, anchor_every=400)
    bp = band_params(0.0, 200, 40, 300 if rows == 6 else 420)
    res, b = run_gpu(ctx, batch, bp, kernel=cp.KERNEL_AUTO, flags=WIDE, ragged=(1, 1))
    check_wide(b.info(), rows)
    assert len(res[0]["triples"]) > 4 * (400 + 800) + 64
    check_oracle(batch, res, bp, (1, 1))
    b.close()


def test_chained_wide_batches(ctx):
    shapes = [SHAPES[1], SHAPES[3]]
    batches = [shape_batch(s) for s in shapes]
    bps = [band_params(0.01, s["md"], s["tb"], s["e"]) for s in shapes]
    ctx.models_clear()
    # one model set for both batches: the second batch's model ids follow the first's
    models = []
    for bt in batches:
        for it in bt["items"]:
            it["model"] += len(models)
        models += bt["models"]
    ctx.models_create([(cp.NANOPORE_TRANSITIONS, m, gx, gy) for m, gx, gy in models])
    bs = [cp.Batch(ctx, make_items(bt, s["ragged"]), bt["x_chars"], bt["events"], bt["anchors"], bp, cp.MODE_POSTERIOR,
                   cp.KERNEL_AUTO, WIDE) for bt, s, bp in zip(batches, shapes, bps)]
    for b, s in zip(bs, shapes):
        check_wide(b.info(), s["rows"])
    prev = None
    for _ in range(3):
        for b in bs:
            b.run(after=prev)
            prev = b
    from harness import batch_results
    for b, bt, s, bp in zip(bs, batches, shapes, bps):
        b.sync()
        res = batch_results(b)
        for i, it in enumerate(bt["items"]):
            ref = run_oracle_item(dict(bt, models=models), i, bp, s["ragged"])
            assert np.array_equal(res[i]["totals"], ref["totals"])
            assert_same_pairs(res[i], ref)
    for b in bs:
        b.close()


def test_environment_switch_through_the_host_library(tmp_path):
    """CPECAN_WIDE_BANDS=1 in a fresh child process: a batch created with no flag runs the six-wave build, and
    getAlignedPairsUsingAnchors of libcpecan_host.so on the same wide read returns the list it returns without the
    variable (there on the general kernel)"""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "wide_env_child.py")
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
    assert out["off"]["info"]["kernel"] == "general" and build_of(out["off"]["info"]["max_band_width"]) == 6
    check_wide(out["on"]["info"], 6)
    assert len(out["on"]["host_pairs"]) > 100
    assert out["on"]["host_pairs"] == out["off"]["host_pairs"]
    assert out["on"]["batch_pairs"] == out["off"]["batch_pairs"]


def fuzz_cases(n):
    """seeded shapes with sparse anchors (150..450 k-mers apart) and expansions of 100..240: most land in a wide
    build's class (tests/tools/wide_band_shapes.py counts them on the CPU); the first ones are the default run's"""
    rng = np.random.default_rng(20260)
    out = []
    for k in range(n):
        lX = int(rng.integers(350, 1000))
        c = dict(seed=7000 + k, n=int(rng.integers(1, 4)), lX=lX, lY=int(lX * rng.uniform(1.6, 2.4)),
                 every=int(rng.integers(150, 451)), e=0, tb=int(rng.integers(1, 60)),
                 thr=float(rng.choice([0.5, 0.01, 1e-4, 0.0])), ragged=(int(rng.integers(0, 2)), int(rng.integers(0, 2))),
                 sigma=float(rng.choice([0.0, 0.3])))
        # (the band is about the expansion plus the drift between two anchors wide: the sparser the anchors, the smaller
        # the expansions drawn, so that most cases stay within 504 k-mers)
        c["e"] = 2 * int(rng.integers(50, 121 - (c["every"] - 150) // 6))
        c["md"] = c["tb"] + 2 + int(rng.integers(0, 400))
        out.append(c)
    return out


def test_fuzz_wide_bands(ctx):
    cases = fuzz_cases(24 * SCALE)
    ran = {6: 0, 8: 0}
    for c in cases:
        batch = synth.make_batch(c["seed"], c["n"], c["lX"], c["lY"], anchor_every=c["every"], length_sigma=c["sigma"])
        bp = band_params(c["thr"], c["md"], c["tb"], c["e"])
        res, b = run_gpu(ctx, batch, bp, kernel=cp.KERNEL_AUTO, flags=WIDE, ragged=c["ragged"])
        info = b.info()
        rows = build_of(info["max_band_width"])
        if rows is not None:  # (a case whose band came out narrower or wider is compared all the same)
            check_wide(info, rows)
            ran[rows] += 1
        print("fuzz case", c["seed"], info)
        check_oracle(batch, res, bp, c["ragged"])
        b.close()
    assert ran[6] >= 1 and ran[8] >= 1 and 4 * (ran[6] + ran[8]) >= 3 * len(cases), ran

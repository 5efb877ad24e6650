"""The assembly sweeps at two cells per lane on the card (CPECAN_FLAG_ASM_NARROW_BANDS / CPECAN_ASM_NARROW=1: strawMan
posterior batches of the wave kernels whose widest band is at most 120 k-mers -- what the reference's default
diagonalExpansion of 20 and its driver's 50 give) against the oracle: cells, totals and their diagonals, pairs, their
order and exponents bit-identical, no tolerance; on both ring layouts, run twice, chained, fuzzed, through the
environment variable alone; and the batches the flag means nothing to.

The fuzz list's widest expansion is 68, not the 69 that would give a band of 120 around anchors every 50 columns: the
library refuses an odd diagonalExpansion, as the reference does (pairwiseAligner.c:880-884).
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import synth
from harness import assert_same_pairs, band_params, batch_results, cp, make_items, run_gpu, run_oracle_item

pytestmark = pytest.mark.gpu

NARROW = cp.FLAG_ASM_NARROW_BANDS
SCALE = max(1, int(os.environ.get("CPECAN_FUZZ_SCALE", "1")))
RAGGED = (1, 1)
MAIN = dict(seed=33, n=3, lX=700, lY=1400, every=50)
MAIN_SHAPES = {20: (72, 7), 50: (102, 8), 60: (112, 8)}   # diagonalExpansion -> widest band, windows of the longest read

_BATCH, _ORACLE = {}, {}


def main_batch():
    if "main" not in _BATCH:
        _BATCH["main"] = synth.make_batch(MAIN["seed"], MAIN["n"], MAIN["lX"], MAIN["lY"], anchor_every=MAIN["every"])
    return _BATCH["main"]


def main_bp(e):
    return band_params(0.01, 300, 40, e)


def main_oracle(e, i):
    if (e, i) not in _ORACLE:
        _ORACLE[(e, i)] = run_oracle_item(main_batch(), i, main_bp(e), RAGGED)
    return _ORACLE[(e, i)]


def assert_oracle(g, ref, what=""):
    assert g["cells"] == ref["cells"], what
    assert np.array_equal(g["totals_xay"], ref["totals_xay"]), what
    assert np.array_equal(g["totals"], ref["totals"]), what
    assert_same_pairs(g, ref)


def assert_two_cells(info):
    assert info["kernel"] == "systolic" and info["family"] == "wave", info
    assert info["assembly_sweeps"] == 2 and info["waves_per_workgroup"] == 2, info


def same_bytes(a, b):
    return all(x["cells"] == y["cells"] and all(np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes()
                                                for k in ("triples", "logp", "totals_xay", "totals")) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def ctx():
    c = cp.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("ring", [0, cp.FLAG_SMALL_FOOTPRINT], ids=["three-window-ring", "small-footprint"])
@pytest.mark.parametrize("e", sorted(MAIN_SHAPES))
def test_narrow_bands_on_the_two_cell_sweeps_equal_the_oracle(ctx, e, ring):
    batch, bp = main_batch(), main_bp(e)
    res, b = run_gpu(ctx, batch, bp, flags=NARROW | ring, ragged=RAGGED)
    info = b.info()
    assert_two_cells(info)
    assert info["max_band_width"] == MAIN_SHAPES[e][0]
    for i in range(MAIN["n"]):
        assert_oracle(res[i], main_oracle(e, i), (e, i))
    b.run()          # the same batch again: the same bytes
    b.sync()
    assert same_bytes(batch_results(b), res)
    b.close()
    # ... and without the flag the compiled sweeps of the same build, as before
    res0, b0 = run_gpu(ctx, batch, bp, flags=ring, ragged=RAGGED)
    assert b0.info()["assembly_sweeps"] == 0 and b0.info()["waves_per_workgroup"] == 2
    assert same_bytes(res0, res)
    b0.close()


def test_two_chained_batches_for_three_rounds():
    """two batches on two contexts, each round's run ordered behind the other batch's (run(after=...)), compared with
    the oracle after every wait"""
    e = 50
    ctxs = [cp.Context(0) for _ in range(2)]
    bs = []
    for cx in ctxs:
        cx.models_clear()
        cx.models_create([(cp.NANOPORE_TRANSITIONS, m, gx, gy) for (m, gx, gy) in main_batch()["models"]])
        bs.append(cp.Batch(cx, make_items(main_batch(), RAGGED), main_batch()["x_chars"], main_batch()["events"],
                           main_batch()["anchors"], main_bp(e), cp.MODE_POSTERIOR, cp.KERNEL_AUTO, NARROW))
        assert_two_cells(bs[-1].info())

    def check(b):
        for i, g in enumerate(batch_results(b)):
            assert_oracle(g, main_oracle(e, i), i)

    pending = [False, False]
    for s in range(6):
        j = s % 2
        if pending[j]:
            bs[j].sync()
            check(bs[j])
        bs[j].run(after=bs[(s - 1) % 2] if s > 0 else None)
        pending[j] = True
    for b in bs:
        b.sync()
        check(b)
    for cx in ctxs:
        cx.close()


def fuzz_cases(n, seed):
    """shaped like test_fuzz_gpu.asm_cases, with the expansions of narrow bands"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        lX = int(rng.integers(130, 901))
        c = dict(seed=7000 + k, lX=lX, lY=int(lX * rng.uniform(1.6, 2.4)), every=int(rng.choice([25, 50, 80])),
                 e=int(rng.choice([0, 2, 10, 20, 40, 50, 60, 68])), tb=int(rng.integers(1, 60)),
                 thr=float(rng.choice([0.5, 0.01, 1e-4, 0.0])), ragged=(int(rng.integers(0, 2)), int(rng.integers(0, 2))),
                 flags=int(rng.choice([0, cp.FLAG_SMALL_FOOTPRINT])), n=int(rng.integers(1, 4)))
        c["md"] = c["tb"] + 2 + int(rng.integers(0, 500))
        out.append(c)
    return out


FUZZ_SEED = 8192


def fuzz_batch(case):
    return synth.make_batch(case["seed"], case["n"], case["lX"], case["lY"], anchor_every=case["every"], length_sigma=0.2)


def planned_cells(case):
    """what cpecan_hip_plan_assembly_sweeps answers for the case's bands, worked out on the host: no device"""
    batch = fuzz_batch(case)
    width, by_one = 0, True
    for it in batch["items"]:
        an = batch["anchors"][it["anchor_offset"]: it["anchor_offset"] + it["n_anchors"]]
        L, R = cp.band_construct(an, it["lX"], it["lY"], case["e"])
        k = np.arange(len(L))
        width = max(width, int((((R - L) >> 1) + 1).max()))
        for edge in ((k + L) // 2, (k + R) // 2):
            by_one = by_one and bool(((np.diff(edge) >= 0) & (np.diff(edge) <= 1)).all())
    return cp.plan_assembly_sweeps(cp.MACHINE_STRAWMAN, cp.MODE_POSTERIOR, cp.KERNEL_AUTO, NARROW | case["flags"], width, by_one)


@pytest.mark.parametrize("case", fuzz_cases(24 * SCALE, FUZZ_SEED), ids=lambda c: "n%d" % c["seed"])
def test_random_case_narrow_bands(ctx, case):
    batch = fuzz_batch(case)
    bp = band_params(case["thr"], case["md"], case["tb"], case["e"])
    res, b = run_gpu(ctx, batch, bp, kernel=cp.KERNEL_AUTO, flags=NARROW | case["flags"], ragged=case["ragged"])
    info = b.info()
    if info["kernel"] == "systolic" and info["waves_per_workgroup"] == 2 and info["max_band_width"] <= 120:
        assert_two_cells(info)
    assert (info.get("assembly_sweeps") == 2 and info.get("waves_per_workgroup") == 2) == (planned_cells(case) == 2), info
    b.close()
    for i in range(case["n"]):
        assert_oracle(res[i], run_oracle_item(batch, i, bp, case["ragged"]), i)


def test_at_least_half_of_the_random_cases_run_the_two_cell_sweeps():
    cases = fuzz_cases(24 * SCALE, FUZZ_SEED)
    assert 2 * sum(planned_cells(c) == 2 for c in cases) >= len(cases)


def test_the_environment_variable_alone(ctx):
    """CPECAN_ASM_NARROW=1 and no flag, in a process of its own (asm_narrow_env_child.py)"""
    e = 20
    env = dict(os.environ, CPECAN_ASM_NARROW="1")
    env.pop("CPECAN_ASM", None)
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "out.json")
        subprocess.check_call([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "asm_narrow_env_child.py"),
                               str(e), out], env=env)
        got = json.load(open(out))
    assert_two_cells(got["info"])
    for i, g in enumerate(got["items"]):
        ref = main_oracle(e, i)
        g = dict(cells=g["cells"], triples=np.array(g["triples"], np.int64).reshape(-1, 3),
                 logp=np.array(g["logp"], np.uint64).view(np.float64), totals_xay=np.array(g["totals_xay"], np.int64),
                 totals=np.array(g["totals"], np.uint64).view(np.float64))
        assert_oracle(g, ref, i)


def test_batches_the_flag_means_nothing_to(ctx):
    """a vanilla posterior batch and a strawMan E-step report with the flag exactly what they report without it"""
    import pyoracle as o
    import test_vanilla_gpu as tv
    batch = synth.make_batch(35, 2, 200, 420, anchor_every=50)
    bp = band_params(0.01, 120, 30, 50)
    models = [o.VanillaModel(m, tv.skip_bins(i), gy) for i, (m, _, gy) in enumerate(batch["models"])]
    seen = []
    for flags in (0, NARROW):
        ctx.models_clear()
        ctx.modelsv_create([(m.scalars, m.match, m.skip, m.gap_y) for m in models])
        b = cp.Batch(ctx, make_items(batch, RAGGED), batch["x_chars"], batch["events"], batch["anchors"], bp, flags=flags,
                     vanilla=True)
        b.run()
        b.sync()
        seen.append((b.info(), batch_results(b)))
        b.close()
    assert seen[0][0] == seen[1][0] and seen[0][0]["assembly_sweeps"] == 0 and seen[0][0]["waves_per_workgroup"] == 2
    assert same_bytes(seen[0][1], seen[1][1])
    seen = []
    for flags in (0, NARROW):
        ctx.models_clear()
        ids = ctx.models_create([(cp.NANOPORE_TRANSITIONS, m, gx, gy) for (m, gx, gy) in batch["models"]])
        b = cp.Batch(ctx, make_items(batch, RAGGED), batch["x_chars"], batch["events"], batch["anchors"], bp,
                     cp.MODE_EXPECTATIONS, cp.KERNEL_AUTO, flags)
        b.run()
        b.sync()
        seen.append((b.info(), [b.expectations(i) for i in ids]))
        b.close()
    assert seen[0][0] == seen[1][0] and seen[0][0]["assembly_sweeps"] == 0 and seen[0][0]["waves_per_workgroup"] == 2
    # (the same kernels both times; their sums are atomic adds whose order differs from run to run: the E-step tests' 1e-9)
    for a, c in zip(seen[0][1], seen[1][1]):
        assert np.allclose(a, c, rtol=1e-9, atol=0.0, equal_nan=True)

"""The vanilla machine's E-step with its expectations summed inside the wave kernels' sweep back
(CPECAN_FLAG_VANILLA_FUSED_ESTEP: cpecan_k_wv_backward_fx_vf2 / _vf3, the post kernel's finish, the re-sweep of the
windows the estimate cannot carry) against the oracle's vanilla E-step and against the path through the ring of backward
cells and cpecan_k_wv_expect.  The shapes are those of test_vanilla_gpu.py::test_vanilla_expectations_match_oracle, one
model per read with skip bins of its own and the two strands' fudge factors in turn, ragged ends.

Bars: against the oracle the project's for every E-step -- the 60 bins to rtol 1e-9 / atol 1e-12 (the same terms added
in another order, the device's exp), the likelihood to rtol 1e-12; fused against the ring 1e-11 on the bins (a term
exp(a - estimate) * exp(estimate - total) in place of exp(a - total): the estimate lies within 30 nats of the total,
so the two differ by a few ulp of an argument of that size) and 1e-12 on the likelihood; the persistent step against a
fresh batch 1e-12 (the same kernels on the same tables: only the order of the atomic additions differs).  Every case
asserts its route: without that each would pass on the ring path."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pyoracle as o
import synth
from cpecan_load import em
from harness import band_params, cp, make_items, orc_params
from test_vanilla_gpu import skip_bins
from test_vanilla_scaled_models_gpu import NEW_BINS, as_tuple, host_scaled, two_strand_batch

pytestmark = pytest.mark.gpu

FUSED = getattr(cp, "FLAG_VANILLA_FUSED_ESTEP", 0)  # (0 before the flag existed: every route assertion then fails)
EXP = cp.FLAG_EXPECTATIONS
# (m_to_y_not_x, e_to_e) of the template and the complement strand, stateMachine3Vanilla_setStrandTransitionsToDefaults
FUDGE = ((float(np.float32(0.17)), float(np.float32(0.55))), (float(np.float32(0.14)), float(np.float32(0.49))))
SHAPES = {
    "two-cells": dict(seed=57, n=4, lX=150, lY=310, every=30, md=60, tb=10, e=20, cells=2),       # short windows, many segments
    "three-cells": dict(seed=57, n=3, lX=700, lY=1500, every=50, md=300, tb=40, e=100, cells=3),  # band 101-156; more than
                                                                                                # 192 columns: slots change column
    "no-anchors": dict(seed=57, n=2, lX=90, lY=200, every=10 ** 6, md=40, tb=5, e=20, cells=2),
    "two-cells-b": dict(seed=58, n=4, lX=150, lY=310, every=30, md=60, tb=10, e=20, cells=2),     # (the chained rounds' second batch)
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(batch, the oracle's models, band parameters) of a shape"""
    sh = SHAPES[name]
    batch = synth.make_batch(sh["seed"], sh["n"], sh["lX"], sh["lY"], anchor_every=sh["every"])
    models = [o.VanillaModel(match, skip_bins(i), gapy, *FUDGE[i % 2]) for i, (match, _, gapy) in enumerate(batch["models"])]
    return batch, models, band_params(0.01, sh["md"], sh["tb"], sh["e"])


@functools.lru_cache(maxsize=None)
def oracle(name):
    """the 61 sums of every model of a shape, computed once for all the tests that compare against them"""
    batch, models, bp = case(name)
    p = orc_params(bp, split=1 << 60)
    hmms = [o.OrcExpectationsV() for _ in models]
    for it in batch["items"]:
        x = batch["x_chars"][it["x_offset"]: it["x_offset"] + it["lX"] + 5]
        ev = batch["events"][it["y_offset"]: it["y_offset"] + it["lY"]]
        an = batch["anchors"][it["anchor_offset"]: it["anchor_offset"] + it["n_anchors"]]
        o.expectations_v_using_anchors(models[it["model"]], x, it["lX"], ev, an, p, hmms[it["model"]], True, True)
    ref = [h.as_array() for h in hmms]
    for r in ref:
        r.setflags(write=False)
    assert sum(np.count_nonzero(r[:60]) for r in ref) > 20  # several beta and alpha bins were hit
    return ref


def create(ctx, name, flags=FUSED):
    batch, models, bp = case(name)
    ctx.models_clear()
    ids = ctx.modelsv_create([(m.scalars, m.match, m.skip, m.gap_y) for m in models])
    b = cp.Batch(ctx, make_items(batch, (1, 1)), batch["x_chars"], batch["events"], batch["anchors"], bp,
                 flags=EXP | flags, vanilla=True)
    info = b.info()
    assert info["kernel"] == "systolic" and info["family"] == "wave", info
    assert info["cells_per_lane"] == SHAPES[name]["cells"], info
    assert info["fused_expectations"] == (1 if flags & FUSED else 0), info
    return b, ids


def sums(b, ids):
    b.run()
    b.sync()
    return [b.expectations(mid) for mid in ids]


def assert_oracle(got, ref, what=""):
    assert len(got) == len(ref)
    for k, (g, r) in enumerate(zip(got, ref)):
        err = np.abs(g[:60] - r[:60]) / np.maximum(np.abs(r[:60]), 1e-300)
        print("%s model %d: largest relative error of the bins %.3g, of the likelihood %.3g" % (
            what, k, err[r[:60] != 0].max(initial=0.0), abs(g[60] - r[60]) / abs(r[60])))
        assert np.allclose(g[:60], r[:60], rtol=1e-9, atol=1e-12), (what, k)
        assert np.isclose(g[60], r[60], rtol=1e-12, atol=0) and g[60] < 0, (what, k, g[60], r[60])


@pytest.fixture(scope="module")
def ctx():
    c = cp.Context(0)
    yield c
    c.close()


def test_the_flag_exists():
    assert FUSED == 16384


@pytest.mark.parametrize("name", ["two-cells", "three-cells", "no-anchors"])
def test_fused_batches_match_the_oracle(ctx, name):
    b, ids = create(ctx, name)
    got = sums(b, ids)
    b.close()
    assert_oracle(got, oracle(name), name)


@pytest.mark.parametrize("name", ["two-cells", "three-cells"])
def test_fused_against_the_ring_of_backward_cells(ctx, name):
    b, ids = create(ctx, name, flags=0)
    ring = sums(b, ids)
    b.close()
    b, ids = create(ctx, name)
    fused = sums(b, ids)
    b.close()
    for f, r in zip(fused, ring):
        assert np.count_nonzero(r[:60]) > 5
        assert np.allclose(f[:60], r[:60], rtol=1e-11, atol=1e-300)
        assert np.isclose(f[60], r[60], rtol=1e-12, atol=0)


@pytest.mark.parametrize("name", ["two-cells", "three-cells"])
@pytest.mark.parametrize("resweep", [1, 2], ids=["every-window", "every-other-window"])
def test_windows_down_the_fallback(ctx, name, resweep, monkeypatch):
    """CPECAN_EXPECT_RESWEEP=1: every window swept back once more against the exact totals; 2: every other one (items
    and windows alternate), so that a model's sums come from both paths"""
    monkeypatch.setenv("CPECAN_EXPECT_RESWEEP", str(resweep))
    b, ids = create(ctx, name)
    got = sums(b, ids)
    b.close()
    assert_oracle(got, oracle(name), "%s resweep %d" % (name, resweep))


def test_chained_rounds_and_two_contexts():
    """two batches of two contexts, the second run behind the first (run(after=...)), three rounds: the segment records
    in scratch are reused from round to round"""
    names = ("two-cells", "two-cells-b")
    ctxs = [cp.Context(0), cp.Context(0)]
    made = [create(c, name) for c, name in zip(ctxs, names)]
    refs = [oracle(name) for name in names]
    for round_ in range(3):
        made[0][0].run()
        made[1][0].run(after=made[0][0])
        for (b, ids), ref, name in zip(made, refs, names):
            b.sync()
            assert_oracle([b.expectations(mid) for mid in ids], ref, "%s round %d" % (name, round_))
    for b, _ in made:
        b.close()
    for c in ctxs:
        c.close()


def test_persistent_e_step_after_new_bins_in_place():
    """em.PersistentVanillaEStep with the flag: an iteration, the skip bins rewritten in place
    (cpecan_hip_modelsv_set_skip_probs), a second iteration -- equal to a fresh fused batch on tables built with the new
    bins"""
    import torch
    sh = SHAPES["two-cells"]
    batch, bases, strand_of, _ = two_strand_batch(65, 6, sh["lX"], sh["lY"], sh["every"])
    bp = band_params(0.01, sh["md"], sh["tb"], sh["e"])
    ctx = cp.Context(0)
    step = em().PersistentVanillaEStep(cp, [ctx], batch, bp, range(6), [as_tuple(m) for m in bases], strand_of, flags=FUSED)
    info = step.batches[0][1].info()
    assert info["fused_expectations"] == 1 and info["cells_per_lane"] == 2, info
    first = step(bases[0].skip.copy())
    second = step(NEW_BINS)
    fresh = cp.Context(0)
    ids = fresh.modelsv_create([host_scaled(bases[strand_of[i]], batch["scalings"][i], NEW_BINS) for i in range(6)])
    items = np.zeros(6, cp.ITEM_DTYPE)
    for i, it in enumerate(batch["items"]):
        items[i] = (it["x_offset"], it["lX"], it["y_offset"], it["lY"], it["anchor_offset"], it["n_anchors"], ids[i], 1, 1, 0)
    b = cp.Batch(fresh, items, batch["x_chars"], batch["events"], batch["anchors"], bp, flags=EXP | FUSED, vanilla=True)
    assert b.info()["fused_expectations"] == 1
    b.run()
    b.sync()
    ptr, n = b.expectations_device_ptr()  # added up as the persistent step adds them: one sum on the device
    want = torch.as_tensor(em()._DeviceDoubles(ptr, n), device="cuda:0").view(-1, 61).sum(0).cpu().numpy()
    b.close()
    assert second.shape == (61,) and np.count_nonzero(want[:60]) > 20 and want[60] < 0
    assert np.allclose(second, want, rtol=1e-12, atol=1e-300)
    assert not np.allclose(second, first, rtol=1e-3, atol=0)  # the new bins are other bins
    step.close()
    fresh.close()
    ctx.close()


def test_host_library_in_a_fresh_process(tmp_path, golden_dir):
    """CPECAN_VANILLA_FUSED_ESTEP=1 in a child process: the reference-shaped vanilla E-step call of libcpecan_host.so on
    the reads of the two-cell shape gives the oracle's sums.  (Which path the call took cannot be seen through the
    reference's interface: results only; the choice itself is covered at the C-ABI.)"""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "vanilla_fused_host_child.py")
    path = str(tmp_path / "sums.json")
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, child, path],
                       env=dict(os.environ, CPECAN_VANILLA_FUSED_ESTEP="1"), capture_output=True, text=True, timeout=150)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.array(json.load(open(path)))
    sh = SHAPES["two-cells"]
    batch = case("two-cells")[0]
    match, skip, gapy = o.load_pore_model(os.path.join(golden_dir, "template_median68pA.model"))
    model = o.VanillaModel(match, skip, gapy, *FUDGE[0])
    p = o.default_params(threshold=0.01, minDiagsBetweenTraceBack=sh["md"], traceBackDiagonals=sh["tb"],
                         diagonalExpansion=sh["e"])
    hmm = o.OrcExpectationsV()
    for it in batch["items"]:
        x = batch["x_chars"][it["x_offset"]: it["x_offset"] + it["lX"] + 5]
        ev = batch["events"][it["y_offset"]: it["y_offset"] + it["lY"]]
        an = batch["anchors"][it["anchor_offset"]: it["anchor_offset"] + it["n_anchors"]]
        o.expectations_v_using_anchors(model, x, it["lX"], ev, an, p, hmm, True, True)
    ref = hmm.as_array()
    assert np.count_nonzero(ref[:60]) > 20
    assert_oracle([got], [ref], "host library")

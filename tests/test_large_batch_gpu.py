"""Batches of more than 65 535 alignments: every per-item launch that puts the item in grid.y caps it at 65 535 and
strides (the k-mer track of the wave, vanilla, HDP and workgroup kernels, the assembly sweeps' mask table).

65 600 items over 61 distinct prototype reads of about 140 k-mers x 280 events, item i on the inputs of prototype
i % 61: 61 shares no factor with 65 535 or 65 536, so an item index that wraps or is clamped lands on another
prototype's answer.  One shared model.  The oracle runs the 61 prototypes; every item is compared with its
prototype's result.

Device footprint.  Traceback every 24 diagonals, 8 back, diagonalExpansion 60 or 100 (bands of 109 or 129 k-mers,
narrow enough for a traceback point on every diagonal past the 24th): a window spans 25 diagonals and every ring has
the minimum of 64 rows (+ 1 on the wave kernels).  Per read, and for the 65 600:
  wave, 2 cells per lane:   ring 65 x 5 KB = 333 KB, scratch 112 KB, track 23 KB:           ~0.47 MB, ~31 GB
  assembly sweeps (small):  ring 65 x 7.5 KB = 499 KB, scratch 166 KB, contexts 111 KB,
                            track 23 KB, masks 27 KB:                                         ~0.83 MB, ~55 GB
  workgroup, 2 waves:       ring 64 x 5 KB = 328 KB, scratch 40 KB, track 23 KB:            ~0.4 MB,  ~26 GB
(no batch of more than 65 535 alignments on the assembly sweeps takes much less: their ring, scratch and contexts are
at their minimum here).  Each batch is closed (and the library's cache trimmed) before the next is made; the test
prints what each took and holds it under 64 GB."""
import numpy as np
import pytest

import pyoracle as o
import synth
from harness import (assert_same_pairs, assert_same_posterior, band_params, batch_results, cp, hdp_batch,
                     make_items, run_oracle_hdp_item, run_oracle_item)

pytestmark = pytest.mark.gpu

N_ITEMS = 65_600
N_PROTO = 61


@pytest.fixture(scope="module")
def ctx():
    c = cp.Context(0)
    yield c
    c.close()


def tiled(proto_items):
    """N_ITEMS items, item i = prototype i % N_PROTO (same input offsets)"""
    return np.ascontiguousarray(proto_items[np.arange(N_ITEMS) % N_PROTO])


def free_bytes():
    import torch
    return torch.cuda.mem_get_info(0)[0]


def run_large(ctx, proto, bp, ragged, what, **kw):
    """runs the tiled batch; returns (results of every item, info)"""
    cp.trim_cache()
    before = free_bytes()
    b = cp.Batch(ctx, tiled(make_items(proto, ragged)), proto["x_chars"], proto["events"], proto["anchors"], bp, **kw)
    info = b.info()
    b.run()
    b.sync()
    used = before - free_bytes()
    print("%s: %d items, device footprint %.1f GB, %r" % (what, N_ITEMS, used / 1e9, info))
    assert used < 64e9
    res = batch_results(b)
    b.close()
    cp.trim_cache()
    return res, info


def check_every_item(res, refs, full=True):
    for i, g in enumerate(res):
        r = refs[i % N_PROTO]
        if full:
            assert_same_posterior(g, r, i)
        else:
            assert np.array_equal(g["totals_xay"], r["totals_xay"]), i
            assert np.array_equal(g["totals"], r["totals"]), i
            assert_same_pairs(g, r)


@pytest.fixture(scope="module")
def proto():
    return synth.make_batch(111, N_PROTO, 140, 280, anchor_every=50, distinct_models=False)


@pytest.mark.parametrize("case", [
    dict(id="wave-compiled", e=60, flags=0, family="wave", build=2, asm=0),
    dict(id="assembly-small-footprint", e=100, flags=cp.FLAG_SMALL_FOOTPRINT, family="wave", build=3, asm=2),
    dict(id="workgroup", e=60, flags=cp.FLAG_WORKGROUP_KERNELS, family="workgroup", build=2),
], ids=lambda c: c["id"])
def test_strawman_batch_of_65600(ctx, proto, case):
    bp = band_params(0.01, 24, 8, case["e"])
    refs = [run_oracle_item(proto, i, bp, (1, 1)) for i in range(N_PROTO)]
    ctx.models_clear()
    ctx.models_create([(cp.NANOPORE_TRANSITIONS,) + proto["models"][0]])
    res, info = run_large(ctx, proto, bp, (1, 1), case["id"], kernel=cp.KERNEL_AUTO, flags=case["flags"])
    assert info["kernel"] == "systolic" and info["family"] == case["family"], info
    assert info["waves_per_workgroup"] == case["build"], info
    if case["family"] == "wave":
        assert info["assembly_sweeps"] == case["asm"], info
    check_every_item(res, refs)


def test_vanilla_batch_of_65600(ctx, proto):
    match, _, gapy = proto["models"][0]
    skip = np.sort(np.random.default_rng(3).uniform(0.05, 0.4, 30))[::-1].copy()
    model = o.VanillaModel(match, skip, gapy, float(np.float32(0.17)), float(np.float32(0.55)))
    bp = band_params(0.01, 24, 8, 60)
    p = o.default_params(threshold=bp.threshold, minDiagsBetweenTraceBack=bp.minDiagsBetweenTraceBack,
                         traceBackDiagonals=bp.traceBackDiagonals, diagonalExpansion=bp.diagonalExpansion,
                         splitMatrixBiggerThanThis=1 << 60)
    refs = []
    for it in proto["items"]:
        x = proto["x_chars"][it["x_offset"]: it["x_offset"] + it["lX"] + 5]
        ev = proto["events"][it["y_offset"]: it["y_offset"] + it["lY"]]
        an = proto["anchors"][it["anchor_offset"]: it["anchor_offset"] + it["n_anchors"]]
        r = o.aligned_pairs_using_anchors(model, x, it["lX"], ev, an, p, 1, 1)
        r["triples"], r["logp"] = r["triples"][::-1], r["logp"][::-1]
        refs.append(r)
    ctx.models_clear()
    ctx.modelsv_create([(model.scalars, model.match, model.skip, model.gap_y)])
    res, info = run_large(ctx, proto, bp, (1, 1), "vanilla", vanilla=True)
    assert info["kernel"] == "systolic" and info["family"] == "wave", info
    check_every_item(res, refs, full=False)


def test_hdp_batch_of_65600(ctx, golden_dir):
    import os
    nhdp = o.load_nhdp(os.path.join(golden_dir, "testTemplate.nhdp"))
    proto, model = hdp_batch(112, N_PROTO, 140, 20, nhdp)  # (anchors every 20: bands of 110, short windows)
    bp = band_params(0.01, 24, 8, 60)
    refs = [run_oracle_hdp_item(proto, i, bp, model, (1, 1)) for i in range(N_PROTO)]
    ctx.models_clear()
    ctx.modelsh_create([(cp.NANOPORE_TRANSITIONS, nhdp["alphabet"], nhdp["grid"], nhdp["y"], nhdp["slope"],
                         nhdp["kmer_row"])])
    res, info = run_large(ctx, proto, bp, (1, 1), "hdp", hdp=True)
    assert info["kernel"] == "systolic" and info["family"] == "wave", info
    check_every_item(res, refs, full=False)

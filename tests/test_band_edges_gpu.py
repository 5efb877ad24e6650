"""Reads whose alignment runs on the band's edges (tests/edge_reads.py) on every kernel path that takes their width,
against the oracle at the suite's bars.  With synth's reads an edge cell holds almost no mass, so a kernel that gets it
wrong (a stale ring value for an out-of-band predecessor, a dropped last lane, a wrapped slot at the widest band)
leaves every total and pair unchanged; with these reads the mass is on the edge.

- posterior: the general kernel's cells bit-identical to the oracle's dump; the wave builds (L = 2, 3, 4), the assembly
  sweeps in both ring layouts, the workgroup family (1-4 waves): cells, totals and pairs as the oracle's
- E-step: the fused sums, the re-sweep (all windows, every other one), the B ring, the workgroup family, the general
  kernel: totals bit-identical, expectations to rtol 1e-9, fused against the ring to 1e-11, the gap-X invariant
- vanilla: the wave builds (L = 2, 3; vanilla has no L = 4 build) and the general kernel, as test_random_case_vanilla
- HDP: path-first reads with events around each k-mer's HDP mode on the HDP wave builds (L = 2, 3, 4) and the general
  kernel, as test_random_case_hdp
- stale state: each posterior case once more on a context whose ring and scratch a centred batch with the same band
  (the same kernel and build) has just used, and as the follower in a run_after chain on two contexts (the
  benchmark's ping-pong)
"""
import os

import numpy as np
import pytest

import edge_reads as er
from harness import assert_same_posterior, band_params, batch_results, cp, make_items, run_gpu, run_oracle_item
from test_fuzz_expectations_gpu import (assert_expectations_match, assert_gap_x_invariant, assert_path,
                                        assert_same_totals, env, oracle_of, run_expectations)

pytestmark = pytest.mark.gpu

# CPECAN_FUZZ_SCALE=N runs N seeds of every family (the first is the default run's)
SCALE = max(1, int(os.environ.get("CPECAN_FUZZ_SCALE", "1")))
THRESHOLDS = (0.01, 1e-4, 0.0)


@pytest.fixture(scope="module")
def ctx():
    c = cp.Context(0)
    yield c
    c.close()


def batch_of(name, k, **kw):
    """family `name`'s batch; k > 0: the same family on another seed (kw: centred, hdp, as edge_reads.edge_batch)"""
    f = er.FAMILIES[name]
    return f, er.family_batch(name, seed=f["seed"] + 100 * k, **kw)


def widest_of(batch):
    return max(er.widest(batch["anchors"][it["anchor_offset"]: it["anchor_offset"] + it["n_anchors"]], it["lX"],
                         it["lY"], batch["e"]) for it in batch["items"])


def posterior_paths(w):
    """(name, kernel, flags, CPECAN_ASM) of every path that takes a band `w` k-mers wide"""
    out = [("general", cp.KERNEL_GENERAL, 0, None)]
    if w <= 248:
        out.append(("wave", cp.KERNEL_AUTO, 0, "0"))
        out.append(("workgroup", cp.KERNEL_AUTO, cp.FLAG_WORKGROUP_KERNELS, None))
    if 120 < w <= 158:
        out.append(("assembly", cp.KERNEL_AUTO, 0, None))
        out.append(("assembly-small", cp.KERNEL_AUTO, cp.FLAG_SMALL_FOOTPRINT, None))
    return out


def assert_posterior_path(info, path, w):
    if path == "general":
        assert info["kernel"] == "general", info
        return
    assert info["kernel"] == "systolic", info
    if path == "workgroup":
        assert info["family"] == "workgroup", info
        assert info["waves_per_workgroup"] == 1 + (w > 56) + (w > 120) + (w > 184), info
    elif path == "wave":
        assert info["family"] == "wave" and info["cells_per_lane"] == 2 + (w > 120) + (w > 184), info
        assert not info.get("assembly_sweeps"), info
    else:
        assert info["assembly_sweeps"] == 2, info


CASES = [(n, k) for k in range(SCALE) for n in er.FAMILIES]


def case_id(c):
    return "%s-%d" % c


_REF = {}


def oracle_posterior(key, batch, bp, ragged):
    if key not in _REF:
        _REF[key] = [run_oracle_item(batch, i, bp, ragged) for i in range(len(batch["items"]))]
    return _REF[key]


# ----------------------------------------------- strawMan posterior -----------------------------------------------


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_edge_posterior(ctx, case):
    """every path that takes the case's width at every threshold (0.01, 1e-4, 0); the general kernel's cells against
    the oracle's dump"""
    name, k = case
    f, batch = batch_of(name, k)
    w = widest_of(batch)
    if k == 0 and f["width"] is not None:
        assert w == f["width"]
    for path, kernel, flags, asm in posterior_paths(w):
        for thr in THRESHOLDS:
            bp = band_params(thr, f["md"], f["tb"], batch["e"])
            dump = path == "general"
            with env(CPECAN_ASM=asm):
                res, b = run_gpu(ctx, batch, bp, kernel=kernel, flags=flags | (cp.FLAG_DEBUG_DUMP if dump else 0),
                                 ragged=f["ragged"])
            info = b.info()
            assert info["max_band_width"] == w
            assert_posterior_path(info, path, w)
            ref = oracle_posterior((name, k, thr), batch, bp, f["ragged"])
            for i in range(len(batch["items"])):
                assert_same_posterior(res[i], ref[i], (path, thr, i))
                if dump:
                    d = run_oracle_item(batch, i, bp, f["ragged"], dump=True)
                    F, B = b.debug_cells(i, d["F"].shape[0])
                    assert np.array_equal(F, d["F"]), (name, i, "forward cells differ")
                    ok = ~np.isnan(d["B"][:, 0])  # diagonal 0 gets no posterior pass
                    assert np.array_equal(B[ok], d["B"][ok]), (name, i, "backward cells differ")
            b.close()


@pytest.mark.parametrize("waves", [1, 2])
def test_workgroup_threshold_zero_keeps_pairs_of_exponent_minus_inf(ctx, waves):
    """regression: at threshold 0 every in-band cell is a pair, one whose F + B is -inf too (exp(-inf) = 0 >= 0).
    The workgroup family decoded from its candidates, which leave such cells out (27 of 19020 pairs missing on the
    crossing case); it now decodes by the scan at threshold 0, as the wave kernels do"""
    f, batch = batch_of("cross" if waves == 1 else "w120", 0)
    bp = band_params(0.0, f["md"], f["tb"], batch["e"])
    res, b = run_gpu(ctx, batch, bp, kernel=cp.KERNEL_AUTO, flags=cp.FLAG_WORKGROUP_KERNELS, ragged=f["ragged"])
    info = b.info()
    b.close()
    assert info["family"] == "workgroup" and info["waves_per_workgroup"] == waves, info
    ref = oracle_posterior((f["seed"], "thr0", waves), batch, bp, f["ragged"])
    assert any(np.any(r["logp"] == -np.inf) for r in ref)
    for i in range(len(batch["items"])):
        assert_same_posterior(res[i], ref[i], i)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_edge_posterior_after_centred_batch(ctx, case):
    """on the path AUTO picks: a centred batch first, on the same context (its ring and scratch), then the edge batch;
    then the edge batch as the follower of a run_after chain on a second context.  The centred batch has the edge
    batch's sequences and anchors, so the same band and the same path; its events come from the nominal path the
    anchors sit on, so its mass runs down the band's middle"""
    name, k = case
    f, batch = batch_of(name, k)
    _, centred = batch_of(name, k, centred=True)
    bp = band_params(0.01, f["md"], f["tb"], batch["e"])
    ref = oracle_posterior((name, k, 0.01), batch, bp, f["ragged"])
    _, b0 = run_gpu(ctx, centred, bp, kernel=cp.KERNEL_AUTO, ragged=f["ragged"])
    i0 = b0.info()
    b0.close()
    res, b = run_gpu(ctx, batch, bp, kernel=cp.KERNEL_AUTO, ragged=f["ragged"])
    i1 = b.info()
    b.close()
    assert i0 == i1, (i0, i1)  # the same kernel, build, layout and widest band
    for i in range(len(batch["items"])):
        assert_same_posterior(res[i], ref[i], ("after a centred batch", i))
    # the benchmark's ping-pong: the centred batch on this context, the edge batch on a second one behind it, then
    # the edge batch here again behind that
    ctx2 = cp.Context(0)
    try:
        cen = new_batch(ctx, centred, bp, f["ragged"])
        b2 = new_batch(ctx2, batch, bp, f["ragged"])
        cen.run()
        b2.run(after=cen)
        b2.sync()
        cen.sync()
        cen.close()
        b1 = new_batch(ctx, batch, bp, f["ragged"])
        b1.run(after=b2)
        b1.sync()
        for bb in (b2, b1):
            for i, g in enumerate(batch_results(bb)):
                assert_same_posterior(g, ref[i], ("chain", i))
        b2.close()
        b1.close()
    finally:
        ctx2.close()


def new_batch(cx, bt, bp, ragged):
    """a batch on the AUTO path with the batch's models uploaded to its context (not run)"""
    cx.models_clear()
    cx.models_create([(cp.NANOPORE_TRANSITIONS, m, gx, gy) for (m, gx, gy) in bt["models"]])
    return cp.Batch(cx, make_items(bt, ragged), bt["x_chars"], bt["events"], bt["anchors"], bp, 0, cp.KERNEL_AUTO, 0)


# ------------------------------------------------- strawMan E-step -------------------------------------------------

E_VARIANTS = ["fused", "ring", "workgroup", "resweep", "half", "general"]
E_CASES = [(n, k) for k in range(SCALE) for n in ("arec120", "arec184", "upper", "lower", "cross", "w57", "w121",
                                                  "w185", "w248", "w249")]


@pytest.mark.parametrize("case,variant", [(c, v) for c in E_CASES for v in E_VARIANTS
                                          if not (v in ("workgroup", "general") and c[0] == "w249")],  # (AUTO: general)
                         ids=lambda x: case_id(x) if isinstance(x, tuple) else x)
def test_edge_expectations(ctx, case, variant):
    """the E-step on every path; the A-record cases among them (bands at a wave build's widest with skipped k-mers
    at the sweep back's trailing edge)"""
    name, k = case
    f, batch = batch_of(name, k)
    w = widest_of(batch)
    bp = band_params(0.01, f["md"], f["tb"], batch["e"])
    ref_items, ref = oracle_of(("edge", name, k), batch, bp, f["ragged"], None)
    if variant == "general":  # the general kernel asked for, at bands the systolic kernels would take
        res, b = run_gpu(ctx, batch, bp, mode=cp.MODE_EXPECTATIONS, kernel=cp.KERNEL_GENERAL, ragged=f["ragged"])
        info = b.info()
        got = [b.expectations(j) for j in range(len(batch["models"]))]
        b.close()
        assert info["kernel"] == "general", info
    else:
        res, info, got = run_expectations(ctx, batch, bp, f["ragged"], variant)
        assert_path(info, variant)
    assert info["max_band_width"] == w
    assert_same_totals(res, ref_items, variant)
    for j, (g, r) in enumerate(zip(got, ref)):
        assert_expectations_match(g, r, (variant, j))
        assert_gap_x_invariant(g, (variant, j))
    if variant == "ring" and info["kernel"] == "systolic":
        fused = run_expectations(ctx, batch, bp, f["ragged"], "fused")[2]
        for fu, r in zip(fused, got):
            assert np.allclose(fu[:-1], r[:-1], rtol=1e-11, atol=1e-300)
            assert np.isclose(fu[-1], r[-1], rtol=1e-12)


# ----------------------------------------------------- vanilla -----------------------------------------------------


@pytest.mark.parametrize("case", [(n, k) for k in range(SCALE) for n in ("upper", "lower", "w120", "w184", "w248",
                                                                              "w249")],
                         ids=case_id)
def test_edge_vanilla(ctx, case):
    import pyoracle as o
    import test_vanilla_gpu as tv
    name, k = case
    f, batch = batch_of(name, k)
    models = [o.VanillaModel(m, tv.skip_bins(i), gy) for i, (m, _, gy) in enumerate(batch["models"])]
    tv.run(ctx, batch, models, band_params(0.01, f["md"], f["tb"], batch["e"]), f["ragged"])


# ------------------------------------------------------- HDP -------------------------------------------------------


@pytest.fixture(scope="module")
def hdp(golden_dir):
    import pyoracle as o
    nhdp = o.load_nhdp(os.path.join(golden_dir, "testTemplate.nhdp"))
    return nhdp, o.HdpModel(nhdp)


@pytest.mark.parametrize("case", [(n, k) for k in range(SCALE) for n in ("upper", "lower", "cross", "w120", "w121",
                                                                         "w184", "w185", "w248", "w249")],
                         ids=case_id)
def test_edge_hdp(ctx, case, hdp):
    """path-first reads for the HDP machine (events around each k-mer's HDP mode) on the HDP wave builds (two, three,
    four cells per lane) and, past 248 k-mers, the general kernel: the bar of test_random_case_hdp"""
    from harness import run_oracle_hdp_item
    nhdp, model = hdp
    name, k = case
    f, batch = batch_of(name, k, hdp=hdp)
    w = widest_of(batch)
    ctx.models_clear()
    ctx.modelsh_create([(cp.NANOPORE_TRANSITIONS, nhdp["alphabet"], nhdp["grid"], nhdp["y"], nhdp["slope"],
                         nhdp["kmer_row"])])
    for thr in THRESHOLDS:
        bp = band_params(thr, f["md"], f["tb"], batch["e"])
        b = cp.Batch(ctx, make_items(batch, f["ragged"]), batch["x_chars"], batch["events"], batch["anchors"], bp,
                     hdp=True)
        info = b.info()
        assert info["max_band_width"] == w
        if w <= 248:
            assert info["kernel"] == "systolic" and info["family"] == "wave", info
            assert info["cells_per_lane"] == 2 + (w > 120) + (w > 184), info
        else:
            assert info["kernel"] == "general", info
        b.run()
        b.sync()
        res = batch_results(b)
        b.close()
        for i in range(len(batch["items"])):
            assert_same_posterior(res[i], run_oracle_hdp_item(batch, i, bp, model, f["ragged"]), (thr, i))

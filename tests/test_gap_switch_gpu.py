"""Transitions with a finite GAP_SWITCH_TO_X (gap Y -> gap X) against the oracle.

A trained model has one: continuousPairHmm_loadTransitionsAndKmerGapProbs sets it to log(E[gapY -> gapX]), finite
after one Baum-Welch step with any pseudocount (em.m_step does the same).  A batch of such a model runs other code
than the nanopore defaults (switch -inf) do: the wave family's _sw builds of the forward, backward, re-sweep and
expectation kernels -- also on a batch planned and laid out for the assembly sweeps, which have no switch term and
stand aside at run time -- the workgroup family's switch branches, the general kernel's switch term and the HDP
machine's.  Two transition sets:
  strong:  the nanopore defaults with the gap-Y row renormalised around a switch of 0.1, so that a dropped or misplaced
           term moves the totals;
  trained: em.m_step of one GPU E-step of the nanopore defaults with the reference's pseudocount of 1e-4 per read,
           a tiny switch as trained models have.
The bar is the suite's: cells, totals and exponents bit-identical, expectations to rtol 1e-9."""
import os

import numpy as np
import pytest

import pyoracle as o
import synth
from harness import (assert_same_posterior, band_params, batch_results, cp, hdp_batch, make_items, run_gpu,
                     run_oracle_hdp_item, run_oracle_item, trained_transitions, with_gap_switch, with_gap_x)

STRONG = with_gap_switch(cp.NANOPORE_TRANSITIONS, 0.1)


@pytest.fixture(scope="module")
def ctx():
    c = cp.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def trained(ctx):
    """(transitions, gap_x) after one EM step from the nanopore defaults"""
    t, gx = trained_transitions(ctx)
    assert np.isfinite(t[7]) and t[7] < np.log(0.01)  # a tiny switch, as trained models have
    return t, gx


@pytest.fixture(params=["strong", "trained"])
def tset(request):
    """(name, transitions, gap_x or None for the batch's own)"""
    if request.param == "strong":
        return "strong", STRONG, None
    t, gx = request.getfixturevalue("trained")
    return "trained", t, gx


_ORACLE = {}


def oracle(batch_key, batch, i, bp, ragged, name, t):
    """run_oracle_item once per distinct read, band, threshold and transition set"""
    key = (batch_key, i, bp.threshold, bp.minDiagsBetweenTraceBack, bp.traceBackDiagonals, bp.diagonalExpansion,
           ragged, name)
    if key not in _ORACLE:
        _ORACLE[key] = run_oracle_item(batch, i, bp, ragged, transitions=t)
    return _ORACLE[key]


def test_strong_switch_moves_the_oracle():
    """(CPU) the strong set changes every total the oracle computes: a kernel that drops the switch term cannot pass"""
    batch = synth.make_batch(81, 3, 150, 310, anchor_every=25)
    bp = band_params(0.01, 60, 10, 20)
    for i in range(3):
        a = run_oracle_item(batch, i, bp, (1, 1))
        b = run_oracle_item(batch, i, bp, (1, 1), transitions=STRONG)
        assert a["cells"] == b["cells"]
        assert not np.any(np.asarray(a["totals"]) == np.asarray(b["totals"]))


# the batch shapes, and what the library must build for them
SHAPES = dict(
    w2=dict(seed=81, n=3, lX=150, lY=310, every=25, e=20, md=60, tb=10),     # bands of 46-47: 2 cells per lane
    asm=dict(seed=82, n=3, lX=700, lY=1400, every=50, e=100, md=300, tb=40),  # 121-158: planned for the assembly sweeps
    w3=dict(seed=83, n=2, lX=600, lY=1200, every=50, e=120, md=300, tb=40),   # 171-173: 3 cells per lane, compiled
    w4=dict(seed=84, n=2, lX=600, lY=1200, every=50, e=180, md=400, tb=40),   # 231-233: 4 cells per lane
    w40=dict(seed=85, n=3, lX=300, lY=610, every=50, e=40, md=100, tb=40),    # 91
)
CASES = [
    dict(id="wave-2", shape="w2", flags=0, family="wave", build=2, asm=0),
    dict(id="wave-asm-ring3", shape="asm", flags=0, family="wave", build=3, asm=2),
    dict(id="wave-asm-small", shape="asm", flags=cp.FLAG_SMALL_FOOTPRINT, family="wave", build=3, asm=2),
    dict(id="wave-3", shape="w3", flags=0, family="wave", build=3, asm=0),
    dict(id="wave-4", shape="w4", flags=0, family="wave", build=4, asm=0),
    dict(id="workgroup", shape="w40", flags=cp.FLAG_WORKGROUP_KERNELS, family="workgroup", build=2),
    dict(id="workgroup-wide", shape="asm", flags=cp.FLAG_WORKGROUP_KERNELS, family="workgroup", build=3),
    dict(id="workgroup-rows4", shape="w40", flags=cp.FLAG_WORKGROUP_KERNELS, family="workgroup", build=4, rows=4),
    dict(id="general", shape="w40", flags=0, kernel=cp.KERNEL_GENERAL, family=None),
]


def shape_batch(name):
    s = SHAPES[name]
    return synth.make_batch(s["seed"], s["n"], s["lX"], s["lY"], anchor_every=s["every"])


@pytest.mark.gpu
@pytest.mark.parametrize("threshold", [0.01, 0.0])
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_switch_posteriors_match_oracle(ctx, case, tset, threshold, monkeypatch):
    """every kernel family and build with a finite switch; threshold 0 decodes every cell (the re-sweep path)"""
    name, t, gx = tset
    if case.get("rows"):
        monkeypatch.setenv("CPECAN_SYSTOLIC_ROWS", str(case["rows"]))
    s = SHAPES[case["shape"]]
    batch = with_gap_x(shape_batch(case["shape"]), gx)
    bp = band_params(threshold, s["md"], s["tb"], s["e"])
    res, b = run_gpu(ctx, batch, bp, kernel=case.get("kernel", cp.KERNEL_AUTO), flags=case["flags"], ragged=(1, 1),
                     transitions=t)
    info = b.info()
    if case["family"] is None:
        assert info["kernel"] == "general"
    else:
        assert info["kernel"] == "systolic" and info["family"] == case["family"], info
        assert info["waves_per_workgroup"] == case["build"], info
        if case["family"] == "wave":
            assert info["assembly_sweeps"] == case["asm"], info  # (planned: the switch keeps them aside at run time)
    b.close()
    for i in range(s["n"]):
        ref = oracle(case["shape"], batch, i, bp, (1, 1), name, t)
        assert_same_posterior(res[i], ref, (case["id"], name, i))


@pytest.fixture(scope="module")
def nhdp(golden_dir):
    return o.load_nhdp(os.path.join(golden_dir, "testTemplate.nhdp"))


@pytest.mark.gpu
@pytest.mark.parametrize("threshold", [0.01, 0.0])
@pytest.mark.parametrize("general", [False, True], ids=["wave", "general"])
def test_switch_hdp_matches_oracle(ctx, nhdp, tset, general, threshold):
    """the HDP machine reads its switch from the model's own transitions"""
    name, t, _ = tset
    batch, _ = hdp_batch(91, 2, 300, 40, nhdp)
    model = o.HdpModel(nhdp, transitions=t)
    bp = band_params(threshold, 100, 40, 40)
    ctx.models_clear()
    ctx.modelsh_create([(t, nhdp["alphabet"], nhdp["grid"], nhdp["y"], nhdp["slope"], nhdp["kmer_row"])])
    b = cp.Batch(ctx, make_items(batch, (1, 1)), batch["x_chars"], batch["events"], batch["anchors"], bp,
                 flags=cp.FLAG_GENERAL_KERNEL if general else 0, hdp=True)
    assert b.info()["kernel"] == ("general" if general else "systolic")
    b.run()
    b.sync()
    res = batch_results(b)
    b.close()
    for i in range(len(batch["items"])):
        ref = run_oracle_hdp_item(batch, i, bp, model, (1, 1))
        assert_same_posterior(res[i], ref, (name, i))


@pytest.mark.gpu
@pytest.mark.parametrize("family", [0, cp.FLAG_WORKGROUP_KERNELS], ids=["wave", "workgroup"])
def test_switch_expectations_match_oracle(ctx, tset, family):
    """Baum-Welch expectations with a switch: the expected gap Y -> gap X count is one of the nine"""
    name, t, gx = tset
    batch = with_gap_x(synth.make_batch(86, 3, 300, 610, anchor_every=50, distinct_models=False), gx)
    bp = band_params(0.01, 100, 40, 40)
    res, b = run_gpu(ctx, batch, bp, mode=cp.MODE_EXPECTATIONS, kernel=cp.KERNEL_SYSTOLIC, flags=family,
                     ragged=(1, 1), transitions=t)
    assert b.info()["family"] == ("workgroup" if family else "wave")
    got = b.expectations(0)
    b.close()
    hmm = o.OrcExpectations()
    for i in range(3):
        ref = run_oracle_item(batch, i, bp, (1, 1), transitions=t, expectations=hmm)
        assert np.array_equal(res[i]["totals"], ref["totals"])
    want = np.array(hmm.transitions[:])
    assert want[7] > 0  # the switch was expected to be taken
    assert np.allclose(got[:9], want, rtol=1e-9, atol=1e-12)
    assert np.allclose(got[9:9 + 4096], np.array(hmm.kmerGap[:]), rtol=1e-9, atol=1e-12)
    assert np.isclose(got[-1], hmm.likelihood, rtol=1e-12)


@pytest.mark.gpu
def test_switch_set_in_place_on_a_batch_planned_for_the_assembly_sweeps(ctx):
    """the EM order of events: a batch created under the defaults (planned for the assembly sweeps), then the M-step's
    transitions written into the context's models; run, compare; the switch back to -inf; run, compare"""
    batch = shape_batch("asm")
    s = SHAPES["asm"]
    bp = band_params(0.01, s["md"], s["tb"], s["e"])
    ctx.models_clear()
    ctx.models_create([(cp.NANOPORE_TRANSITIONS, m, gx, gy) for (m, gx, gy) in batch["models"]])
    b = cp.Batch(ctx, make_items(batch, (1, 1)), batch["x_chars"], batch["events"], batch["anchors"], bp)
    assert b.info()["assembly_sweeps"] == 2
    for name, t in (("strong", STRONG), ("defaults", cp.NANOPORE_TRANSITIONS)):
        ctx.models_set_transitions(t)
        b.run()
        b.sync()
        res = batch_results(b)
        for i in range(s["n"]):
            assert_same_posterior(res[i], oracle("asm", batch, i, bp, (1, 1), name, t), (name, i))
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, cp.FLAG_WORKGROUP_KERNELS], ids=["wave", "workgroup"])
def test_mixed_batch_of_switch_and_no_switch_models(ctx, flags):
    """half the reads under the strong set, half under the defaults, in one batch: the batch runs the switch builds,
    and the reads without a switch must still equal the oracle under their own transitions"""
    batch = synth.make_batch(87, 6, 700, 1400, anchor_every=50)
    bp = band_params(0.01, 300, 40, 100)
    ts = [STRONG if k % 2 == 0 else cp.NANOPORE_TRANSITIONS for k in range(6)]
    res, b = run_gpu(ctx, batch, bp, flags=flags, ragged=(1, 1), model_transitions=ts)
    if not flags:
        assert b.info()["assembly_sweeps"] == 2
    b.close()
    for i in range(6):
        ref = run_oracle_item(batch, i, bp, (1, 1), transitions=ts[i])
        assert_same_posterior(res[i], ref, i)

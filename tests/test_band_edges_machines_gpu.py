"""Reads whose alignment runs on the band's edges (tests/edge_reads.py) on the kernels of the machines other than
strawMan, against the oracle at each machine's own bar.  Their existing tests use reads whose mass runs down the
middle of the band, where a kernel that reads a stale or wrapped neighbour at the edge still gives every total and
pair unchanged.

- DNA (5-state) posterior: every DNA family at thresholds 0.01, 1e-4 and 0 on one wave per alignment
  (CPECAN_WAVE5_PAIRED=0), a pair of waves (=1) and the general kernel, as test_dna5_gpu.run_case; the widths sit at
  each wave5 build's limit (64, 128, 192 cells) and one past it, and at the general kernel's LDS limit (248) and its
  256-thread chunk.  Widths 193-248 run the general kernel with its diagonals in LDS, 249 and up through HBM.
- DNA E-step on the same three forms, as test_discrete_expectations_match_oracle.
- vanilla E-step on the wave builds (L = 2, 3) and the general kernel; HDP E-step and event assignments on the HDP
  wave builds (L = 2, 3, 4) and the general kernel.
- 4-state posterior (cpecan_k_general4) at the edges and at bands of 256 k-mers and one past.
- echelon posterior (cpecan_k_generale, against the host DP) at bands of 64 and 256 k-mers and one past: a width test
  only, since the echelon machine's posterior does not follow the reads' path onto the edge.
- stale state: a DNA edge batch right after a centred batch with the same band on the same context, on each form.

CPECAN_FUZZ_SCALE=N runs N seeds of every family (the first is the default run's).
"""
import os

import numpy as np
import pytest

import edge_reads as er
import pyoracle as o
from harness import assert_same_pairs, band_params, cp, make_items, orc_params
from test_dna5_gpu import KERNEL_FORMS, KERNEL_IDS, pick_form
from test_fuzz_expectations_gpu import assert_expectations_match

pytestmark = pytest.mark.gpu

SCALE = max(1, int(os.environ.get("CPECAN_FUZZ_SCALE", "1")))
THRESHOLDS = (0.01, 1e-4, 0.0)


@pytest.fixture(scope="module")
def ctx():
    c = cp.Context(0)
    yield c
    c.close()


def case_id(c):
    return "%s-%d" % c if isinstance(c, tuple) else str(c)


def seed_of(f, k):
    return f["seed"] + 100 * k


_REF = {}


def cached(key, fn):
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


# ------------------------------------------------------- DNA -------------------------------------------------------


def dna_batch(name, k, centred=False):
    f = er.DNA_FAMILIES[name]
    return f, cached(("dna", name, k, centred), lambda: er.dna_batch(name, seed=seed_of(f, k), centred=centred))


def dna_items(ctx, seqs, ragged):
    model = o.Sm5Model()
    ctx.models_clear()
    ids = ctx.models5_create([(list(model.c.t), model.match, model.gx, model.gy)])
    xs, ys, an = "", "", []
    items = np.zeros(len(seqs), cp.ITEM_DTYPE)
    for i, (x, y, a) in enumerate(seqs):
        items[i] = (len(xs), len(x), len(ys), len(y), sum(len(q) for q in an), len(a), ids[0], ragged[0], ragged[1], 0)
        xs += x
        ys += y
        an.append(a)
    return model, ids, items, xs, ys, np.concatenate(an)


def assert_dna_route(info, w, flags):
    assert info["kernel"] == "general" and info["max_band_width"] == w, info
    assert (info.get("family") == "wave (5-state)") == (w <= 192 and not flags & cp.FLAG_GENERAL_KERNEL), info


def run_dna(ctx, key, seqs, bp, ragged, w, flags):
    """test_dna5_gpu.run_case's bar with the oracle cached per case: cells, totals and exponents bit-identical, the
    pairs in the reference's order; and the route the width asks for"""
    model, _, items, xs, ys, anchors = dna_items(ctx, seqs, ragged)
    b = cp.Batch(ctx, items, xs, None, anchors, bp, flags=flags, y_chars=ys)
    assert_dna_route(b.info(), w, flags)
    b.run()
    b.sync()
    npairs, ntot, ncells = b.counts()
    p = orc_params(bp, split=1 << 60)
    for i, (x, y, a) in enumerate(seqs):
        def oracle():
            r = o.aligned_pairs_using_anchors(model, x, len(x), y, a, p, ragged[0], ragged[1])
            r["triples"], r["logp"] = r["triples"][::-1], r["logp"][::-1]  # emission order
            return r
        ref = cached(key + (i,), oracle)
        tri, lp = b.pairs(i, npairs[i])
        xay, tot = b.totals(i, ntot[i])
        assert int(ncells[i]) == ref["cells"], (key, i)
        assert np.array_equal(xay, ref["totals_xay"]), (key, i)
        assert np.array_equal(tot.view(np.uint64), ref["totals"].view(np.uint64)), (key, i)
        assert_same_pairs(dict(triples=tri, logp=lp), ref)
        assert len(tri) > 0
    b.close()


def dna_width(batch):
    return max(er.widest(a, len(x), len(y), batch["e"]) for x, y, a in batch["seqs"])


def dna_forms(names, ids):
    """(case, form) of every family on every form; past 192 cells both wave forms route to the general kernel, so only
    the first (the route asserted) and the general kernel asked for"""
    out = []
    for k in range(SCALE):
        for n in names:
            wide = (er.DNA_FAMILIES[n]["width"] or 0) > er.DNA_WAVE_L3
            out += [pytest.param((n, k), fm, id="%s-%d-%s" % (n, k, i))
                    for fm, i in zip(KERNEL_FORMS, ids) if not (wide and fm == KERNEL_FORMS[1])]
    return out


@pytest.mark.parametrize("case,form", dna_forms(er.DNA_FAMILIES, KERNEL_IDS))
def test_dna_edge_posterior(ctx, case, form, monkeypatch):
    name, k = case
    f, batch = dna_batch(name, k)
    w = dna_width(batch)
    if k == 0 and f["width"] is not None:
        assert w == f["width"]
    flags = pick_form(monkeypatch, form)
    for thr in THRESHOLDS:
        bp = band_params(thr, f["md"], f["tb"], batch["e"])
        run_dna(ctx, ("dna", name, k, thr), batch["seqs"], bp, f["ragged"], w, flags)


@pytest.mark.parametrize("form", KERNEL_FORMS, ids=KERNEL_IDS)
@pytest.mark.parametrize("case", [(n, k) for k in range(SCALE) for n in ("w64", "w128", "w192", "upper")],
                         ids=case_id)
def test_dna_edge_after_centred_batch(ctx, case, form, monkeypatch):
    """a centred batch (the edge batch's x and anchors: the same band, the same kernel and build; its mass down the
    middle), then the edge batch on the same context: the wave5 kernels keep neighbours in registers and the forward
    cells in Fstore, and the edge batch must not see the centred one's"""
    name, k = case
    f, batch = dna_batch(name, k)
    _, centred = dna_batch(name, k, centred=True)
    w = dna_width(batch)
    assert dna_width(centred) == w and centred["e"] == batch["e"]
    flags = pick_form(monkeypatch, form)
    bp = band_params(0.01, f["md"], f["tb"], batch["e"])
    run_dna(ctx, ("dna-centred", name, k, 0.01), centred["seqs"], bp, f["ragged"], w, flags)
    run_dna(ctx, ("dna", name, k, 0.01), batch["seqs"], bp, f["ragged"], w, flags)


DNA_E = ("upper", "lower", "cross", "w64", "w65", "w128", "w129", "w192", "w193", "w249")


@pytest.mark.parametrize("case,form", dna_forms(DNA_E, ["wave5e", "wave5pe", "general5"]))
def test_dna_edge_expectations(ctx, case, form, monkeypatch):
    """the 5-state E-step (25 transitions, 80 emission bins, the likelihood) as test_discrete_expectations_match_oracle:
    rtol 1e-9 / atol 1e-12, the likelihood to 1e-12, non-finite entries where the oracle has them"""
    name, k = case
    f, batch = dna_batch(name, k)
    w = dna_width(batch)
    flags = pick_form(monkeypatch, form) | cp.FLAG_EXPECTATIONS
    bp = band_params(0.01, f["md"], f["tb"], batch["e"])
    model, ids, items, xs, ys, anchors = dna_items(ctx, batch["seqs"], f["ragged"])
    b = cp.Batch(ctx, items, xs, None, anchors, bp, flags=flags, y_chars=ys)
    assert_dna_route(b.info(), w, flags)
    b.run()
    b.sync()
    got = b.expectations(ids[0])
    b.close()

    def oracle():
        hmm = o.OrcExpectations5()
        p = orc_params(bp, split=1 << 60)
        for x, y, a in batch["seqs"]:
            o.expectations5_using_anchors(model, x, len(x), y, a, p, hmm, f["ragged"][0], f["ragged"][1])
        return hmm.as_array()
    ref = cached(("dna-e", name, k), oracle)
    assert ref[-1] < 0 and ref[0] > 10
    assert np.count_nonzero(ref[25:105]) >= 60  # most emission bins are hit
    assert_expectations_match(got, ref, (name, form))


# ----------------------------------------------------- vanilla -----------------------------------------------------


def signal_batch(name, k):
    f = er.signal_family(name)
    return f, cached(("signal", name, k), lambda: er.signal_batch(name, seed=seed_of(f, k)))


def widest_of(batch):
    return max(er.widest(batch["anchors"][it["anchor_offset"]: it["anchor_offset"] + it["n_anchors"]], it["lX"],
                         it["lY"], batch["e"]) for it in batch["items"])


def read_of(batch, it):
    return (batch["x_chars"][it["x_offset"]: it["x_offset"] + it["lX"] + 5],
            batch["events"][it["y_offset"]: it["y_offset"] + it["lY"]],
            batch["anchors"][it["anchor_offset"]: it["anchor_offset"] + it["n_anchors"]])


@pytest.mark.parametrize("general", [False, True], ids=["wave", "general"])
@pytest.mark.parametrize("case", [(n, k) for k in range(SCALE)
                                  for n in ("upper", "lower", "cross", "w120", "w121", "w184", "w185")], ids=case_id)
def test_vanilla_edge_expectations(ctx, case, general):
    """the vanilla E-step (30 beta + 30 alpha skip bins, the likelihood) as test_vanilla_expectations_match_oracle, on
    the wave builds (two, three cells per lane; vanilla has no four-cell build: past 184 k-mers AUTO takes the
    general kernel) and the general kernel"""
    import test_vanilla_gpu as tv
    name, k = case
    f, batch = signal_batch(name, k)
    w = widest_of(batch)
    models = [o.VanillaModel(m, tv.skip_bins(i), gy) for i, (m, _, gy) in enumerate(batch["models"])]
    bp = band_params(0.01, f["md"], f["tb"], batch["e"])
    ctx.models_clear()
    ids = ctx.modelsv_create([(m.scalars, m.match, m.skip, m.gap_y) for m in models])
    b = cp.Batch(ctx, make_items(batch, f["ragged"]), batch["x_chars"], batch["events"], batch["anchors"], bp,
                 flags=cp.FLAG_EXPECTATIONS | (cp.FLAG_GENERAL_KERNEL if general else 0), vanilla=True)
    info = b.info()
    assert info["max_band_width"] == w, info
    if general or w > 184:
        assert info["kernel"] == "general", info
    else:
        assert info["kernel"] == "systolic" and info["family"] == "wave", info
        assert info["cells_per_lane"] == 2 + (w > 120), info
    b.run()
    b.sync()
    got = [b.expectations(mid) for mid in ids]
    b.close()

    def oracle():
        p = orc_params(bp, split=1 << 60)
        hmms = [o.OrcExpectationsV() for _ in models]
        for it in batch["items"]:
            x, ev, an = read_of(batch, it)
            o.expectations_v_using_anchors(models[it["model"]], x, it["lX"], ev, an, p, hmms[it["model"]],
                                           f["ragged"][0], f["ragged"][1])
        return [h.as_array() for h in hmms]
    seen = 0
    for g, ref in zip(got, cached(("vanilla-e", name, k), oracle)):
        assert np.allclose(g, ref, rtol=1e-9, atol=1e-12), (name, np.flatnonzero(~np.isclose(g, ref, 1e-9, 1e-12)))
        assert ref[-1] < 0
        seen += np.count_nonzero(ref[:60])
    assert seen > 20


# ------------------------------------------------------- HDP -------------------------------------------------------


@pytest.fixture(scope="module")
def hdp(golden_dir):
    nhdp = o.load_nhdp(os.path.join(golden_dir, "testTemplate.nhdp"))
    return nhdp, o.HdpModel(nhdp)


@pytest.mark.parametrize("general", [False, True], ids=["wave", "general"])
@pytest.mark.parametrize("case", [(n, k) for k in range(SCALE) for n in ("upper", "lower", "cross", "w120", "w121",
                                                                         "w184", "w185", "w248", "w249")],
                         ids=case_id)
def test_hdp_edge_expectations_and_assignments(ctx, case, general, hdp):
    """the HDP E-step (9 transitions to rtol 1e-9, the likelihood to 1e-12) and each read's event-to-k-mer
    assignments bit-identical and in the reference's order, as test_hdp_expectations_and_assignments_match_oracle; on
    the HDP wave builds (two, three, four cells per lane; past 248 k-mers the general kernel) and the general kernel"""
    nhdp, model = hdp
    name, k = case
    f = er.FAMILIES[name]
    batch = cached(("hdp", name, k), lambda: er.family_batch(name, seed=seed_of(f, k), hdp=hdp))
    w = widest_of(batch)
    ctx.models_clear()
    ids = ctx.modelsh_create([(cp.NANOPORE_TRANSITIONS, nhdp["alphabet"], nhdp["grid"], nhdp["y"], nhdp["slope"],
                               nhdp["kmer_row"])])
    threshold = 0.05
    bp = band_params(threshold, f["md"], f["tb"], batch["e"])
    b = cp.Batch(ctx, make_items(batch, f["ragged"]), batch["x_chars"], batch["events"], batch["anchors"], bp,
                 flags=cp.FLAG_EXPECTATIONS | (cp.FLAG_GENERAL_KERNEL if general else 0), hdp=True)
    info = b.info()
    assert info["max_band_width"] == w, info
    if general or w > 248:
        assert info["kernel"] == "general", info
    else:
        assert info["kernel"] == "systolic" and info["family"] == "wave", info
        assert info["cells_per_lane"] == 2 + (w > 120) + (w > 184), info
    b.run()
    b.sync()
    npairs, _, _ = b.counts()
    got = b.expectations(ids[0])
    per_read = [b.pairs(i, npairs[i]) for i in range(len(batch["items"]))]
    b.close()
    p = orc_params(bp, split=1 << 60)
    reads = [(x, it["lX"], ev, an) for it in batch["items"] for x, ev, an in [read_of(batch, it)]]
    rl, rr = f["ragged"]
    total = cached(("hdp-e", name, k), lambda: o.expectations_h_using_anchors(model, reads, p, threshold, rl, rr))
    assert np.allclose(got[:9], total["transitions"], rtol=1e-9, atol=1e-12)
    assert np.isclose(got[9], total["likelihood"], rtol=1e-12) and total["likelihood"] != 0.0
    n_assign = 0
    for i, rd in enumerate(reads):
        ref = cached(("hdp-a", name, k, i), lambda: o.expectations_h_using_anchors(model, [rd], p, threshold, rl, rr))
        tri, lp = per_read[i]
        assert np.array_equal(tri, ref["assign"]), (name, i)
        assert np.array_equal(lp, ref["logp"]), (name, i)
        n_assign += len(tri)
    assert n_assign > 50 and n_assign == len(total["assign"])


# ----------------------------------------------------- 4-state -----------------------------------------------------


@pytest.mark.parametrize("case", [(n, k) for k in range(SCALE)
                                  for n in ("upper", "lower", "cross", "upper-out", "w256", "w257")], ids=case_id)
def test_sm4_edge_posterior(ctx, case):
    """cpecan_k_general4 at thresholds 0.01, 1e-4 and 0 at test_sm4_gpu.run's bar (totals and exponents
    bit-identical, the pairs in the reference's order); the band at 256 k-mers and one past it is the general
    kernel's 256-thread chunk and one cell into the next"""
    import test_sm4_gpu as t4
    name, k = case
    f, batch = signal_batch(name, k)
    w = widest_of(batch)
    if k == 0 and f["width"] is not None:
        assert w == f["width"]
    models = t4.models_of(batch)
    for thr in THRESHOLDS:
        bp = band_params(thr, f["md"], f["tb"], batch["e"])
        tris = t4.run(ctx, batch, models, bp, f["ragged"])
        assert all(len(t) > 0 for t in tris)
        b = cp.Batch(ctx, make_items(batch, f["ragged"]), batch["x_chars"], batch["events"], batch["anchors"], bp,
                     sm4=True)  # (the models t4.run uploaded)
        assert b.info()["max_band_width"] == w and b.info()["kernel"] == "general", b.info()
        b.close()


# ----------------------------------------------------- echelon -----------------------------------------------------


def echelon_info(ctx, rds, bp, ragged):
    """info() of the batch test_echelon_gpu.run_batch makes of whole reads (not run)"""
    ctx.models_clear()
    ids = ctx.modelse_create([r["machine"].gpu_model() for r in rds])
    items = np.zeros(len(rds), cp.ITEM_DTYPE)
    xs, evs, ao, yo = b"", [], 0, 0
    for i, r in enumerate(rds):
        lX, lY = len(r["seq"]) - 5, len(r["events"])
        items[i] = (len(xs), lX, yo, lY, ao, len(r["anchors"]), ids[i], ragged[0], ragged[1], 0)
        xs += r["seq"]
        evs.append(r["events"])
        ao += len(r["anchors"])
        yo += lY
    b = cp.Batch(ctx, items, xs, np.concatenate(evs), np.concatenate([r["anchors"] for r in rds]), bp, echelon=True)
    info = b.info()
    b.close()
    return info


@pytest.mark.parametrize("case", [(n, k) for k in range(SCALE) for n in ("w64", "w65", "w256", "w257")], ids=case_id)
def test_echelon_wide_band_posterior(ctx, case):
    """cpecan_k_generale against the host DP at thresholds 0.01 and 0 (test_echelon_gpu.same: totals bit-identical,
    the pairs identical) on bands of exactly 64 and 256 k-mers and one past: the general kernel's wave and its
    256-thread chunk.  Not an edge test: the echelon machine's posterior follows no path of these reads (see
    test_band_edges_cpu.py), so little of its mass reaches the band's edge; every cell still enters the totals"""
    import test_echelon_gpu as te
    name, k = case
    f, batch = signal_batch(name, k)
    w = widest_of(batch)
    if k == 0:
        assert w == f["width"]
    rds = er.echelon_reads(batch, seed_of(f, k))
    try:
        pieces = [(r, 0, 0, len(r["seq"]) - 5, len(r["events"]), r["anchors"], f["ragged"][0], f["ragged"][1])
                  for r in rds]
        for thr in (0.01, 0.0):
            bp = band_params(thr, f["md"], f["tb"], batch["e"])
            info = echelon_info(ctx, rds, bp, f["ragged"])
            assert info["kernel"] == "general" and info["machine"] == "echelon" and info["max_band_width"] == w, info
            got = te.run_batch(ctx, pieces, bp)
            for g, pc in zip(got, pieces):
                ref = cached(("echelon", name, k, thr, pc[0]["seq"]), lambda: te.host_piece(*pc, bp))
                te.same(g, ref)
                assert len(ref["triples"]) > 0
    finally:
        for r in rds:
            r["machine"].close()

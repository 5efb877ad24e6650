"""Shared helpers of the GPU parity tests: run work items through the C-ABI, run the same items on
the oracle, and compare."""
import numpy as np

import pyoracle as o
from cpecan_load import binding

cp = binding()

# every environment variable batch creation's kernel choice reads (read_batch_env in cpecan_hip.hip; the plan calls read
# them the same way): what a test of the choice clears first.  tests/test_expectation_pass_dispatch_cpu.py holds it
# against the source
BATCH_ENV = ("CPECAN_DNA_GENERAL", "CPECAN_WIDE_BANDS", "CPECAN_KERNELS", "CPECAN_SYSTOLIC_ROWS", "CPECAN_ASM",
             "CPECAN_WIDE_BANDS_HDP", "CPECAN_WIDE_BANDS_HDP_ESTEP", "CPECAN_WIDE_BANDS_VANILLA_ESTEP", "CPECAN_ASM_NARROW",
             "CPECAN_EXPECT_FUSED_WORKGROUP", "CPECAN_EXPECT_FUSED_WIDE", "CPECAN_EXPECT_FUSED", "CPECAN_EXPECT_RESWEEP",
             "CPECAN_SYSTOLIC_GROUPS", "CPECAN_RING_PAD")


def band_params(threshold=0.01, min_diags=1000, tb_diags=40, expansion=20):
    return cp.BandParams(threshold, min_diags, tb_diags, expansion)


def orc_params(bp, split=3000 * 3000):
    return o.default_params(threshold=bp.threshold, minDiagsBetweenTraceBack=bp.minDiagsBetweenTraceBack,
                            traceBackDiagonals=bp.traceBackDiagonals,
                            diagonalExpansion=bp.diagonalExpansion, splitMatrixBiggerThanThis=split)


def make_items(batch, ragged=(0, 0)):
    items = np.zeros(len(batch["items"]), cp.ITEM_DTYPE)
    for i, it in enumerate(batch["items"]):
        items[i] = (it["x_offset"], it["lX"], it["y_offset"], it["lY"], it["anchor_offset"],
                    it["n_anchors"], it["model"], ragged[0], ragged[1], 0)
    return items


def batch_results(b, items=None):
    """per-item dicts (triples, logp, totals_xay, totals, cells) of a batch that has run and been waited for"""
    npairs, ntot, ncells = b.counts()
    out = []
    for i in range(b.n) if items is None else items:
        tri, lp = b.pairs(i, npairs[i])
        xay, tot = b.totals(i, ntot[i])
        out.append(dict(triples=tri, logp=lp, totals_xay=xay, totals=tot, cells=int(ncells[i])))
    return out


def run_gpu(ctx, batch, bp, mode=0, kernel=0, flags=0, ragged=(0, 0), transitions=None, model_transitions=None):
    """Returns (list of per-item dicts, Batch).  Uploads the batch's models (ids = list index), every one with
    `transitions` (default: the nanopore defaults), or model k with model_transitions[k]."""
    t = transitions if transitions is not None else cp.NANOPORE_TRANSITIONS
    ts = model_transitions if model_transitions is not None else [t] * len(batch["models"])
    ctx.models_clear()
    ctx.models_create([(tk, m, gx, gy) for tk, (m, gx, gy) in zip(ts, batch["models"])])
    b = cp.Batch(ctx, make_items(batch, ragged), batch["x_chars"], batch["events"], batch["anchors"],
                 bp, mode, kernel, flags)
    b.run()
    b.sync()
    return batch_results(b), b


def run_oracle_item(batch, i, bp, ragged=(0, 0), transitions=None, dump=False, expectations=None):
    it = batch["items"][i]
    m, gx, gy = batch["models"][it["model"]]
    model = o.Sm3Model(m, gy, gx, transitions)
    x = batch["x_chars"][it["x_offset"]: it["x_offset"] + it["lX"] + 5]
    ev = batch["events"][it["y_offset"]: it["y_offset"] + it["lY"]]
    an = batch["anchors"][it["anchor_offset"]: it["anchor_offset"] + it["n_anchors"]]
    p = orc_params(bp, split=1 << 60)  # one item == one getPosteriorProbsWithBanding call
    if dump:
        return o.banded_dump(model, x, it["lX"], ev, an, p, ragged[0], ragged[1])
    r = o.aligned_pairs_using_anchors(model, x, it["lX"], ev, an, p, ragged[0], ragged[1],
                                      expectations=expectations)
    r["triples"] = r["triples"][::-1]  # undo the stList_pop reversal: emission order
    r["logp"] = r["logp"][::-1]
    return r


def assert_same_pairs(g, r, exact_logp=True):
    """GPU result g vs oracle result r for one item: same cells, same order; the exponent
    (F+B)-total is bit-identical, and so is the integer posterior floor(p * 1e7): the device selects pairs by the
    exponent, exp() and the threshold test are finished by the C-ABI layer with the host libm, the one the
    reference (and the oracle) calls (impl/pairwiseAligner.c:776-786)."""
    gt, rt = g["triples"], r["triples"]
    if exact_logp:
        assert len(gt) == len(rt), (len(gt), len(rt))
        assert np.array_equal(g["logp"], r["logp"])
        assert np.array_equal(gt, rt)
    else:
        gd = {(int(x), int(y)): int(p) for p, x, y in gt}
        rd = {(int(x), int(y)): int(p) for p, x, y in rt}
        for k in set(gd) ^ set(rd):  # membership may differ only at the threshold itself
            assert abs((gd.get(k) or rd.get(k)) - 100000) <= 2, k
        for k in set(gd) & set(rd):
            assert abs(gd[k] - rd[k]) <= max(1, 1e-6 * rd[k]), (k, gd[k], rd[k])


def assert_same_posterior(g, r, what=""):
    """the posterior bar: cells, totals_xay and totals bit-identical, pairs identical with exact exponents"""
    assert g["cells"] == r["cells"], (what, g["cells"], r["cells"])
    assert np.array_equal(g["totals_xay"], r["totals_xay"]), what
    assert np.array_equal(np.asarray(g["totals"]).view(np.uint64), np.asarray(r["totals"]).view(np.uint64)), what
    assert_same_pairs(g, r)


def with_gap_switch(t, p_switch):
    """strawMan transitions whose gap-Y row (to match, gap-Y extension, switch to gap X) is renormalised to give the
    switch to gap X probability p_switch: the other two keep their ratio"""
    t = np.array(t, dtype=np.float64)
    t[2] = np.log((1.0 - p_switch) * np.exp(t[2]))  # MATCH_FROM_GAP_Y
    t[6] = np.log((1.0 - p_switch) * np.exp(t[6]))  # GAP_EXTEND_Y
    t[7] = np.log(p_switch)                         # GAP_SWITCH_TO_X
    return tuple(float(v) for v in t)


def with_gap_x(batch, gx):
    """the batch with every model's gap-X table replaced (a trained set's); gx None: the batch as it is"""
    if gx is None:
        return batch
    return dict(batch, models=[(m, gx, gy) for (m, _, gy) in batch["models"]])


def trained_transitions(ctx):
    """(transitions, gap_x) after one EM step from the nanopore defaults: em.m_step of one GPU E-step with the
    reference's pseudocount of 1e-4 per read, a tiny finite gap Y -> gap X switch as trained models have"""
    import dist_em
    import synth
    batch = synth.make_batch(47, 6, 150, 310, anchor_every=30)
    got = dist_em.gpu_e_step(cp, ctx, batch, band_params(0.01, 100, 20, 40), list(range(6)), cp.NANOPORE_TRANSITIONS,
                             batch["models"][0][1], pseudocount=1e-4)
    t, gx = dist_em.m_step(got)
    assert np.isfinite(t[7]) and t[7] < np.log(0.01)
    return tuple(float(v) for v in t), gx


def hdp_batch(seed, n, lX, every, nhdp):
    """reads for the HDP machine whose event means are drawn around the mode of each k-mer's HDP density.
    Returns (batch, the oracle's HdpModel with its default transitions)."""
    rng = np.random.default_rng(seed)
    model = o.HdpModel(nhdp)
    xs, evs, ans, items = "", [], [], []
    for _ in range(n):
        x = "".join(rng.choice(list("ACGT"), lX + 5))
        ev, anchors = [], []
        for k in range(lX):
            row = nhdp["kmer_row"][model.kmer_id(x[k:k + 6])]
            mode = nhdp["grid"][int(np.argmax(nhdp["y"][row]))]
            if rng.random() < 0.1:
                continue                                   # skipped k-mer
            if k % every == 0:
                anchors.append((k, len(ev)))
            for _ in range(1 + rng.geometric(0.6) - 1 if rng.random() < 0.5 else 1):
                ev.append((mode + rng.normal(0, 1.0), abs(rng.normal(1.0, 0.2)) + 1e-3, 0.01))
        items.append(dict(x_offset=len(xs), lX=lX, y_offset=sum(len(e) for e in evs), lY=len(ev),
                          anchor_offset=sum(len(a) for a in ans), n_anchors=len(anchors), model=0))
        xs += x
        evs.append(np.array(ev))
        ans.append(np.array(anchors, np.int64).reshape(-1, 2))
    return dict(x_chars=xs, events=np.concatenate(evs), anchors=np.concatenate(ans), items=items), model


def run_oracle_hdp_item(batch, i, bp, model, ragged=(0, 0)):
    """one item of an hdp_batch on the oracle, pairs in emission order"""
    it = batch["items"][i]
    x = batch["x_chars"][it["x_offset"]: it["x_offset"] + it["lX"] + 5]
    ev = batch["events"][it["y_offset"]: it["y_offset"] + it["lY"]]
    an = batch["anchors"][it["anchor_offset"]: it["anchor_offset"] + it["n_anchors"]]
    r = o.aligned_pairs_using_anchors(model, x, it["lX"], ev, an, orc_params(bp, split=1 << 60), ragged[0], ragged[1])
    r["triples"], r["logp"] = r["triples"][::-1], r["logp"][::-1]
    return r

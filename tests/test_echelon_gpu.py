"""GPU parity of the echelon signal machine (cpecan_k_generale through cpecan_hip_modelse_create /
cpecan_hip_batch_create_echelon, and through the host API) against the library's own host cell function driven
diagonal by diagonal (echelon_dp.py).  Bar: every totalProbability refresh bit-identical (np.array_equal), the pairs
of diagonalCalculationMultiPosteriorMatchProbs identical -- coordinates, order, integer posteriors, repeats."""
import ctypes as C
import os

import numpy as np
import pytest

import echelon_dp as e
import host_api as h
import synth
from harness import band_params, cp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = cp.Context(0)
    yield c
    c.close()


def reads(seed, n, lX, lY, anchor_every=20):
    """n synthetic reads, each with a model of its own (the pore model rescaled per read, skip bins of its own)"""
    base, _, gap_y = synth.synthetic_pore_model(seed)
    out = []
    for r in range(n):
        rng = np.random.default_rng(seed * 100 + r)
        rd = synth.make_read(rng, base, lX, lY, anchor_every)
        rd["events"][:, 2] = rng.uniform(0.0008, 0.012, lY)
        skip = np.sort(rng.uniform(0.05, 0.4, 30))[::-1]
        rd["machine"] = e.Machine(rd["scaled_match"], np.concatenate([skip, skip]), gap_y)
        out.append(rd)
    return out


def run_batch(ctx, pieces, bp, flags=0):
    """pieces: (read, x1, y1, x2, y2, anchors relative to the piece, ragged_left, ragged_right) -> the batch's pairs
    and totals per piece; the read's characters go in whole, the piece's look-ahead reads on into the rest of them"""
    ctx.models_clear()
    rds = []
    for pc in pieces:
        if not any(pc[0] is r for r in rds):
            rds.append(pc[0])
    ids = ctx.modelse_create([r["machine"].gpu_model() for r in rds])
    xs, evs, ans, off = b"", [], [], {}
    for k, r in enumerate(rds):
        off[id(r)] = (len(xs), sum(len(v) for v in evs))
        xs += r["seq"]
        evs.append(r["events"])
    items = np.zeros(len(pieces), cp.ITEM_DTYPE)
    ao = 0
    for i, (r, x1, y1, x2, y2, an, rl, rr) in enumerate(pieces):
        xo, yo = off[id(r)]
        lXr = len(r["seq"]) - 5
        items[i] = (xo + x1, x2 - x1, yo + y1, y2 - y1, ao, len(an), ids[[q is r for q in rds].index(True)], rl, rr,
                    min(30, lXr - x2))
        ans.append(np.asarray(an, np.int64).reshape(-1, 2))
        ao += len(an)
    b = cp.Batch(ctx, items, xs, np.concatenate(evs), np.concatenate(ans) if ans else np.zeros((0, 2), np.int64), bp,
                 flags=flags, echelon=True)
    info = b.info()
    assert info["kernel"] == "general" and info["machine"] == "echelon"
    b.run()
    b.sync()
    npairs, ntot, _ = b.counts()
    out = []
    for i in range(len(pieces)):
        tri, logp = b.pairs(i, npairs[i])
        xay, tot = b.totals(i, ntot[i])
        out.append(dict(triples=tri, logp=logp, totals_xay=xay, totals=tot))
    b.close()
    return out


def host_piece(r, x1, y1, x2, y2, an, rl, rr, bp, exponents=False):
    s = e.Seqs(r["seq"][x1:], x2 - x1, r["events"][y1:y2])
    ref = e.banded(r["machine"], s, an, bp.threshold, bp.minDiagsBetweenTraceBack, bp.traceBackDiagonals,
                   bp.diagonalExpansion, (rl, rr), exponents)
    s.close()
    return ref


def same(got, ref):
    assert np.array_equal(got["totals_xay"], ref["totals_xay"])
    assert np.array_equal(got["totals"], ref["totals"])
    assert got["triples"].shape == ref["triples"].shape
    assert np.array_equal(got["triples"], ref["triples"])


def test_unbanded_toy_pairs_and_total(ctx):
    rd = reads(3, 1, 30, 45)[0]
    bp = band_params(0.01, 1000, 40, 20)
    got = run_batch(ctx, [(rd, 0, 0, 30, 45, [], 0, 0)], bp, flags=cp.FLAG_UNBANDED)[0]
    s = e.Seqs(rd["seq"], 30, rd["events"])
    ref = e.unbanded(rd["machine"], s, 0.01)
    s.close()
    D = 75
    assert np.array_equal(got["totals_xay"], [D]) and np.array_equal(got["totals"], [ref["total"]])
    want = np.concatenate([ref["per_diagonal"][d] for d in range(D, -1, -1)])  # the device walks the diagonals down
    assert len(want) > 0 and np.array_equal(got["triples"], want)


@pytest.mark.parametrize("threshold,ragged", [(0.01, (0, 0)), (0.01, (1, 1)), (0.0, (1, 0))])
def test_banded_batch_of_reads_with_their_own_models(ctx, threshold, ragged):
    rds = reads(7, 4, 120, 190)
    bp = band_params(threshold, 60, 20, 16)
    pieces = [(r, 0, 0, 120, 190, r["anchors"], ragged[0], ragged[1]) for r in rds]
    got = run_batch(ctx, pieces, bp)
    for g, pc in zip(got, pieces):
        ref = host_piece(*pc, bp)
        same(g, ref)
        assert len(ref["totals"]) > 2 and len(ref["triples"]) > 0
        if threshold == 0.0:  # every cell emits 15 pairs, coordinates repeating
            assert len(ref["triples"]) % 15 == 0 and len(ref["triples"]) > 15 * 190
            assert len({tuple(t) for t in ref["triples"][:, 1:]}) < len(ref["triples"])


def test_split_batch_reads_on_into_the_rest_of_the_read(ctx):
    """sub-alignments of getSplitPoints (a small maxMatrix): ragged inner ends, and the look-ahead of a piece's last
    k-mers reads the read's next characters, not the pad"""
    rds = reads(9, 2, 160, 240, anchor_every=12)
    bp = band_params(0.01, 60, 20, 16)
    pieces = []
    for r in rds:
        an = r["anchors"]
        an = an[(np.arange(len(an)) % 6) < 2]  # gaps wide enough to split at
        sp = cp.split_points(an, 160, 240, 40 * 40, 1, 1)
        assert len(sp) > 2
        j = 0
        for k, (x1, y1, x2, y2) in enumerate(sp):
            mine = []
            while j < len(an) and an[j, 0] + an[j, 1] < x2 + y2:
                mine.append((an[j, 0] - x1, an[j, 1] - y1))
                j += 1
            pieces.append((r, int(x1), int(y1), int(x2), int(y2), mine, 1, 1))
    got = run_batch(ctx, pieces, bp)
    for g, pc in zip(got, pieces):
        same(g, host_piece(*pc, bp))


def test_one_band_wider_than_248_kmers(ctx):
    rd = reads(13, 1, 320, 420)[0]
    bp = band_params(0.01, 1000, 40, 300)
    pc = (rd, 0, 0, 320, 420, rd["anchors"][::4], 0, 0)
    got = run_batch(ctx, [pc], bp)[0]
    same(got, host_piece(*pc, bp))


def test_zymo_template_through_get_aligned_pairs_using_anchors(golden_dir, zymo_read):
    """test_echelon_getAlignedPairsWithBanding (signalPairwiseTest.c:1388): the shipped read's template strand,
    getStateMachineEchelon + scaleModel, X padded, decoded with diagonalCalculationMultiPosteriorMatchProbs: every pair
    valid, and the whole list the host-driven DP's, tail first as getAlignedPairsUsingAnchors returns it"""
    L = e.lib()
    sm = L.getStateMachineEchelon(os.path.join(golden_dir, "template_median68pA.model").encode())
    L.emissions_signal_scaleModel(sm, *zymo_read["template_params"])
    ref_seq = zymo_read["reference"].encode()
    ev = np.ascontiguousarray(zymo_read["template_events"], dtype=np.float64).reshape(-1)
    lX, lY = len(ref_seq) - 5, ev.size // 3
    xbuf = C.create_string_buffer(ref_seq)
    p = L.pairwiseAlignmentBandingParameters_construct()
    p.contents.threshold = 0.15
    # anchors (lastz is not here): every 25th of the strongest quarter of the un-banded alignment's pairs
    full = L.getAlignedPairsWithoutBanding(sm, C.cast(xbuf, C.c_void_p), ev.ctypes.data_as(C.c_void_p), lX, lY, p,
                                           h.fn_ptr("sequence_getKmer2"), h.fn_ptr("sequence_getEvent"),
                                           h.fn_ptr("diagonalCalculationMultiPosteriorMatchProbs"), False, False)
    fa = h.list_to_array(full)
    L.stList_destruct(full)
    assert len(fa) > 100
    # (the echelon machine spreads a cell's mass over its six match states: its strongest pairs are far below 1)
    strong = fa[fa[:, 0] >= np.quantile(fa[:, 0], 0.75)]
    anchors = np.ascontiguousarray(strong[np.argsort(strong[:, 1], kind="stable")][::25, 1:3])
    anchors = anchors[np.concatenate([[True], (np.diff(anchors[:, 0]) > 0) & (np.diff(anchors[:, 1]) > 0)])]
    assert len(anchors) > 5
    sX = L.sequence_construct2(lX, C.cast(xbuf, C.c_void_p), h.fn_ptr("sequence_getKmer2"),
                               h.fn_ptr("sequence_sliceNucleotideSequence2"))
    L.sequence_padSequence(sX)
    sY = L.sequence_construct2(lY, ev.ctypes.data_as(C.c_void_p), h.fn_ptr("sequence_getEvent"),
                               h.fn_ptr("sequence_sliceEventSequence2"))
    lst = h.make_anchor_list(anchors)
    pairs = L.getAlignedPairsUsingAnchors(sm, sX, sY, lst, p, h.fn_ptr("diagonalCalculationMultiPosteriorMatchProbs"),
                                          False, False)
    got = h.list_to_array(pairs)
    assert len(got) > 200
    assert np.all(got[:, 0] >= 1500000) and np.all(got[:, 0] <= 10000000)
    assert np.all((got[:, 1] >= 0) & (got[:, 1] < lX)) and np.all((got[:, 2] >= 0) & (got[:, 2] < lY))
    m = e.Machine(np.ctypeslib.as_array(sm.contents.model.EMISSION_MATCH_PROBS, (20481,)).copy(),
                  np.ctypeslib.as_array(sm.contents.model.EMISSION_GAP_X_PROBS, (60,)).copy(),
                  np.ctypeslib.as_array(sm.contents.model.EMISSION_GAP_Y_PROBS, (20481,)).copy())
    s = e.Seqs(ref_seq, lX, ev)
    ref = e.banded(m, s, anchors, p.contents.threshold, p.contents.minDiagsBetweenTraceBack,
                   p.contents.traceBackDiagonals, p.contents.diagonalExpansion, (0, 0))
    assert np.array_equal(got, ref["triples"][::-1])
    s.close()
    m.close()
    for obj in (pairs, lst):
        L.stList_destruct(obj)
    L.sequence_sequenceDestroy(sX)
    L.sequence_sequenceDestroy(sY)
    L.pairwiseAlignmentBandingParameters_destruct(p)
    L.stateMachine_destruct(sm)


def test_unbanded_through_the_host_api_walks_the_diagonals_up(golden_dir):
    """getAlignedPairsWithoutBanding: the diagonals in ascending order, the pairs of one cell's states kept together"""
    rd = reads(17, 1, 40, 60)[0]
    L = e.lib()
    m = rd["machine"]
    xbuf = C.create_string_buffer(rd["seq"])
    ev = np.ascontiguousarray(rd["events"], dtype=np.float64).reshape(-1)
    p = L.pairwiseAlignmentBandingParameters_construct()
    pairs = L.getAlignedPairsWithoutBanding(m.sm, C.cast(xbuf, C.c_void_p), ev.ctypes.data_as(C.c_void_p), 40, 60, p,
                                            h.fn_ptr("sequence_getKmer2"), h.fn_ptr("sequence_getEvent"),
                                            h.fn_ptr("diagonalCalculationMultiPosteriorMatchProbs"), True, True)
    got = h.list_to_array(pairs)
    L.stList_destruct(pairs)
    s = e.Seqs(rd["seq"], 40, rd["events"])
    ref = e.unbanded(m, s, p.contents.threshold, (1, 1))
    s.close()
    assert np.array_equal(got, np.concatenate(ref["per_diagonal"]))
    L.pairwiseAlignmentBandingParameters_destruct(p)

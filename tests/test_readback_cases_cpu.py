"""The inputs of readback_cases.py are what they claim, on the oracle alone (no GPU): the filter of the threshold-0
list is the oracle's result at every threshold the builder emits; the tiny items' posteriors sit where the
construction puts them; the capacity batches' predicted counts fall on the side of the list's capacity they are meant
for; the long reads reach the ends of their long axis."""
import math

import numpy as np

import readback_cases as rc
from harness import band_params


def cell_q(ref, x, y):
    (i,) = np.flatnonzero((ref["triples"][:, 1] == x) & (ref["triples"][:, 2] == y))
    return ref["p"][i] * 10000000.0, int(ref["triples"][i, 0])


def test_filter_of_the_threshold_zero_list_is_the_oracle_at_every_threshold():
    shape = rc.strawman_shape()
    models = rc.sm3_models(shape["batch"])
    refs0 = rc.refs_at_zero("strawman-cpu", models, shape)
    cases = rc.threshold_cases(refs0[0])
    assert len(cases) == 18
    reads = rc.reads_of(shape["batch"])
    for j, (k, e, thr, keeps) in enumerate(cases):
        assert keeps == rc.KEEPS[j % 6] == (math.exp(e) >= thr), (j, e, thr)
        for i, it in enumerate(shape["batch"]["items"]):
            ref = rc.oracle_item(models[it["model"]], reads[i], rc.shape_bp(shape, thr), shape["ragged"])
            want = rc.expected_at(refs0[i], thr)
            for key in ("triples", "logp", "totals_xay", "totals"):
                assert np.array_equal(want[key], ref[key]), (j, i, key)
            assert want["cells"] == ref["cells"]
        cell = tuple(refs0[0]["triples"][k, 1:])
        kept = rc.expected_at(refs0[0], thr)["triples"]
        present = any(tuple(t[1:]) == cell for t in kept)
        assert present == keeps, (j, cell, thr)
    kept = [c[3] for c in cases]
    assert sum(kept) == 6 and len(kept) - sum(kept) == 12  # per cell: two thresholds keep it, four drop it
    # the slack threshold: the cell is below it, and still a candidate of the kernels' log(threshold) - 1e-3 cut
    for k, e, thr, keeps in cases[5::6]:
        assert not keeps and e >= math.log(thr) - 1e-3


def test_filter_of_the_echelon_threshold_zero_list_is_the_host_dp_at_every_threshold():
    """the echelon machine's exponents are read from the host DP's cells (echelon_dp.banded(exponents=True)): the list
    they filter is what diagonalCalculationMultiPosteriorMatchProbs itself returns at each threshold (item 0 at all
    18, item 1 at the three inside the kernels' slack)"""
    import test_echelon_gpu as te
    pieces, refs0 = rc.echelon_case()
    assert all(len(r["logp"]) == len(r["triples"]) > 15 * 190 and len(r["totals"]) > 2 for r in refs0)
    cases = rc.threshold_cases(refs0[0])
    assert len(cases) == 18
    for j, (k, e, thr, keeps) in enumerate(cases):
        assert keeps == rc.KEEPS[j % 6] == (math.exp(e) >= thr), (j, e, thr)
        for i in (0, 1) if j % 6 == 5 else (0,):
            te.same(rc.expected_at(refs0[i], thr), te.host_piece(*pieces[i], band_params(thr, **rc.ECHELON_BP)))
        # the state the threshold sits on emits its s pairs under that exponent: all of them kept, or none
        n0 = np.count_nonzero(refs0[0]["logp"] == e)
        assert 1 <= n0 <= 5 and np.count_nonzero(rc.expected_at(refs0[0], thr)["logp"] == e) == (n0 if keeps else 0), j
    for k, e, thr, keeps in cases[5::6]:
        assert not keeps and e >= math.log(thr) - 1e-3


def test_tiny_items_sit_next_to_multiples_of_1e_7_and_next_to_1():
    batch, refs, classes = rc.floor_batch()
    counts = {k: len(v) for k, v in classes.items()}
    assert classes["k"] == [1, 37, 4999999, 9990001] and classes["unreachable"] == [9999998], counts
    for j, k in enumerate(classes["k"]):
        for name, lo, hi, want in (("below-in", -1e-5, 0.0, k - 1), ("above-in", 0.0, 1e-5, k),
                                   ("below-out", -2e-4, -1e-5, k - 1), ("above-out", 1e-5, 2e-4, k)):
            q, integer = cell_q(refs[classes[name][j]], 1, 2)
            assert lo < q - k < hi and integer == want, (k, name, q - k, integer)
    for above, below in zip(classes["pad-above"], classes["pad-below"]):
        (qa, ia), (qb, ib) = cell_q(refs[above], 1, 2), cell_q(refs[below], 1, 2)
        assert ia == ib + 1 and qa >= ia > qb and qa - qb < 1e-5, (qa, qb)
    assert len(classes["pad-above"]) > 250, counts
    for name, test, integer in (("one-zero", lambda e: e == 0.0, 10000000), ("one-positive", lambda e: e > 0.0, 10000000),
                                ("one-window", lambda e: -1e-15 < e < 0.0, 9999999)):
        assert len(classes[name]) >= 1, counts
        for i in classes[name]:
            k = int(np.argmax(refs[i]["logp"]))
            assert test(refs[i]["logp"][k]) and refs[i]["triples"][k, 0] == integer, (name, refs[i])
    assert len(batch["items"]) == len(refs) > 600, counts


def test_capacity_batches_fall_on_the_side_meant():
    n, m = rc.counts_of(rc.LARGE, rc.LARGE_LIST_THRESHOLD)
    assert n > rc.THREADED_ABOVE and 1000 < m < rc.UNDECIDED_CAP // 2, (n, m)
    n0, m0 = rc.counts_of(rc.LARGE, 0.0)
    assert n0 > rc.THREADED_ABOVE and m0 > 2 * rc.UNDECIDED_CAP, (n0, m0)
    ns, ms = rc.counts_of(rc.SMALL_OVER, 0.0)
    assert ns < rc.THREADED_ABOVE and ms > rc.UNDECIDED_CAP + 1000, (ns, ms)
    big = rc.undecided(rc.cap_read("big")["ref0"], rc.LARGE_LIST_THRESHOLD)[0]
    assert 2 * big > n and sum(x is not None for x in rc.LARGE) >= 16 and rc.LARGE[0] is None and rc.LARGE[-1] is None
    for target in (rc.UNDECIDED_CAP, rc.UNDECIDED_CAP + 1):
        names = rc.exact_cap_names(target)
        assert names is not None and rc.counts_of(names, 0.0)[1] == target, target


def test_long_reads_reach_the_end_of_their_long_axis():
    for name, (axis, length, _, packed) in rc.LONG_CASES.items():
        batch, refs = rc.long_batch(name)
        it = batch["items"][0]
        assert (it["lX"] if axis == "x" else it["lY"]) == length
        assert (max(max(i["lX"], i["lY"]) for i in batch["items"]) < 65536) == packed
        col = refs[0]["triples"][:, 1 if axis == "x" else 2]
        assert col.max() == length - 1 and np.count_nonzero(col >= length - 10) >= 5, (name, col.max())
        assert all(len(r["triples"]) > 50 for r in refs)

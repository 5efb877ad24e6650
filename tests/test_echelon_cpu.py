"""The echelon signal machine behind the reference's interface, on the host (no GPU): the exported names and the
machine's members (getStateMachineEchelon, stateMachineEchelon_construct, impl/stateMachine.c:1602-1640, 1773), the
reference's test_echelon_cell / test_echelon_dpDiagonal properties (tests/signalPairwiseTest.c:365-505) restated on the
library's own host cell function, a plain-Python restatement of the recurrence (multipleKmerMatchProb's look-ahead
included) equal to the host DP, and the duration term against its formula."""
import ctypes as C
import math

import numpy as np
import pytest

import echelon_dp as e
import host_api as h
import synth

END_MATCH, END_X = 0.79015888282447311, 0.19652425498269727


def toy(seed, lX, lY, skip_lo=0.05, skip_hi=0.4):
    """a random k-mer sequence, events near its k-mers' levels, the synthetic pore model and 60 skip bins"""
    rng = np.random.default_rng(seed)
    match, _, gap_y = synth.synthetic_pore_model(seed)
    rd = synth.make_read(rng, match, lX, lY, anchor_every=10)
    skip = np.sort(rng.uniform(skip_lo, skip_hi, 30))[::-1]
    rd["events"][:, 2] = rng.uniform(0.001, 0.012, lY)
    return match, np.concatenate([skip, skip]), gap_y, rd


def test_echelon_names_are_exported_and_the_machine_is_the_references():
    L = e.lib()
    for name in ("getStateMachineEchelon", "stateMachineEchelon_construct", "emissions_signal_multipleKmerMatchProb"):
        assert hasattr(L, name)
    sm = L.getStateMachineEchelon(None)
    s = sm.contents
    assert s.model.type == e.ECHELON and s.model.stateNumber == 7 and s.model.matchState == 1
    assert s.DEFAULT_END_MATCH_PROB == END_MATCH and s.DEFAULT_END_FROM_X_PROB == END_X
    assert s.BACKGROUND_EVENT_PROB == -3.0
    fn = lambda name: C.cast(getattr(s.model, name), C.CFUNCTYPE(C.c_double, C.c_void_p, C.c_int64))
    assert [fn("startStateProb")(sm, i) for i in range(7)] == [-math.inf, 0.0] + [-math.inf] * 5
    assert [fn("raggedStartStateProb")(sm, i) for i in range(7)] == [-math.inf] * 6 + [0.0]
    for name in ("endStateProb", "raggedEndStateProb"):
        assert [fn(name)(sm, i) for i in range(7)] == [END_MATCH] * 6 + [END_X]
    assert s.getDurationProb == C.cast(L.emissions_signal_getDurationProb, C.c_void_p).value
    assert s.getMatchProbFcn == C.cast(L.emissions_signal_multipleKmerMatchProb, C.c_void_p).value
    L.stateMachine_destruct(sm)


@pytest.mark.parametrize("ragged", [(0, 0), (1, 1)])
def test_forward_and_backward_totals_agree_on_a_toy(ragged):
    """test_echelon_dpDiagonal (signalPairwiseTest.c:505-530): the full matrix forward and back on a 5-event toy.
    The two totals agree up to the error of logAdd's table (the reference's own toy lands within 1e-5; this one's
    paths sum differently, within 1e-3), and the total at the last diagonal agrees with the forward one"""
    match, skip, gap_y, rd = toy(11, 12, 5)
    m = e.Machine(match, skip, gap_y)
    s = e.Seqs(rd["seq"], 12, rd["events"])
    r = e.unbanded(m, s, 0.01, ragged)
    assert math.isfinite(r["forward_total"]) and abs(r["forward_total"] - r["backward_total"]) < 1e-3
    assert abs(r["total"] - r["forward_total"]) < 1e-3
    s.close()
    m.close()


@pytest.mark.parametrize("seed,lX,lY,ragged", [(1, 9, 11, False), (2, 14, 9, True), (3, 7, 16, False)])
def test_python_restatement_equals_the_host_dp(seed, lX, lY, ragged):
    """every forward cell of the full matrix, bit for bit, against the formulas restated in Python"""
    match, skip, gap_y, rd = toy(seed, lX, lY)
    m = e.Machine(match, skip, gap_y)
    s = e.Seqs(rd["seq"], lX, rd["events"])
    r = e.unbanded(m, s, 0.01, (ragged, False))
    py = e.PyEchelon(match, skip, gap_y, rd["seq"] + e.PAD, rd["events"]).forward(lX, lY, ragged)
    assert set(py) == set(r["forward_cells"])
    for k, v in py.items():
        assert v == r["forward_cells"][k], k
    s.close()
    m.close()


def test_lookahead_cuts_off_n_kmers_at_the_pad_and_at_lower_case():
    """multipleKmerMatchProb returns log zero exactly when the character 6n places after the getKmer2 pointer is not
    upper case; otherwise 0.0 logAdded with the n two-distribution terms, minus log(n)"""
    L = e.lib()
    match, skip, gap_y, rd = toy(5, 20, 10)
    py = e.PyEchelon(match, skip, gap_y, rd["seq"] + e.PAD, rd["events"])
    buf = C.create_string_buffer(rd["seq"] + e.PAD)
    mt = np.ascontiguousarray(match)
    ev = np.ascontiguousarray(rd["events"][3])
    host = lambda p, n: L.emissions_signal_multipleKmerMatchProb(mt.ctypes.data_as(C.POINTER(C.c_double)),
                                                                C.cast(C.addressof(buf) + p, C.c_void_p),
                                                                ev.ctypes.data_as(C.c_void_p), n)
    seen_cut = seen_full = 0
    for p in range(0, 20):
        for n in range(1, 6):
            want = py.multi(p, ev, n)
            assert host(p, n) == want
            if p + 6 * n >= 25:
                assert want == -math.inf  # the look-ahead reaches the pad
                seen_cut += 1
            else:
                assert math.isfinite(want)
                seen_full += 1
    assert seen_cut and seen_full
    # a lower-case base in the sequence itself cuts off exactly the n whose look-ahead lands on it
    low = bytearray(rd["seq"] + e.PAD)
    low[12] = ord(chr(low[12]).lower())
    buf2 = C.create_string_buffer(bytes(low))
    for n in range(1, 6):
        got = L.emissions_signal_multipleKmerMatchProb(mt.ctypes.data_as(C.POINTER(C.c_double)),
                                                       C.cast(C.addressof(buf2) + 0, C.c_void_p),
                                                       ev.ctypes.data_as(C.c_void_p), n)
        assert (got == -math.inf) == (n == 2 or 6 * n >= 25)  # (n = 5 reaches the pad)


def test_host_dp_with_a_cut_off_state_matches_the_restatement():
    """a toy short enough that the 6n look-ahead cuts match2..match5 off at the end of the sequence"""
    match, skip, gap_y, rd = toy(21, 6, 7)
    m = e.Machine(match, skip, gap_y)
    s = e.Seqs(rd["seq"], 6, rd["events"])
    r = e.unbanded(m, s, 0.01)
    py = e.PyEchelon(match, skip, gap_y, rd["seq"] + e.PAD, rd["events"]).forward(6, 7)
    assert all(py[k] == r["forward_cells"][k] for k in py)
    assert all(py[6, y][5] == -math.inf for y in range(1, 8))  # match5 at the end: the look-ahead hits the pad
    s.close()
    m.close()


def test_duration_term_is_the_poisson_formula():
    L = e.lib()
    for d in (0.0007, 0.00332005312085, 0.004, 0.0123):
        ev = np.array([60.0, 1.0, d])
        for n in range(6):
            got = L.emissions_signal_getDurationProb(ev.ctypes.data_as(C.c_void_p), n)
            lam = d / 0.00332005312085
            want = (n + 1) * 0.1397619423751586 + n * math.log(lam) - \
                [0.0, 0.0, 0.69314718056, 1.79175946923, 3.17805383035, 4.78749174278][n] - 2 * lam
            assert got == want == e.duration(ev, n)

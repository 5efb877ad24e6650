"""Inputs and expected values for the readback tests (test_readback_cases_cpu.py, test_readback_gpu.py,
readback_env_child.py): everything here runs on the CPU, against the oracle alone.

The readback is what follows the sweeps: each kernel keeps a cell whose exponent (F + B) - total reaches
log(threshold) - 1e-3 as a candidate, cpecan_k_pack_pairs gives every candidate a verdict from the device's exp()
(surely below the threshold, an integer posterior, or a close call), ensure_counts settles the close calls with the
host libm, cpecan_hip_batch_fetch_pairs expands what is left.  The inputs below sit where that stretch decides:

1. thresholds placed on a real candidate (threshold_cases / expected_at; echelon_case for the echelon machine),
2. posteriors next to a multiple of 1e-7 and next to 1, from 1 x 1 alignments (floor_items),
3. batches whose close calls fall on either side of the list's capacity (compose),
4. sequences of 65 535 and 65 536 elements (long_batch).

The expected result at a threshold is the oracle's list at threshold 0 filtered in order by exp(e) >= threshold with
math.exp -- the libm the oracle calls; test_readback_cases_cpu.py proves the filter against oracle runs."""
import math
import os

import numpy as np

import pyoracle as o
import synth
from harness import band_params, orc_params

HERE = os.path.dirname(os.path.abspath(__file__))
UNDECIDED_CAP = 65536      # CP_UNDECIDED_CAP of cpecan_batch.h
THREADED_ABOVE = 200000    # candidates past which ensure_counts deals the items to host threads

_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def host_exp(logp):
    """exp() of every exponent with the host libm (math.exp, not np.exp: the oracle's and ensure_counts' function)"""
    return np.array([math.exp(e) for e in logp], np.float64)


def with_p(ref):
    """an oracle result at threshold 0 with p = exp(logp) added (once)"""
    if "p" not in ref:
        ref["p"] = host_exp(ref["logp"])
    return ref


def expected_at(ref0, threshold):
    """the oracle's result at `threshold` from its result at threshold 0: the pairs filtered in order by
    exp(e) >= threshold, the integer posterior floor(min(p, 1) * 1e7); totals and cells do not depend on it"""
    p = with_p(ref0)["p"]
    keep = p >= threshold
    tri = ref0["triples"][keep].copy()
    tri[:, 0] = np.floor(np.minimum(p[keep], 1.0) * 10000000.0).astype(np.int64)
    out = dict(triples=tri, logp=ref0["logp"][keep], totals_xay=ref0["totals_xay"], totals=ref0["totals"])
    if "cells" in ref0:  # (the echelon machine's host DP counts none)
        out["cells"] = ref0["cells"]
    return out


# ------------------------------------------- 1. a threshold on a candidate -------------------------------------------

P_RANGES = ((0.1, 0.9), (1e-3, 1e-2), (1e-8, 1e-5))
KEEPS = (True, False, True, False, False, False)  # of the cell the six thresholds are built on


def six_thresholds(e):
    """the thresholds around a cell of exponent e: on it, one ulp above, inside the pack kernel's 1e-9 margin on either
    side, outside it, and half-way into the kernels' 1e-3 candidate slack"""
    t = math.exp(e)
    return (t, math.nextafter(t, math.inf), t * (1.0 - 0.9e-9), t * (1.0 + 0.9e-9), t * (1.0 + 1.1e-9),
            math.exp(e + 5e-4))


def pick_cells(ref0):
    """one cell of a threshold-0 result per range of P_RANGES (the middle one of those in range, by emission order):
    their indices"""
    p = with_p(ref0)["p"]
    out = []
    for lo, hi in P_RANGES:
        idx = np.flatnonzero((p >= lo) & (p <= hi))
        assert len(idx) > 0, "no cell with a posterior in [%g, %g]" % (lo, hi)
        out.append(int(idx[len(idx) // 2]))
    return out


def threshold_cases(ref0):
    """[(cell index, exponent, threshold, keeps the cell)] : 18 thresholds built on three cells of item 0"""
    out = []
    for k in pick_cells(ref0):
        e = float(ref0["logp"][k])
        for thr in six_thresholds(e):
            out.append((k, e, thr, math.exp(e) >= thr))
    return out


def oracle_item(model, read, bp, ragged):
    """one read (x, lX, y, anchors) on the oracle, pairs in emission order"""
    x, lX, y, an = read
    r = o.aligned_pairs_using_anchors(model, x, lX, y, an, orc_params(bp, split=1 << 60), ragged[0], ragged[1])
    r["triples"], r["logp"] = r["triples"][::-1], r["logp"][::-1]
    return r


def reads_of(batch):
    return [(batch["x_chars"][it["x_offset"]: it["x_offset"] + it["lX"] + 5], it["lX"],
             batch["events"][it["y_offset"]: it["y_offset"] + it["lY"]],
             batch["anchors"][it["anchor_offset"]: it["anchor_offset"] + it["n_anchors"]]) for it in batch["items"]]


def strawman_shape():
    """two strawMan reads of 150 k-mers and 310 events, several traceback windows"""
    return dict(batch=synth.make_batch(1234, 2, 150, 310, anchor_every=30), md=100, tb=20, e=40, ragged=(0, 0))


def family_shape(name, hdp=None):
    """a family of edge_reads (the w... ones: the widest band exactly that many k-mers)"""
    import edge_reads as er
    f = er.FAMILIES[name]
    batch = er.family_batch(name, hdp=hdp)
    return dict(batch=batch, md=f["md"], tb=f["tb"], e=batch["e"], ragged=f["ragged"])


def wide_shape(width, hdp=None):
    """two reads of 700 k-mers whose widest band is exactly `width` k-mers, as the wide builds' tests make them"""
    import edge_reads as er
    batch = er.edge_batch(1, 2, 700, 1050, "upper", every=1, e=40, width=width, hdp=hdp)
    return dict(batch=batch, md=150, tb=40, e=batch["e"], ragged=(width % 2, 1))


def shape_bp(shape, threshold):
    return band_params(threshold, shape["md"], shape["tb"], shape["e"])


def sm3_models(batch):
    return [o.Sm3Model(m, gy, gx) for (m, gx, gy) in batch["models"]]


def vanilla_models(batch):
    from test_vanilla_workgroup_gpu import vanilla_models as make
    return make(batch)


def sm4_models(batch):
    return [o.Sm4Model(m, gy) for (m, _, gy) in batch["models"]]


def load_nhdp():
    return cached("nhdp", lambda: o.load_nhdp(os.path.join(HERE, "golden", "testTemplate.nhdp")))


def first_pair_allocation(lX, lY):
    """the pairs a strawMan item has room for on a batch's first run (pairCapFactor 4 of cpecan_hip.hip's machine
    table): an item with more candidates makes ensure_counts run the batch again"""
    return 4 * (lX + lY) + 64


def refs_at_zero(key, models, shape):
    """the oracle's threshold-0 result of every item of a signal shape (models: one per batch model), once per key"""
    def run():
        bp = shape_bp(shape, 0.0)
        return [with_p(oracle_item(models[it["model"]], rd, bp, shape["ragged"]))
                for it, rd in zip(shape["batch"]["items"], reads_of(shape["batch"]))]
    return cached(("ref0", key), run)


ECHELON_BP = dict(min_diags=60, tb_diags=20, expansion=16)


def echelon_case():
    """the echelon machine's case: (pieces for test_echelon_gpu.run_batch, the host DP's threshold-0 result per piece
    with every pair's exponent): two reads of 120 k-mers and 190 events with models of their own, several traceback
    windows.  At threshold 0 every state 1..5 of every cell emits its s pairs, so an exponent stands s times in the
    list and a coordinate under several exponents; a threshold placed on one state's exponent keeps or drops that
    state's pairs, which the filter of expected_at follows pair by pair."""
    def build():
        import test_echelon_gpu as te
        pieces = [(r, 0, 0, 120, 190, r["anchors"], 0, 0) for r in te.reads(7, 2, 120, 190)]
        bp = band_params(0.0, **ECHELON_BP)
        return pieces, [with_p(te.host_piece(*pc, bp, exponents=True)) for pc in pieces]
    return cached("echelon", build)


# ------------------------------------- 2. multiples of 1e-7 and the neighbourhood of 1 -------------------------------------
# A 1 x 1 strawMan alignment has one path, and so has every 1 x n and 2 x 2 one (the alignment starts in a match, and
# the machine has no gap X <-> gap Y switch): its match posteriors are 1 or 0 whatever the events.  The smallest
# alignment with a choice is 2 k-mers x 3 events: match, match, extra event -- or match, extra event, match.  The cells
# (1, 1) and (1, 2) then have posteriors 1 - p and p, and p is a continuous, monotone function of how far the second
# or the third event's mean lies from the k-mers' level (both k-mers are the same homopolymer, so one level).

FLOOR_KS = (1, 37, 4999999, 9999998, 9990001)
# The oracle's (the reference's) logAdd returns the larger term where the other is more than about e^-7.7 of it, so q
# steps from 9 995 5xx straight to 1e7 here: k = 9 999 998 is out of these items' reach (floor_items lists it under
# 'unreachable'; test_readback_cases_cpu.py pins that), and 9 990 001 stands next to it as the highest that is not.
FLOOR_BP = dict(min_diags=100, tb_diags=20, expansion=40)
N_PAD_KS = 300
SPAN = 16.0  # standard deviations an event mean is moved by at most


class TwoByThree:
    """the oracle on 2 x 3 alignments of a homopolymer: q = 1e7 * posterior of the cell (k-mer 1, event 2) as a
    function of one parameter s in [-SPAN, SPAN]: s < 0 moves the second event's mean -s standard deviations off the
    k-mer's level (q rises towards 1e7), s > 0 the third event's (q falls towards 0)"""

    def __init__(self):
        self.tables = synth.synthetic_pore_model()
        match, gap_x, gap_y = self.tables
        self.model = o.Sm3Model(match, gap_y, gap_x)
        self.params = orc_params(band_params(0.0, **FLOOR_BP), split=1 << 60)
        self.no_anchors = np.zeros((0, 2), np.int64)
        self.level = match[1:].reshape(synth.NUM_KMERS, 5)

    def events(self, base, s):
        k = int(synth.kmer_indices(base.encode() * 6)[0])
        mu, sd = self.level[k, 0], self.level[k, 1]
        return np.array([[mu, 1.0, 0.01], [mu + max(-s, 0.0) * sd, 1.0, 0.01], [mu + max(s, 0.0) * sd, 1.0, 0.01]])

    def result(self, x, events):
        r = o.aligned_pairs_using_anchors(self.model, x, len(x) - 5, events, self.no_anchors, self.params, 0, 0)
        r["triples"], r["logp"] = r["triples"][::-1], r["logp"][::-1]
        return r

    def q(self, base, events):
        r = self.result(base * 7, events)
        (i,) = np.flatnonzero((r["triples"][:, 1] == 1) & (r["triples"][:, 2] == 2))
        return math.exp(r["logp"][i]) * 10000000.0


def bisect_s(one, base, target, tol):
    """events at which q is within tol of target (None where q steps over that window); tol None: bisect until the
    events stop changing and return (the last events with q >= target, the first with q < target)"""
    lo, hi = -SPAN, SPAN
    elo, ehi = one.events(base, lo), one.events(base, hi)
    assert one.q(base, elo) >= target > one.q(base, ehi), (base, target)
    while True:
        mid = 0.5 * (lo + hi)
        em = one.events(base, mid)
        if np.array_equal(em, elo) or np.array_equal(em, ehi) or not lo < mid < hi:
            return (elo, ehi) if tol is None else None
        qm = one.q(base, em)
        if tol is not None and abs(qm - target) <= tol:
            return em
        if qm >= target:
            lo, elo = mid, em
        else:
            hi, ehi = mid, em


def floor_items():
    """(items, classes): items = [(x characters, events[n][3])] of tiny alignments, classes = name -> item indices.
    For each k of FLOOR_KS: q just below and just above k inside the pack kernel's 1e-5 window, and 1e-4 either side,
    outside it.  Then, for N_PAD_KS other k, the two neighbouring inputs between which q crosses k: the closest these
    inputs come to a posterior that is a multiple of 1e-7 (where the device's exp() and the host's may fall on
    different sides).  Then the items next to 1 (near_one_items)."""
    def build():
        one = TwoByThree()
        rng = np.random.default_rng(20261018)
        items, classes = [], {}

        def add(name, x, events):
            classes.setdefault(name, []).append(len(items))
            items.append((x, events))
        for j, k in enumerate(FLOOR_KS):
            base = "ACGT"[j % 4]
            four = [("below-in", bisect_s(one, base, k - 5e-6, 2e-6)), ("above-in", bisect_s(one, base, k + 5e-6, 2e-6)),
                    ("below-out", bisect_s(one, base, k - 1e-4, 2e-5)), ("above-out", bisect_s(one, base, k + 1e-4, 2e-5))]
            if any(ev is None for _, ev in four):
                classes.setdefault("unreachable", []).append(k)
                continue
            classes.setdefault("k", []).append(k)
            for name, ev in four:
                add(name, base * 7, ev)
        pad_ks = np.unique(np.concatenate([rng.integers(2, 9990000, N_PAD_KS // 2),
                                           np.floor(10.0 ** rng.uniform(0.5, 6.99, N_PAD_KS // 2)).astype(np.int64)]))
        for k in pad_ks:
            base = "ACGT"[int(rng.integers(0, 4))]
            above, below = bisect_s(one, base, float(k), None)
            add("pad-above", base * 7, above)
            add("pad-below", base * 7, below)
        for name, x, events in near_one_items(one):
            add(name, x, events)
        return items, classes
    return cached("floor_items", build)


def near_one_items(one):
    """[(class, x, events)] of 1 x 2, 1 x 3 and 2 x 3 items with a cell whose exponent is exactly 0 ('one-zero'),
    positive ('one-positive') or in (-1e-15, 0) ('one-window': this needs a total below 8 in magnitude, whose ulp is
    below 1e-15), searched over random k-mers and events; at most 8 of each.  A class that no input reaches stays
    empty (the CPU test says which)."""
    rng = np.random.default_rng(7)
    out, seen = [], {"one-zero": 0, "one-positive": 0, "one-window": 0}
    for _ in range(4000):
        if min(seen.values()) >= 8:
            break
        lX, lY = ((1, 2), (1, 3), (2, 3))[int(rng.integers(0, 3))]
        x = "".join(rng.choice(list("ACGT"), lX + 5))
        ks = synth.kmer_indices(x.encode())
        ev = np.array([[one.level[ks[min(i, lX - 1)], 0] + rng.normal(0, 1.0), rng.uniform(0.4, 2.0), 0.01]
                       for i in range(lY)])
        e = float(one.result(x, ev)["logp"].max())
        name = "one-zero" if e == 0.0 else "one-positive" if e > 0.0 else "one-window" if e > -1e-15 else None
        if name is not None and seen[name] < 8:
            seen[name] += 1
            out.append((name, x, ev))
    return out


def floor_batch():
    """the items of floor_items() as one batch (one model): every distinct sequence's characters once, every item its
    own events; and the oracle's threshold-0 result per item"""
    def build():
        items, classes = floor_items()
        x_of, xs, its, yo = {}, "", [], 0
        for x, ev in items:
            if x not in x_of:
                x_of[x] = len(xs)
                xs += x
            its.append(dict(x_offset=x_of[x], lX=len(x) - 5, y_offset=yo, lY=len(ev), anchor_offset=0, n_anchors=0,
                            model=0))
            yo += len(ev)
        batch = dict(x_chars=xs.encode(), events=np.concatenate([ev for _, ev in items]),
                     anchors=np.zeros((0, 2), np.int64), items=its, models=[synth.synthetic_pore_model()])
        one = TwoByThree()
        refs = [with_p(one.result(x, ev)) for x, ev in items]
        return batch, refs, classes
    return cached("floor_batch", build)


# --------------------------------------------- 3. the close-call list's capacity ---------------------------------------------

CAP_BP = dict(min_diags=100, tb_diags=20, expansion=40)


def undecided(ref0, threshold):
    """(candidates, close calls) the readback sees for an oracle threshold-0 result at `threshold`, by the pack kernel's
    rules with the host's exp() (the device's differs by an ulp or two: the counts can differ where a posterior sits
    on a margin's own edge, which the tests that use them would show)"""
    e, p = ref0["logp"], with_p(ref0)["p"]
    cand = e >= (math.log(threshold) - 1e-3 if threshold > 0 else -math.inf)
    margin = 1e-9 * threshold + 1e-300
    below = p < threshold - margin
    above = (p > threshold + margin) | (threshold == 0.0)
    q = p * 10000000.0
    fl = np.floor(q)
    decided_mid = (p < 1.0 - 1e-9) & (q - fl > 1e-5) & (fl + 1.0 - q > 1e-5)
    decided_one = (p > 1.0 + 1e-9) | ((p >= 1.0 - 1e-9) & ((e >= 0.0) | (e <= -1e-15)))
    close = cand & ~below & ~(above & (decided_mid | decided_one))
    return int(cand.sum()), int(close.sum())


CAP_SHAPES = dict(big=(16000, 33000), small=(150, 310), s1=(40, 85), s2=(33, 70), s3=(26, 50), s4=(12, 27))


def cap_read(name):
    """one of the distinct reads the capacity batches are made of (built when first asked for), with a model of its own
    and its threshold-0 oracle result: 'big' (alone more than half of a large batch's candidates), 'small', and four
    short ones of other lengths whose close-call counts let copies sum to exactly the list's capacity"""
    def build():
        lX, lY = CAP_SHAPES[name]
        b = synth.make_batch(4321 + list(CAP_SHAPES).index(name), 1, lX, lY, anchor_every=30)
        bp = band_params(0.0, **CAP_BP)
        return dict(batch=b, ref0=with_p(oracle_item(sm3_models(b)[0], reads_of(b)[0], bp, (0, 0))))
    return cached(("cap_read", name), build)


def compose(names):
    """a batch of copies of cap_read()s in the order of `names` (None: an empty 0 x 0 item); copies share their read's
    characters, events, anchors and model through their offsets.  Returns (batch, names)."""
    used = [n for n in dict.fromkeys(names) if n is not None]
    xs, evs, ans, models, first = [], [], [], [], {}
    xo = yo = ao = 0
    for n in used:
        b = cap_read(n)["batch"]
        it = b["items"][0]
        first[n] = dict(x_offset=xo, lX=it["lX"], y_offset=yo, lY=it["lY"], anchor_offset=ao,
                        n_anchors=it["n_anchors"], model=len(models))
        xs.append(b["x_chars"])
        evs.append(b["events"])
        ans.append(b["anchors"])
        models.append(b["models"][0])
        xo, yo, ao = xo + len(b["x_chars"]), yo + len(b["events"]), ao + len(b["anchors"])
    empty = dict(x_offset=0, lX=0, y_offset=0, lY=0, anchor_offset=0, n_anchors=0, model=0)
    return dict(x_chars=b"".join(xs), events=np.concatenate(evs), anchors=np.concatenate(ans),
                items=[dict(first[n]) if n is not None else dict(empty) for n in names], models=models), list(names)


def counts_of(names, threshold):
    """(N, M) the readback should print for compose(names) at `threshold`"""
    per = {n: undecided(cap_read(n)["ref0"], threshold) for n in set(names) if n is not None}
    return (sum(per[n][0] for n in names if n is not None), sum(per[n][1] for n in names if n is not None))


LARGE = [None] + ["small"] * 32 + [None, "big"] + ["small"] * 32 + [None]
LARGE_LIST_THRESHOLD = 1e-13   # close calls: the candidates between 1e-13 and 1e-12, and the few on other margins
SMALL_OVER = ["small"] * 4


def exact_cap_names(target, threshold=0.0):
    """copies of the short reads (and 'small') whose close calls at `threshold` sum to exactly `target`, or None"""
    names = ["small", "s1", "s2", "s3", "s4"]
    m = [undecided(cap_read(n)["ref0"], threshold)[1] for n in names]
    # fewest items: dynamic programme over the sum (a coin problem)
    best = [None] * (target + 1)
    best[0] = (0, -1, -1)
    for s in range(1, target + 1):
        for j, mj in enumerate(m):
            if 0 < mj <= s and best[s - mj] is not None and (best[s] is None or best[s - mj][0] + 1 < best[s][0]):
                best[s] = (best[s - mj][0] + 1, j, s - mj)
    if best[target] is None:
        return None
    out, s = [], target
    while s > 0:
        _, j, s = best[s]
        out.append(names[j])
    return sorted(out, key=names.index)


# ------------------------------------------------ 4. 65 535 and 65 536 ------------------------------------------------

LONG_BP = dict(min_diags=1000, tb_diags=40, expansion=10)
LONG_THRESHOLD = 0.01


def long_read(long_axis, length):
    """one strawMan read whose `long_axis` ('x' or 'y') has `length` elements, anchors every 30 k-mers to its end, and
    its oracle result at LONG_THRESHOLD with the narrow band of LONG_BP"""
    def build():
        lX, lY = (length, int(length * 0.9)) if long_axis == "x" else (length // 2, length)
        match = synth.synthetic_pore_model()[0]
        for seed in range(9000, 9100):  # a read whose last k-mer emits exactly the last event: its last cell is a pair
            k = synth.make_read(np.random.default_rng(synth.SEED0 + seed * 1000), match, lX, lY, 30)["ev_kmer"]
            if k[-1] == lX - 1 and k[-2] != lX - 1:
                break
        b = synth.make_batch(seed, 1, lX, lY, anchor_every=30)
        bp = band_params(LONG_THRESHOLD, **LONG_BP)
        return dict(batch=b, ref=oracle_item(sm3_models(b)[0], reads_of(b)[0], bp, (0, 0)))
    return cached(("long", long_axis, length), build)


def short_read():
    def build():
        b = synth.make_batch(9100, 1, 100, 200, anchor_every=30)
        bp = band_params(LONG_THRESHOLD, **LONG_BP)
        return dict(batch=b, ref=oracle_item(sm3_models(b)[0], reads_of(b)[0], bp, (0, 0)))
    return cached("short", build)


def join(parts):
    """reads (each a one-item batch with its model) as one batch, and their oracle results"""
    xs, evs, ans, items, models = [], [], [], [], []
    xo = yo = ao = 0
    for p in parts:
        b = p["batch"]
        it = b["items"][0]
        items.append(dict(it, x_offset=xo, y_offset=yo, anchor_offset=ao, model=len(models)))
        xs.append(b["x_chars"])
        evs.append(b["events"])
        ans.append(b["anchors"])
        models.append(b["models"][0])
        xo, yo, ao = xo + len(b["x_chars"]), yo + len(b["events"]), ao + len(b["anchors"])
    return dict(x_chars=b"".join(xs), events=np.concatenate(evs), anchors=np.concatenate(ans), items=items,
                models=models), [p["ref"] for p in parts]


LONG_CASES = {
    # name: (the long read's axis, its length, the other item, whether the batch crosses PCIe packed)
    "y65535": ("y", 65535, "long", True),
    "y65536": ("y", 65536, "long", False),
    "x65535": ("x", 65535, "long", True),
    "x65536": ("x", 65536, "long", False),
    "y65536-and-short": ("y", 65536, "short", False),
}


def long_batch(name):
    axis, length, other, _ = LONG_CASES[name]
    second = short_read() if other == "short" else long_read(axis, 30000)
    return join([long_read(axis, length), second])

"""The echelon machine's CPU ground truth for the tests: the host library's own cell function (stateMachineEchelon's
cellCalculate in libcpecan_host.so) driven diagonal by diagonal through the exported DP internals, in the control flow
of the reference's getPosteriorProbsWithBanding (impl/pairwiseAligner.c:870-1006) and getAlignedPairsWithoutBanding
(:1512-1565); and a plain-Python restatement of the machine's forward recurrence for toy cases."""
import ctypes as C
import math

import numpy as np

import host_api as h
from cpecan_load import binding

cp = binding()
ECHELON = 5
PAD = b"n" * 30


class StateMachineEchelon(C.Structure):
    _fields_ = [("model", h.StateMachine), ("BACKGROUND_EVENT_PROB", C.c_double),
                ("DEFAULT_END_MATCH_PROB", C.c_double), ("DEFAULT_END_FROM_X_PROB", C.c_double),
                ("getKmerSkipProb", C.c_void_p), ("getDurationProb", C.c_void_p), ("getMatchProbFcn", C.c_void_p),
                ("getScaledMatchProbFcn", C.c_void_p)]


def lib():
    L = h.lib()
    if getattr(L, "_echelon_ready", False):
        return L
    vp = C.c_void_p
    SP = C.POINTER(StateMachineEchelon)
    L.getStateMachineEchelon.restype = SP
    L.getStateMachineEchelon.argtypes = [C.c_char_p]
    L.stateMachineEchelon_construct.restype = SP
    L.stateMachineEchelon_construct.argtypes = [C.c_int, C.c_int64] + [vp] * 6
    L.emissions_signal_multipleKmerMatchProb.restype = C.c_double
    L.emissions_signal_multipleKmerMatchProb.argtypes = [C.POINTER(C.c_double), vp, vp, C.c_int64]
    L.emissions_signal_getDurationProb.restype = C.c_double
    L.emissions_signal_getDurationProb.argtypes = [vp, C.c_int64]
    L.sequence_construct.restype = vp
    L.sequence_construct.argtypes = [C.c_int64, vp, vp]
    L.sequence_sequenceDestroy.argtypes = [vp]
    L.sequence_padSequence.argtypes = [vp]
    L.dpMatrix_construct.restype = vp
    L.dpMatrix_construct.argtypes = [C.c_int64, C.c_int64]
    L.dpMatrix_destruct.argtypes = [vp]
    L.dpMatrix_createDiagonal.restype = vp
    L.dpMatrix_createDiagonal.argtypes = [vp, h.Diagonal]
    L.dpMatrix_getDiagonal.restype = vp
    L.dpMatrix_getDiagonal.argtypes = [vp, C.c_int64]
    L.dpMatrix_deleteDiagonal.argtypes = [vp, C.c_int64]
    L.dpDiagonal_zeroValues.argtypes = [vp]
    L.dpDiagonal_initialiseValues.argtypes = [vp, vp, vp]
    L.dpDiagonal_getCell.restype = C.POINTER(C.c_double)
    L.dpDiagonal_getCell.argtypes = [vp, C.c_int64]
    L.dpDiagonal_dotProduct.restype = C.c_double
    L.dpDiagonal_dotProduct.argtypes = [vp, vp]
    for name in ("diagonalCalculationForward", "diagonalCalculationBackward"):
        getattr(L, name).argtypes = [vp, C.c_int64, vp, vp, vp]
    L.diagonalCalculationTotalProbability.restype = C.c_double
    L.diagonalCalculationTotalProbability.argtypes = [vp, C.c_int64, vp, vp, vp, vp]
    L.diagonalCalculationMultiPosteriorMatchProbs.argtypes = [vp, C.c_int64, vp, vp, vp, vp, C.c_double,
                                                              C.POINTER(h.Params), vp]
    L.cell_dotProduct2.restype = C.c_double
    L.cell_dotProduct2.argtypes = [C.POINTER(C.c_double), vp, vp]
    L._echelon_ready = True
    return L


class Machine:
    """an echelon StateMachine of the host library with the given tables (match and extra-event table in the
    reference's layout, 60 skip bins)"""

    def __init__(self, match, skip60, gap_y):
        L = lib()
        self.sm = L.getStateMachineEchelon(None)
        m = self.sm.contents.model
        C.memmove(m.EMISSION_MATCH_PROBS, np.ascontiguousarray(match, np.float64).ctypes.data, 8 * len(match))
        C.memmove(m.EMISSION_GAP_Y_PROBS, np.ascontiguousarray(gap_y, np.float64).ctypes.data, 8 * len(gap_y))
        C.memmove(m.EMISSION_GAP_X_PROBS, np.ascontiguousarray(skip60, np.float64).ctypes.data, 8 * 60)
        self.match, self.skip, self.gap_y = np.array(match, np.float64), np.array(skip60, np.float64), \
            np.array(gap_y, np.float64)

    def gpu_model(self):
        s = self.sm.contents
        return ((s.DEFAULT_END_MATCH_PROB, s.DEFAULT_END_FROM_X_PROB), self.match, self.skip, self.gap_y)

    def close(self):
        lib().stateMachine_destruct(self.sm)


class Seqs:
    """X (k-mers read through sequence_getKmer2, padded as sequence_padSequence does) and Y (events)"""

    def __init__(self, x_chars, lX, events, pad=True):
        L = lib()
        self.xbuf = C.create_string_buffer(bytes(x_chars) + (PAD if pad else b""))
        self.ev = np.ascontiguousarray(events, dtype=np.float64).reshape(-1).copy()
        self.lX, self.lY = lX, self.ev.size // 3
        self.sX = L.sequence_construct(lX, C.cast(self.xbuf, C.c_void_p), h.fn_ptr("sequence_getKmer2"))
        self.sY = L.sequence_construct(self.lY, self.ev.ctypes.data_as(C.c_void_p), h.fn_ptr("sequence_getEvent"))

    def close(self):
        lib().sequence_sequenceDestroy(self.sX)
        lib().sequence_sequenceDestroy(self.sY)


def _fn(sm, name):
    return getattr(sm.contents.model, name)


def _decode(L, sm, d, F, B, seqs, total, p):
    lst = L.stList_construct3(0, h.fn_ptr("stIntTuple_destruct"))
    args = (C.c_void_p * 1)(lst)
    L.diagonalCalculationMultiPosteriorMatchProbs(sm, d, F, B, seqs.sX, seqs.sY, total, p, C.cast(args, C.c_void_p))
    out = h.list_to_array(lst)
    L.stList_destruct(lst)
    return out


def _exponents(L, d, F, B, l, r, total, threshold):
    """the exponent (F[s] + B[s]) - total of every pair diagonalCalculationMultiPosteriorMatchProbs emits on diagonal
    d, in its order, read from the DP cells (the function keeps the integer posterior only)"""
    f, b = L.dpMatrix_getDiagonal(F, d), L.dpMatrix_getDiagonal(B, d)
    out = []
    for xmy in range(l, r + 1, 2):
        if (d + xmy) // 2 <= 0 or (d - xmy) // 2 <= 0:
            continue
        fc, bc = L.dpDiagonal_getCell(f, xmy), L.dpDiagonal_getCell(b, xmy)
        for s in range(1, 6):
            e = fc[s] + bc[s] - total
            if not math.exp(e) < threshold:
                out += [e] * s
    return out


def banded(machine, seqs, anchors, threshold, min_diags, tb_diags, expansion, ragged=(0, 0), exponents=False):
    """getPosteriorProbsWithBanding with diagonalCalculationMultiPosteriorMatchProbs: pairs in emission order and the
    (diagonal, totalProbability) refreshes in the order computed; with `exponents`, also every pair's exponent
    ('logp'), read from the DP cells on the host"""
    L, sm = lib(), machine.sm
    lX, lY = seqs.lX, seqs.lY
    Lb, Rb = cp.band_construct(np.asarray(anchors, np.int64).reshape(-1, 2), lX, lY, expansion)
    D = lX + lY
    diag = lambda d: h.Diagonal(d, int(Lb[d]), int(Rb[d]))
    F, B = L.dpMatrix_construct(D, 7), L.dpMatrix_construct(D, 7)
    p = L.pairwiseAlignmentBandingParameters_construct()
    p.contents.threshold = threshold
    L.dpDiagonal_initialiseValues(L.dpMatrix_createDiagonal(F, diag(0)), sm,
                                  _fn(sm, "raggedStartStateProb" if ragged[0] else "startStateProb"))
    pairs, totals, logp = [], [], []
    traced = 0
    for d in range(1, D + 1):
        L.dpDiagonal_zeroValues(L.dpMatrix_createDiagonal(F, diag(d)))
        L.diagonalCalculationForward(sm, d, F, seqs.sX, seqs.sY)
        at_end = d == D
        width = (int(Rb[d]) - int(Lb[d])) // 2 + 1
        if not (at_end or (d >= traced + min_diags and width <= expansion * 2 + 1)):
            continue
        L.dpDiagonal_initialiseValues(L.dpMatrix_createDiagonal(B, diag(d)), sm,
                                      _fn(sm, "raggedEndStateProb" if at_end and ragged[1] else "endStateProb"))
        if d > traced + 1:
            L.dpDiagonal_zeroValues(L.dpMatrix_createDiagonal(B, diag(d - 1)))
        frm = d - (0 if at_end else tb_diags + 1)
        total, calcs = -math.inf, 0
        d2 = d
        while d2 > traced:
            if d2 > traced + 2:
                L.dpDiagonal_zeroValues(L.dpMatrix_createDiagonal(B, diag(d2 - 2)))
            if d2 > traced + 1:
                L.diagonalCalculationBackward(sm, d2, B, seqs.sX, seqs.sY)
            if d2 <= frm:
                if calcs % 10 == 0:
                    total = L.diagonalCalculationTotalProbability(sm, d2, F, B, seqs.sX, seqs.sY)
                    totals.append((d2, total))
                calcs += 1
                pairs.append(_decode(L, sm, d2, F, B, seqs, total, p))
                if exponents:
                    logp += _exponents(L, d2, F, B, int(Lb[d2]), int(Rb[d2]), total, threshold)
                    assert len(logp) == sum(len(q) for q in pairs), d2
                if d2 < frm or at_end:
                    L.dpMatrix_deleteDiagonal(F, d2)
            if d2 + 1 <= D:
                L.dpMatrix_deleteDiagonal(B, d2 + 1)
            d2 -= 1
        traced = frm
        L.dpMatrix_deleteDiagonal(B, d2 + 1)
        L.dpMatrix_deleteDiagonal(F, d2)
        if at_end:
            break
    L.dpMatrix_destruct(F)
    L.dpMatrix_destruct(B)
    L.pairwiseAlignmentBandingParameters_destruct(p)
    tri = np.concatenate(pairs) if pairs else np.zeros((0, 3), np.int64)
    out = dict(triples=tri, totals_xay=np.array([t[0] for t in totals], np.int64),
               totals=np.array([t[1] for t in totals], np.float64))
    if exponents:
        out["logp"] = np.array(logp, np.float64)
    return out


def unbanded(machine, seqs, threshold, ragged=(0, 0)):
    """getAlignedPairsWithoutBanding with diagonalCalculationMultiPosteriorMatchProbs: the pairs per diagonal
    (ascending), the total taken at the last diagonal, and the forward / backward totals of the full matrix"""
    L, sm = lib(), machine.sm
    lX, lY = seqs.lX, seqs.lY
    Lb, Rb = cp.band_construct(np.zeros((0, 2), np.int64), lX, lY, 2)
    D = lX + lY
    F, B = L.dpMatrix_construct(D, 7), L.dpMatrix_construct(D, 7)
    for d in range(D + 1):
        L.dpDiagonal_zeroValues(L.dpMatrix_createDiagonal(B, h.Diagonal(d, int(Lb[d]), int(Rb[d]))))
        L.dpDiagonal_zeroValues(L.dpMatrix_createDiagonal(F, h.Diagonal(d, int(Lb[d]), int(Rb[d]))))
    L.dpDiagonal_initialiseValues(L.dpMatrix_getDiagonal(F, 0), sm,
                                  _fn(sm, "raggedStartStateProb" if ragged[0] else "startStateProb"))
    L.dpDiagonal_initialiseValues(L.dpMatrix_getDiagonal(B, D), sm,
                                  _fn(sm, "raggedEndStateProb" if ragged[1] else "endStateProb"))
    for d in range(D + 1):
        L.diagonalCalculationForward(sm, d, F, seqs.sX, seqs.sY)
    for d in range(D, 0, -1):
        L.diagonalCalculationBackward(sm, d, B, seqs.sX, seqs.sY)
    total = L.diagonalCalculationTotalProbability(sm, D, F, B, seqs.sX, seqs.sY)
    p = L.pairwiseAlignmentBandingParameters_construct()
    p.contents.threshold = threshold
    per = [_decode(L, sm, d, F, B, seqs, total, p) for d in range(D + 1)]
    # the two ends of the matrix: forward against the end vector, backward against the start vector
    end_fn = _fn(sm, "raggedEndStateProb" if ragged[1] else "endStateProb")
    start_fn = _fn(sm, "raggedStartStateProb" if ragged[0] else "startStateProb")
    fwd = L.cell_dotProduct2(L.dpDiagonal_getCell(L.dpMatrix_getDiagonal(F, D), lX - lY), sm, end_fn)
    bwd = L.cell_dotProduct2(L.dpDiagonal_getCell(L.dpMatrix_getDiagonal(B, 0), 0), sm, start_fn)
    fcells = {}
    for d in range(D + 1):
        dg = L.dpMatrix_getDiagonal(F, d)
        for xmy in range(int(Lb[d]), int(Rb[d]) + 1, 2):
            c = L.dpDiagonal_getCell(dg, xmy)
            fcells[((d + xmy) // 2, (d - xmy) // 2)] = [c[s] for s in range(7)]
    for d in range(D + 1):
        L.dpMatrix_deleteDiagonal(F, d)
        L.dpMatrix_deleteDiagonal(B, d)
    L.dpMatrix_destruct(F)
    L.dpMatrix_destruct(B)
    L.pairwiseAlignmentBandingParameters_destruct(p)
    return dict(per_diagonal=per, total=total, forward_total=fwd, backward_total=bwd, forward_cells=fcells)


# ---- a plain-Python restatement of the machine (the formulas of impl/stateMachine.c:345-370, 530-549, 1411-1455) ----
_F32 = lambda v: float(np.float32(v))
_LOOKUP = [(1.00, [_F32(c) for c in (-0.009350833524763, 0.130659527668286, 0.498799810682272, 0.693203116424741)]),
           (2.50, [_F32(c) for c in (-0.014532321752540, 0.139942324101744, 0.495635523139337, 0.692140569840976)]),
           (4.50, [_F32(c) for c in (-0.004605031767994, 0.063427417320019, 0.695956496475118, 0.514272634594009)]),
           (math.inf, [_F32(c) for c in (-0.000458661602210, 0.009695946122598, 0.930734667215156, 0.168037164329057)])]


def log_add(x, y):
    if x < y:
        x, y = y, x
    if y == -math.inf or x - y >= 7.5:
        return x
    d = x - y
    for lim, (a, b, c, e) in _LOOKUP:
        if d <= _F32(lim) if lim != math.inf else True:
            return ((a * d + b) * d + c) * d + e + y


def kmer_index(s):
    k = 0
    for ch in s[:6]:
        k = k * 4 + "ACGT".index(chr(ch))
    return k


def duration(event, n):
    lam = event[2] / 0.00332005312085
    lf = [0.0, 0.0, 0.69314718056, 1.79175946923, 3.17805383035, 4.78749174278][n]
    return (n + 1) * 0.1397619423751586 + n * math.log(lam) - lf - 2 * lam


class PyEchelon:
    """the echelon machine's forward recurrence over a full matrix, in the reference's order of transitions"""

    def __init__(self, match, skip60, gap_y, x_padded, events):
        self.match, self.skip, self.gap_y = match, skip60, gap_y
        self.x, self.ev = x_padded, np.asarray(events, np.float64).reshape(-1, 3)

    def two_dists(self, table, pos, e):  # emissions_signal_getEventMatchProbWithTwoDists of the k-mer at pos
        k = kmer_index(self.x[pos:pos + 6])
        mu, sd, nmu, lam = table[1 + 5 * k], table[2 + 5 * k], table[3 + 5 * k], table[5 + 5 * k]
        a = (e[0] - mu) / sd
        level = -0.91893853320467267 - math.log(sd) + (-0.5 * a * a)
        b = (e[1] - nmu) / nmu
        noise = (math.log(lam) - 1.8378770664093453 - 3 * math.log(e[1]) - lam * b * b / e[1]) / 2
        return level + noise

    def multi(self, p, e, n):
        if not chr(self.x[p + 6 * n]).isupper():
            return -math.inf
        s = 0.0
        for i in range(n):
            s = log_add(s, self.two_dists(self.match, p + i + 1, e))
        return s - math.log(n)

    def skips(self, p):
        mu = lambda q: self.match[1 + 5 * kmer_index(self.x[q:q + 6])]
        b = min(int(abs(mu(p + 1) - mu(p)) / 0.5), 29)
        return self.skip[b], self.skip[b + 30]

    def forward(self, lX, lY, ragged_left=False):
        NEG = -math.inf
        F = {}
        for x in range(lX + 1):
            for y in range(lY + 1):
                if x == 0 and y == 0:
                    F[0, 0] = [NEG] * 6 + [0.0] if ragged_left else [NEG, 0.0] + [NEG] * 5
                    continue
                p = max(x - 2, 0)
                e = self.ev[y - 1] if y > 0 else None
                beta, alpha = self.skips(p)
                la_mx, la_mh, la_xx, la_xh = math.log(beta), math.log(1 - beta), math.log(alpha), math.log(1 - alpha)
                o = [NEG] * 7
                if x > 0:  # lower
                    lo = F[x - 1, y]
                    for n in range(1, 6):
                        o[6] = log_add(o[6], lo[n] + (0 + la_mx))
                    o[6] = log_add(o[6], lo[6] + (0 + la_xx))
                if x > 0 and y > 0:  # middle
                    mi = F[x - 1, y - 1]
                    eps = {n: self.multi(p, e, n) for n in range(1, 6)}
                    for n in range(1, 6):
                        for frm in range(6):
                            o[n] = log_add(o[n], mi[frm] + (eps[n] + (la_mh + duration(e, n))))
                    for n in range(1, 6):
                        o[n] = log_add(o[n], mi[6] + (eps[n] + (la_xh + duration(e, n))))
                if y > 0:  # upper
                    up = F[x, y - 1]
                    ey = self.two_dists(self.gap_y, p + 1, e)
                    for n in range(1, 6):
                        o[0] = log_add(o[0], up[n] + (ey + (la_mh + duration(e, 0))))
                F[x, y] = o
        return F

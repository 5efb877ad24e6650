"""ctypes view of the stream in expectation mode (cpecan_stream_open_expectations, include/cpecan_api.h), beside
stream_api.py: the struct a stream adds to, per machine, as a vector; the call on one read alone; one run of a stream."""
import ctypes as C

import numpy as np

import host_api as h
import stream_api as sa

DONE_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int64, C.c_bool)
ESTEP_EXPORTS = ["cpecan_stream_open_expectations", "cpecan_stream_expectations_class"]
MACHINE_OF = {"strawman": 0, "dna5": 1, "vanilla": 2, "hdp": 3, "sm4": 4, "echelon": 5}  # CPECAN_MACHINE_*
HDP_THRESHOLD = 0.05
_READY = False


def lib():
    global _READY
    L = sa.lib()
    if not _READY:
        vp = C.c_void_p
        L.cpecan_stream_open_expectations.restype = vp
        L.cpecan_stream_open_expectations.argtypes = [C.POINTER(h.Params), C.c_bool, C.c_bool,
                                                      C.POINTER(sa.StreamOptions), vp, DONE_FN, sa.CHUNK_FN, vp]
        L.cpecan_stream_expectations_class.restype = C.c_int32
        L.cpecan_stream_expectations_class.argtypes = [C.c_int32] * 3 + [C.POINTER(C.c_int32)] * 3
        _READY = True
    return L


def expectations_class(machine, width, step_by_one=True):
    """(kernel, wave, rows) of an E-step read of that widest band, as the stream classes it"""
    k, w, r = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    rc = lib().cpecan_stream_expectations_class(machine, width, int(step_by_one), C.byref(k), C.byref(w), C.byref(r))
    assert rc == 0, rc
    return k.value, w.value, r.value


class Target:
    """the struct the expectations of `kind` go to: what the single-read call takes, and what a stream is opened with"""

    def __init__(self, kind, pseudocount=0.0):
        L = lib()
        self.kind = kind
        if kind == "strawman":
            self.obj = h.Expectations()
            self.ptr = C.cast(C.pointer(self.obj), C.c_void_p)
        elif kind == "vanilla":
            self.obj = h.VanillaExpectations()
            self.ptr = C.cast(C.pointer(self.obj), C.c_void_p)
        elif kind == "hdp":
            self.obj = L.cpecan_hdpExpectations_construct(pseudocount, HDP_THRESHOLD)
            self.ptr = C.cast(self.obj, C.c_void_p)
        elif kind == "dna5":
            self.obj = h.new_hmm_discrete(pseudocount)
            self.ptr = C.cast(self.obj, C.c_void_p)
        else:
            raise ValueError(kind)

    def alone(self, sm, rd, p):
        """the E-step of one read added to this struct by the single-read call of its machine"""
        L = lib()
        if self.kind == "strawman":
            L.cpecan_getSignalExpectationsUsingAnchors(sm, C.byref(self.obj), rd.sX, rd.sY, rd.lst, p, True, True)
        elif self.kind == "vanilla":
            L.cpecan_getVanillaExpectationsUsingAnchors(sm, C.byref(self.obj), rd.sX, rd.sY, rd.lst, p, True, True)
        elif self.kind == "hdp":
            L.cpecan_getHdpExpectationsUsingAnchors(sm, self.obj, rd.sX, rd.sY, rd.lst, p, True, True)
        else:
            L.getExpectationsUsingAnchors(sm, self.ptr, rd.sX, rd.sY, rd.lst, p,
                                          h.fn_ptr("diagonalCalculation_Expectations"), True, True)
        return self

    def vector(self):
        """[the sums | likelihood]"""
        if self.kind == "strawman":
            o = self.obj
            return np.concatenate([np.array(o.transitions), np.array(o.individualKmerGapProbs), [o.likelihood]])
        if self.kind == "vanilla":
            return np.concatenate([np.array(self.obj.kmerSkipBins), [self.obj.likelihood]])
        if self.kind == "hdp":
            o = self.obj.contents
            return np.concatenate([np.array(o.transitions), [o.likelihood]])
        o = self.obj.contents
        return np.concatenate([np.array(o.transitions[:25]), np.array(o.emissions[:80]), [o.baseHmm.likelihood]])

    def assignments(self):
        """HDP: [(tag, x, y, k-mer, event mean)] in the struct's order"""
        o = self.obj.contents
        out = []
        for i in range(o.numberOfAssignments):
            kmer = C.string_at(C.addressof(o.kmerAssignments.contents) + 7 * i)
            out.append((o.assignmentXY[3 * i + 2], o.assignmentXY[3 * i], o.assignmentXY[3 * i + 1], kmer,
                        o.eventAssignments[i]))
        return out


def assert_vectors_match(got, want, what=""):
    """the suite's bars for E-step sums taken in another order: sums to rtol 1e-9 / atol 1e-12, likelihood to rtol 1e-12"""
    assert got.shape == want.shape and np.all(np.isfinite(want)), what
    bad = np.flatnonzero(~np.isclose(got[:-1], want[:-1], rtol=1e-9, atol=1e-12))
    assert bad.size == 0, (what, bad[:10], got[bad[:10]], want[bad[:10]])
    assert np.isclose(got[-1], want[-1], rtol=1e-12, atol=0) and want[-1] < 0, (what, got[-1], want[-1])


def run_stream(sms, reads, p, target, tags=None, **options):
    """the reads through one expectation stream into `target`.  Returns dict(done=[(tag, refused) in order of the calls],
    chunks=[dict per chunk], n_chunks, n_refused, peak)."""
    L = lib()
    done, chunks = [], []

    def on_done(_arg, tag, refused):
        done.append((tag, bool(refused)))

    def on_chunk(_arg, c):
        chunks.append({name: getattr(c.contents, name) for name, _ in sa.StreamChunk._fields_})

    cb_d, cb_c = DONE_FN(on_done), sa.CHUNK_FN(on_chunk)
    o = sa.StreamOptions(**options)
    s = L.cpecan_stream_open_expectations(p, True, True, C.byref(o), target.ptr, cb_d, cb_c, None)
    for i, rd in enumerate(reads):
        sm = sms[i] if isinstance(sms, (list, tuple)) else sms
        L.cpecan_stream_submit(s, i if tags is None else tags[i], sm, rd.sX, rd.sY, rd.lst)
    n_chunks, n_refused, peak = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    L.cpecan_stream_close(s, C.byref(n_chunks), C.byref(n_refused), C.byref(peak))
    return dict(done=done, chunks=chunks, n_chunks=n_chunks.value, n_refused=n_refused.value, peak=peak.value)

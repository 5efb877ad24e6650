"""ctypes view of the stream of libcpecan_host.so (include/cpecan_api.h) and the reads its tests share: a read of any
of the six machines as a C caller would hold it, the per-read reference call, anchors with one jump, and the batches of
the memory-limit test.  Beside host_api.py, which it builds on."""
import ctypes as C
import os

import numpy as np

import host_api as h
import synth
from cpecan_load import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")
KERNEL_GENERAL, KERNEL_SYSTOLIC = 1, 2


class StreamOptions(C.Structure):
    _fields_ = [("deviceBytes", C.c_int64), ("slots", C.c_int32), ("producerThreads", C.c_int32),
                ("maxReadsPerChunk", C.c_int64), ("oneClass", C.c_int32)]


class StreamChunk(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("index", "nReads", "nItems", "deviceBytes")] + [
        (n, C.c_int32) for n in ("kernel", "wave", "rows", "maxWidth", "halvings")]


RESULT_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int64, C.c_void_p)
CHUNK_FN = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(StreamChunk))
STREAM_EXPORTS = ["cpecan_stream_open", "cpecan_stream_submit", "cpecan_stream_flush", "cpecan_stream_close",
                  "cpecan_stream_plan_chunks"]
_READY = False


def lib():
    global _READY
    L = h.lib()
    if not _READY:
        vp = C.c_void_p
        L.cpecan_stream_open.restype = vp
        L.cpecan_stream_open.argtypes = [C.POINTER(h.Params), C.c_bool, C.c_bool, C.POINTER(StreamOptions), RESULT_FN,
                                         CHUNK_FN, vp]
        L.cpecan_stream_submit.argtypes = [vp, C.c_int64, vp, vp, vp, vp]
        L.cpecan_stream_flush.argtypes = [vp]
        L.cpecan_stream_close.argtypes = [vp] + [C.POINTER(C.c_int64)] * 3
        L.cpecan_stream_plan_chunks.restype = C.c_int64
        L.cpecan_stream_plan_chunks.argtypes = [C.c_int64, vp, vp, C.c_int64, C.c_int64, C.c_int32, vp, vp]
        for name in ("getStateMachineEchelon",):
            getattr(L, name).restype = vp
            getattr(L, name).argtypes = [C.c_char_p]
        _READY = True
    return L


def plan_chunks(classes, cells, max_reads, cell_budget, one_class=False):
    """the chunking rule through its test hook: (chunk of every read, its place inside that chunk, number of chunks)"""
    cl = np.ascontiguousarray(classes, dtype=np.int32)
    ce = np.ascontiguousarray(cells, dtype=np.int64)
    out, rank = np.full(cl.size, -1, np.int64), np.full(cl.size, -1, np.int64)
    n = lib().cpecan_stream_plan_chunks(cl.size, cl.ctypes.data, ce.ctypes.data, max_reads, cell_budget, int(one_class),
                                        out.ctypes.data, rank.ctypes.data)
    return out, rank, n


class SeqRead:
    """one read as a C caller holds it: X over characters (k-mer getter `get_x`, or bases), Y over events or bases"""

    def __init__(self, x_chars, y, get_x="sequence_getKmer", anchors=()):
        L = lib()
        xb = x_chars if isinstance(x_chars, bytes) else x_chars.encode()
        self.xbuf = C.create_string_buffer(xb)
        dna = get_x == "sequence_getBase"
        if dna:
            self.ybuf = C.create_string_buffer(y if isinstance(y, bytes) else y.encode())
            self.lX, self.lY = len(xb), len(self.ybuf.value)
            self.sX = L.sequence_construct2(self.lX, C.cast(self.xbuf, C.c_void_p), h.fn_ptr(get_x),
                                            h.fn_ptr("sequence_sliceNucleotideSequence"))
            self.sY = L.sequence_construct2(self.lY, C.cast(self.ybuf, C.c_void_p), h.fn_ptr(get_x),
                                            h.fn_ptr("sequence_sliceNucleotideSequence"))
        else:
            self.ev = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
            self.lX, self.lY = len(xb) - 5, self.ev.size // 3
            self.sX = L.sequence_construct2(self.lX, C.cast(self.xbuf, C.c_void_p), h.fn_ptr(get_x),
                                            h.fn_ptr("sequence_sliceNucleotideSequence2"))
            self.sY = L.sequence_construct2(self.lY, self.ev.ctypes.data_as(C.c_void_p), h.fn_ptr("sequence_getEvent"),
                                            h.fn_ptr("sequence_sliceEventSequence2"))
        self.anchors = np.asarray(anchors, np.int64).reshape(-1, 2)
        self.lst = h.make_anchor_list(self.anchors)


def params(expansion=20, min_diags=120):
    p = lib().pairwiseAlignmentBandingParameters_construct()
    p.contents.diagonalExpansion = expansion
    p.contents.minDiagsBetweenTraceBack = min_diags
    return p


def alone(sm, rd, p, echelon=False):
    """getAlignedPairsUsingAnchors on the read alone: the triples, in its order"""
    L = lib()
    fn = "diagonalCalculationMultiPosteriorMatchProbs" if echelon else "diagonalCalculationPosteriorMatchProbs"
    lst = L.getAlignedPairsUsingAnchors(sm, rd.sX, rd.sY, rd.lst, p, h.fn_ptr(fn), True, True)
    out = h.list_to_array(lst)
    L.stList_destruct(lst)
    return out


def run_stream(sms, reads, p, tags=None, **options):
    """the reads through one stream; sms: one machine for all, or one per read.
    Returns dict(results={tag: triples or None}, delivered=[tags in order of delivery], chunks=[dict per chunk],
    n_chunks, n_refused, peak)."""
    L = lib()
    results, delivered, chunks = {}, [], []

    def on_result(_arg, tag, lst):
        delivered.append(tag)
        if lst:
            results[tag] = h.list_to_array(lst)
            L.stList_destruct(lst)
        else:
            results[tag] = None

    def on_chunk(_arg, c):
        chunks.append({name: getattr(c.contents, name) for name, _ in StreamChunk._fields_})

    cb_r, cb_c = RESULT_FN(on_result), CHUNK_FN(on_chunk)
    o = StreamOptions(**options)
    s = L.cpecan_stream_open(p, True, True, C.byref(o), cb_r, cb_c, None)
    for i, rd in enumerate(reads):
        sm = sms[i] if isinstance(sms, (list, tuple)) else sms
        L.cpecan_stream_submit(s, i if tags is None else tags[i], sm, rd.sX, rd.sY, rd.lst)
    n_chunks, n_refused, peak = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    L.cpecan_stream_close(s, C.byref(n_chunks), C.byref(n_refused), C.byref(peak))
    return dict(results=results, delivered=delivered, chunks=chunks, n_chunks=n_chunks.value,
                n_refused=n_refused.value, peak=peak.value)


def with_jump(anchors, jump, after=2):
    """the anchors with those dropped that follow anchor `after` within `jump` k-mers: one anchor-free stretch that is
    `jump` k-mers longer than the others, and the band that much wider there"""
    a = np.asarray(anchors, np.int64).reshape(-1, 2)
    if jump <= 0:
        return a
    x0 = a[after, 0]
    keep = (np.arange(len(a)) <= after) | (a[:, 0] > x0 + jump)
    return a[keep]


# ---- machines over the synthetic pore model (tests/synth.py), built the way a C caller builds them ----
def _install_synthetic_tables(sm, model):
    m, _, gy = model
    s = C.cast(sm, C.POINTER(h.StateMachine)).contents
    C.memmove(s.EMISSION_MATCH_PROBS, m.ctypes.data, m.nbytes)
    C.memmove(s.EMISSION_GAP_Y_PROBS, gy.ctypes.data, gy.nbytes)


def machine(kind):
    """(StateMachine *, k-mer getter of X) of `kind`: strawman, vanilla, sm4, echelon -- over the synthetic pore model
    (the skip bins of the vanilla and echelon machines are the shipped template model's)"""
    L = lib()
    golden = os.path.join(GOLDEN, "template_median68pA.model").encode()
    if kind == "strawman":
        sm, get_x = C.cast(L.getStrawManStateMachine3(None), C.c_void_p), "sequence_getKmer"
    elif kind == "vanilla":
        sm, get_x = L.getSignalStateMachine3Vanilla(golden), "sequence_getKmer2"
    elif kind == "sm4":
        sm, get_x = L.getStateMachine4(golden), "sequence_getKmer"
    elif kind == "echelon":
        sm, get_x = L.getStateMachineEchelon(golden), "sequence_getKmer2"
    else:
        raise ValueError(kind)
    _install_synthetic_tables(sm, synth.synthetic_pore_model())
    return sm, get_x


def synthetic_reads(config_id, lengths, get_x="sequence_getKmer", anchor_every=30, jumps=None):
    """reads of synth.make_read over the unscaled synthetic model, lengths = [(lX, lY), ...]; jumps[i]: with_jump"""
    match = synth.synthetic_pore_model()[0]
    out = []
    for r, (lx, ly) in enumerate(lengths):
        rng = np.random.default_rng(synth.SEED0 + config_id * 1000 + r)
        rd = synth.make_read(rng, match, lx, ly, anchor_every)
        # (the machines here carry the unscaled model: the events are taken back through the read's own scaling)
        scale, shift = rd["scale_params"][:2]
        ev = rd["events"].copy()
        ev[:, 0] = (ev[:, 0] - shift) / scale
        out.append(SeqRead(rd["seq"], ev, get_x, with_jump(rd["anchors"], jumps[r] if jumps else 0)))
    return out


def hdp_machine_and_reads(seed, lengths, every=40):
    """(machine, NanoporeHDP, reads) on the shipped serialized HDP: every k-mer emits one or two events at the mode of
    its distribution"""
    import pyoracle as o
    L = lib()
    path = os.path.join(GOLDEN, "testTemplate.nhdp")
    nh = L.deserialize_nhdp(path.encode())
    sm = L.getHdpStateMachine3(nh)
    parsed = o.load_nhdp(path)
    om = o.HdpModel(parsed)
    rng = np.random.default_rng(seed)
    reads = []
    for lX in lengths:
        x = "".join(rng.choice(list("ACGT"), lX + 5))
        ev, anchors = [], []
        for k in range(lX):
            row = parsed["kmer_row"][om.kmer_id(x[k:k + 6])]
            mode = parsed["grid"][int(np.argmax(parsed["y"][row]))]
            if k % every == every // 2:
                anchors.append((k, len(ev)))
            for _ in range(1 if rng.random() < 0.6 else 2):
                ev.append((mode + rng.normal(0, 1.0), 1.0, 0.01))
        reads.append(SeqRead(x, np.array(ev), "sequence_getKmer3", anchors))
    return sm, nh, reads


def dna_machine_and_reads(seed, lengths):
    L = lib()
    sm = L.stateMachine5_construct(0, 4, h.fn_ptr("emissions_symbol_setEmissionsToDefaults"),
                                   h.fn_ptr("emissions_symbol_getGapProb"), h.fn_ptr("emissions_symbol_getGapProb"),
                                   h.fn_ptr("emissions_symbol_getMatchProb"), h.fn_ptr("cell_updateExpectations"))
    rng = np.random.default_rng(seed)
    reads = []
    for n in lengths:
        x = "".join(rng.choice(list("ACGT"), n))
        y = "".join(ch if rng.random() > 0.15 else rng.choice(list("ACGT")) for ch in x)
        reads.append(SeqRead(x, y, "sequence_getBase", [(k, k) for k in range(20, n - 10, 40)]))
    return sm, reads


# ---- the batches of the memory-limit test, and the same reads for the stream's budget test ----
LIMIT_READS, LIMIT_LX, LIMIT_LY, LIMIT_EVERY, LIMIT_CONFIG = 16, 200, 420, 40, 77
_LIMIT = {}


def limit_case(cp, ctx):
    """The 16 reads, the first 4 of them, and the limit between: dict(batch4, batch16, bp, b4, b16, need4, L).
    b4, b16: Batch.device_bytes() after creation on the unlimited `ctx`; need4: what that context held at the most over
    the 4-read batch's whole life (model table, run, readback) -- b4 is the batch at creation alone, and a limit that
    the batch could not run under would test nothing; L: need4 plus the room the allocator's block reuse may take, which
    is per block: a quarter, and 4 KB for each of the batch's blocks -- a batch holds fewer than 64 buffers
    (cpecan_batch.h), tables and pack buffers included.  Worked out once per process."""
    if _LIMIT:
        return _LIMIT
    from harness import band_params, make_items
    bp = band_params(0.01, 120, 40, 20)
    mk = lambda n: synth.make_batch(LIMIT_CONFIG, n, LIMIT_LX, LIMIT_LY, anchor_every=LIMIT_EVERY, distinct_models=False)
    b4s, b16s = mk(4), mk(16)
    sizes = {}
    for name, batch in (("b16", b16s), ("b4", b4s)):
        ctx.models_clear()
        ctx.models_create([(cp.NANOPORE_TRANSITIONS,) + tuple(batch["models"][0])])
        ctx.memory(reset_peak=True)
        b = cp.Batch(ctx, make_items(batch, (1, 1)), batch["x_chars"], batch["events"], batch["anchors"], bp,
                     cp.MODE_POSTERIOR, cp.KERNEL_AUTO, cp.FLAG_SMALL_FOOTPRINT)
        sizes[name] = b.device_bytes()
        if name == "b4":
            b.run()
            b.sync()
            b.counts()
            sizes["need4"] = ctx.memory()["peak"]
        b.close()
    _LIMIT.update(batch4=b4s, batch16=b16s, bp=bp, L=sizes["need4"] + sizes["need4"] // 4 + 64 * 4096, **sizes)
    return _LIMIT

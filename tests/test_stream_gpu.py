"""The stream of libcpecan_host.so (cpecan_stream_*, include/cpecan_api.h): every read's list equals what
getAlignedPairsUsingAnchors gives for that read alone -- same length, same triples, same order -- whatever the chunks;
reads are grouped by the kernel each would run on alone; the device-memory budget holds, and a read that cannot fit is
refused without harm to the others."""
import ctypes as C

import numpy as np
import pytest

import host_api as h
import stream_api as sa
from harness import cp

pytestmark = pytest.mark.gpu

# 12 reads of mixed lengths, 300-800 events
MIXED = [(150, 300), (400, 800), (220, 450), (310, 640), (180, 380), (260, 500), (390, 790), (160, 330), (350, 700),
         (200, 410), (280, 560), (240, 470)]


def _identical(out, refs, n_reads):
    assert sorted(out["delivered"]) == list(range(n_reads))  # every tag exactly once
    for i in range(n_reads):
        got = out["results"][i]
        assert got is not None and got.shape == refs[i].shape and np.array_equal(got, refs[i]), i
        assert len(got) > 0
    _order_within_chunks(out, n_reads)


def _order_within_chunks(out, n_reads):
    """Chunks finish in the order in which their runs were queued, which is the order onChunk reported them in, and a
    chunk delivers its reads in the order of their submission: `delivered` is the chunks' reads one chunk after the
    other, ascending inside each (tags here are submission indices).  For streams that refused no read."""
    pos = 0
    for c in sorted(out["chunks"], key=lambda c: c["index"]):
        piece = out["delivered"][pos:pos + c["nReads"]]
        assert len(piece) == c["nReads"] and piece == sorted(piece), (c, piece)
        pos += c["nReads"]
    assert pos == n_reads


def _signal_case(kind, lengths, config_id, jumps=None):
    sm, get_x = sa.machine(kind)
    reads = sa.synthetic_reads(config_id, lengths, get_x, jumps=jumps)
    return sm, reads


@pytest.mark.parametrize("kind", ["strawman", "vanilla", "hdp"])
def test_every_read_equals_the_call_on_that_read_alone(kind):
    p = sa.params()
    if kind == "hdp":
        sm, _nh, reads = sa.hdp_machine_and_reads(41, [lx for lx, _ in MIXED])
    else:
        sm, reads = _signal_case(kind, MIXED, 41)
    refs = [sa.alone(sm, rd, p) for rd in reads]
    out = sa.run_stream(sm, reads, p, maxReadsPerChunk=4, slots=3)
    _identical(out, refs, 12)
    assert out["n_chunks"] >= 3 and out["n_refused"] == 0 and len(out["chunks"]) == out["n_chunks"]
    assert sum(c["nReads"] for c in out["chunks"]) == 12 and all(c["nReads"] <= 4 for c in out["chunks"])
    assert out["delivered"] == list(range(12))  # one class, nothing cut: chunks in submission order, and reads inside them
    assert all(c["deviceBytes"] > 0 for c in out["chunks"]) and out["peak"] > 0


@pytest.mark.parametrize("kind", ["sm4", "echelon", "dna5"])
def test_the_other_three_machines_in_two_chunks(kind):
    p = sa.params()
    if kind == "dna5":
        p.contents.minDiagsBetweenTraceBack = 60
        p.contents.traceBackDiagonals = 10
        sm, reads = sa.dna_machine_and_reads(43, [180, 260, 210, 300])
    else:
        sm, reads = _signal_case(kind, MIXED[:4], 43)
    refs = [sa.alone(sm, rd, p, echelon=kind == "echelon") for rd in reads]
    out = sa.run_stream(sm, reads, p, maxReadsPerChunk=2, slots=2, oneClass=1)
    _identical(out, refs, 4)
    assert out["n_chunks"] == 2 and out["n_refused"] == 0 and out["delivered"] == [0, 1, 2, 3]


def test_a_second_machine_kind_is_refused_by_submit():
    """(in a child process: the refusal ends the process, as the batch call's does)"""
    import subprocess
    import sys
    code = ("import stream_api as sa, ctypes as C\n"
            "L = sa.lib(); p = sa.params()\n"
            "a, ga = sa.machine('strawman'); b, gb = sa.machine('vanilla')\n"
            "ra = sa.synthetic_reads(1, [(100, 200)], ga); rb = sa.synthetic_reads(1, [(100, 200)], gb)\n"
            "sa.run_stream([a, b], ra + rb, p, slots=2)\n")
    import os
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(sys.path))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 1 and "cannot mix state machine kinds" in r.stderr


# four reads without a jump, four with the jump that needs three cells per lane, four with the jump past 248 k-mers
CLASS_JUMPS = [0, 90, 260] * 4


def _kernels(chunks):
    return sorted({(c["kernel"], c["wave"], c["rows"]) for c in chunks})


def test_strawman_reads_are_grouped_by_the_kernel_each_runs_on_alone():
    p = sa.params()
    sm, reads = _signal_case("strawman", [(360, 720)] * 12, 45, jumps=CLASS_JUMPS)
    widths = [cp.band_extent(rd.anchors, rd.lX, rd.lY, 20)[0] for rd in reads]
    assert all(w <= 120 for w in widths[0::3]) and all(120 < w <= 184 for w in widths[1::3])
    assert all(w > 248 for w in widths[2::3])
    refs = [sa.alone(sm, rd, p) for rd in reads]
    out = sa.run_stream(sm, reads, p, slots=3)
    _identical(out, refs, 12)
    # one chunk per class, none mixing them: the narrow reads at two cells per lane, the middle ones at three, the wide
    # ones on the general kernel -- with each class's own widest band
    assert _kernels(out["chunks"]) == [(sa.KERNEL_GENERAL, 0, 0), (sa.KERNEL_SYSTOLIC, 1, 2), (sa.KERNEL_SYSTOLIC, 1, 3)]
    assert sorted(c["nReads"] for c in out["chunks"]) == [4, 4, 4]
    by_kernel = {(c["kernel"], c["rows"]): c["maxWidth"] for c in out["chunks"]}
    assert by_kernel[(sa.KERNEL_SYSTOLIC, 2)] == max(widths[0::3])
    assert by_kernel[(sa.KERNEL_SYSTOLIC, 3)] == max(widths[1::3])
    assert by_kernel[(sa.KERNEL_GENERAL, 0)] == max(widths[2::3])
    # without the grouping the widest read picks the kernel for all: what callers had
    one = sa.run_stream(sm, reads, p, slots=3, oneClass=1)
    _identical(one, refs, 12)
    assert _kernels(one["chunks"]) == [(sa.KERNEL_GENERAL, 0, 0)] and one["delivered"] == list(range(12))
    for k in range(3):  # grouped: every class's reads still arrive in the order of their submission
        mine = [t for t in out["delivered"] if t % 3 == k]
        assert mine == sorted(mine) and len(mine) == 4


def test_a_vanilla_read_that_touches_an_n_gets_a_chunk_of_its_own():
    p = sa.params()
    sm, get_x = sa.machine("vanilla")
    reads = sa.synthetic_reads(47, MIXED[:6], get_x)
    seq = bytearray(reads[3].xbuf.value)
    seq[len(seq) // 2] = ord("N")
    reads[3] = sa.SeqRead(bytes(seq), reads[3].ev, get_x, reads[3].anchors)
    out = sa.run_stream(sm, reads, p, slots=2)
    assert sorted(out["delivered"]) == list(range(6)) and out["n_refused"] == 0
    for i, rd in enumerate(reads):
        ref = sa.alone(sm, rd, p)
        assert out["results"][i].shape == ref.shape and np.array_equal(out["results"][i], ref), i
    chunks = sorted(out["chunks"], key=lambda c: c["nReads"])
    assert [c["nReads"] for c in chunks] == [1, 5]
    assert chunks[0]["kernel"] == sa.KERNEL_GENERAL and chunks[1]["kernel"] == sa.KERNEL_SYSTOLIC
    _order_within_chunks(out, 6)
    assert [t for t in out["delivered"] if t != 3] == [0, 1, 2, 4, 5]


def _limit_reads():
    """the 16 reads of the memory-limit test as the host library takes them (one machine, the unscaled model)"""
    ctx = cp.Context(0)
    case = sa.limit_case(cp, ctx)
    ctx.close()
    L = h.lib()
    batch = case["batch16"]
    sm = L.getStrawManStateMachine3(None)
    m, _, gy = batch["models"][0]
    C.memmove(sm.contents.model.EMISSION_MATCH_PROBS, m.ctypes.data, m.nbytes)
    C.memmove(sm.contents.model.EMISSION_GAP_Y_PROBS, gy.ctypes.data, gy.nbytes)
    reads = []
    for it in batch["items"]:
        x = batch["x_chars"][it["x_offset"]: it["x_offset"] + it["lX"] + 5]
        ev = batch["events"][it["y_offset"]: it["y_offset"] + it["lY"]]
        reads.append(sa.SeqRead(x, ev, "sequence_getKmer",
                                batch["anchors"][it["anchor_offset"]: it["anchor_offset"] + it["n_anchors"]]))
    return case, C.cast(sm, C.c_void_p), reads


def test_the_budget_holds_and_a_read_that_cannot_fit_is_refused():
    case, sm, reads = _limit_reads()
    p = sa.params(expansion=int(case["bp"].diagonalExpansion), min_diags=int(case["bp"].minDiagsBetweenTraceBack))
    refs = [sa.alone(sm, rd, p) for rd in reads]
    L = case["L"]
    out = sa.run_stream(sm, reads, p, slots=2, deviceBytes=2 * L)
    print("limit %d: %d chunks %r, peak %d" % (L, out["n_chunks"], [(c["nReads"], c["halvings"], c["deviceBytes"])
                                                                  for c in out["chunks"]], out["peak"]))
    _identical(out, refs, 16)
    assert out["peak"] <= 2 * L and out["n_chunks"] >= 4 and out["n_refused"] == 0
    assert all(c["deviceBytes"] <= L for c in out["chunks"])
    # a budget below one read's own bytes: every read comes back refused, and nothing else is the worse for it
    tiny = sa.run_stream(sm, reads, p, slots=2, deviceBytes=2 * 4096)
    assert sorted(tiny["delivered"]) == list(range(16)) and all(v is None for v in tiny["results"].values())
    assert tiny["n_refused"] == 16 and tiny["n_chunks"] == 0
    again = sa.run_stream(sm, reads, p, slots=2)
    _identical(again, refs, 16)
    assert again["n_refused"] == 0

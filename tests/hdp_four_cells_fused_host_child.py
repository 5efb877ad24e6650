"""Child process of test_hdp_four_cells_fused_estep_gpu.py's host-library test: one read whose diagonalExpansion
makes its band 185..248 k-mers wide (seed, k-mers, anchor spacing, expansion and the expected width on the command line,
after the output file) through libcpecan_host.so's HDP E-step call (cpecan_getHdpExpectationsUsingAnchors, twice,
each call into an HdpHmmExpectations of its own) under whatever CPECAN_HDP_FOUR_CELLS_FUSED_ESTEP the parent set; writes
the transitions, the likelihood and the assignment list to the JSON file."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(os.path.dirname(HERE), "oracle")]
import numpy as np  # noqa: E402
import pyoracle as o  # noqa: E402

import host_api as h  # noqa: E402
from harness import cp, hdp_batch  # noqa: E402

out = sys.argv[1]
seed, lX, every, e, width = (int(v) for v in sys.argv[2:7])
L = h.lib()
path = os.path.join(HERE, "golden", "testTemplate.nhdp")
nhdp = o.load_nhdp(path)
batch, _ = hdp_batch(seed, 1, lX, every, nhdp)
it = batch["items"][0]
bl, br = cp.band_construct(batch["anchors"], it["lX"], it["lY"], e)
assert int(((br - bl) // 2 + 1).max()) == width and 185 <= width <= 248
nh = L.deserialize_nhdp(path.encode())
sm = L.getHdpStateMachine3(nh)
ev = np.ascontiguousarray(np.asarray(batch["events"], np.float64).reshape(-1))
xbuf = C.create_string_buffer(batch["x_chars"].encode())
sX = L.sequence_construct2(it["lX"], C.cast(xbuf, C.c_void_p), h.fn_ptr("sequence_getKmer3"),
                           h.fn_ptr("sequence_sliceNucleotideSequence2"))
sY = L.sequence_construct2(ev.size // 3, ev.ctypes.data_as(C.c_void_p), h.fn_ptr("sequence_getEvent"),
                           h.fn_ptr("sequence_sliceEventSequence2"))
p = L.pairwiseAlignmentBandingParameters_construct()
p.contents.minDiagsBetweenTraceBack = 200
p.contents.diagonalExpansion = e
lst = h.make_anchor_list([tuple(int(v) for v in a) for a in batch["anchors"]])
runs = []
for _ in range(2):
    hmm = L.cpecan_hdpExpectations_construct(0.0, 0.05)
    L.cpecan_getHdpExpectationsUsingAnchors(sm, hmm, sX, sY, lst, p, True, True)
    r = hmm.contents
    n = r.numberOfAssignments
    runs.append(dict(t=[float(v) for v in r.transitions], lik=float(r.likelihood), n=int(n),
                     kmers=[r.kmerAssignments[i * 7:i * 7 + 6].decode() for i in range(n)],
                     events=[float(r.eventAssignments[i]) for i in range(n)]))
    L.cpecan_hdpExpectations_destruct(hmm)
L.stList_destruct(lst)
L.sequence_sequenceDestroy(sX)
L.sequence_sequenceDestroy(sY)
L.pairwiseAlignmentBandingParameters_destruct(p)
L.stateMachine_destruct(sm)
L.destroy_nanopore_hdp(nh)
first, second = runs
json.dump(dict(first, first=[first["n"], first["kmers"], first["events"]],
               second=[second["n"], second["kmers"], second["events"]]), open(out, "w"))

"""Child process of test_hdp_wide_fused_estep_gpu.py's host-library test: one read whose diagonalExpansion makes its
band 300 k-mers wide (the read of test_hdp_workgroup_estep_gpu.py's host test) through libcpecan_host.so's HDP E-step
call (cpecan_getHdpExpectationsUsingAnchors, twice, each call into an HdpHmmExpectations of its own) under whatever
CPECAN_WIDE_BANDS_HDP_ESTEP and CPECAN_WIDE_BANDS_HDP_FUSED_ESTEP the parent set; writes the transitions, the likelihood
and the assignment list to the JSON file named on the command line."""
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

L = h.lib()
path = os.path.join(HERE, "golden", "testTemplate.nhdp")
nhdp = o.load_nhdp(path)
batch, _ = hdp_batch(91, 1, 299, 299, nhdp)  # a single anchor: the band is the whole matrix
it = batch["items"][0]
e = 280
bl, br = cp.band_construct(batch["anchors"], it["lX"], it["lY"], e)
assert int(((br - bl) // 2 + 1).max()) == 300
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
               second=[second["n"], second["kmers"], second["events"]]), open(sys.argv[1], "w"))

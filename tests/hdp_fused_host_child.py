"""Child process of test_hdp_fused_estep_gpu.py's host-library test: the read of test_hdp_machine_through_host_api
through libcpecan_host.so's HDP E-step call (cpecan_getHdpExpectationsUsingAnchors, twice, each call into an
HdpHmmExpectations of its own) under whatever CPECAN_HDP_FUSED_ESTEP the parent set; writes the transitions, the
likelihood and the assignment list to the JSON file named on the command line."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(os.path.dirname(HERE), "oracle")]
import numpy as np  # noqa: E402
import pyoracle as o  # noqa: E402

import host_api as h  # noqa: E402

L = h.lib()
path = os.path.join(HERE, "golden", "testTemplate.nhdp")
nh = L.deserialize_nhdp(path.encode())
sm = L.getHdpStateMachine3(nh)
parsed = o.load_nhdp(path)
om = o.HdpModel(parsed)
rng = np.random.default_rng(71)
lX = 160
x = "".join(rng.choice(list("ACGT"), lX + 5))
ev, anchors = [], []
for k in range(lX):
    row = parsed["kmer_row"][om.kmer_id(x[k:k + 6])]
    mode = parsed["grid"][int(np.argmax(parsed["y"][row]))]
    if k % 40 == 20:
        anchors.append((k, len(ev)))
    for _ in range(1 if rng.random() < 0.6 else 2):
        ev.append((mode + rng.normal(0, 1.0), 1.0, 0.01))
ev = np.ascontiguousarray(np.array(ev).reshape(-1))
xbuf = C.create_string_buffer(x.encode())
sX = L.sequence_construct2(lX, C.cast(xbuf, C.c_void_p), h.fn_ptr("sequence_getKmer3"),
                           h.fn_ptr("sequence_sliceNucleotideSequence2"))
sY = L.sequence_construct2(ev.size // 3, ev.ctypes.data_as(C.c_void_p), h.fn_ptr("sequence_getEvent"),
                           h.fn_ptr("sequence_sliceEventSequence2"))
p = L.pairwiseAlignmentBandingParameters_construct()
p.contents.minDiagsBetweenTraceBack = 100
lst = h.make_anchor_list(anchors)
runs = []
for _ in range(2):
    hmm = L.cpecan_hdpExpectations_construct(0.0, 0.05)
    L.cpecan_getHdpExpectationsUsingAnchors(sm, hmm, sX, sY, lst, p, True, True)
    e = hmm.contents
    n = e.numberOfAssignments
    runs.append(dict(t=[float(v) for v in e.transitions], lik=float(e.likelihood), n=int(n),
                     kmers=[e.kmerAssignments[i * 7:i * 7 + 6].decode() for i in range(n)],
                     events=[float(e.eventAssignments[i]) for i in range(n)]))
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

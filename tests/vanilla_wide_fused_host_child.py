"""Child process of test_vanilla_wide_fused_expectations_gpu.py's host-library test: the reads of its four-wave shape
through libcpecan_host.so's vanilla E-step call (cpecan_getVanillaExpectationsUsingAnchors, one call per read into one
VanillaHmm) under whatever CPECAN_WIDE_BANDS_VANILLA_ESTEP and CPECAN_WIDE_BANDS_VANILLA_FUSED_ESTEP the parent set, with
the template strand's model and transitions; writes the 60 skip-bin sums and the likelihood to the JSON file named on
the command line."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(os.path.dirname(HERE), "oracle")]
import numpy as np  # noqa: E402

import host_api as h  # noqa: E402
from test_vanilla_workgroup_gpu import shape_batch, shape_of  # noqa: E402

HOST_SHAPE = shape_of(4, 2)  # two reads of 450 k-mers x 900 events, each with a widest band of the four-wave class

if __name__ == "__main__":
    L = h.lib()
    sh = HOST_SHAPE
    batch = shape_batch(sh)
    sm = L.getSignalStateMachine3Vanilla(os.path.join(HERE, "golden", "template_median68pA.model").encode())
    L.stateMachine3Vanilla_setStrandTransitionsToDefaults(sm, 0)
    p = L.pairwiseAlignmentBandingParameters_construct()
    p.contents.threshold = 0.01
    p.contents.minDiagsBetweenTraceBack = sh["md"]
    p.contents.traceBackDiagonals = sh["tb"]
    p.contents.diagonalExpansion = sh["e"]
    hmm = h.VanillaExpectations()
    for it in batch["items"]:
        xbuf = C.create_string_buffer(batch["x_chars"][it["x_offset"]: it["x_offset"] + it["lX"] + 5])
        ev = np.ascontiguousarray(batch["events"][it["y_offset"]: it["y_offset"] + it["lY"]], dtype=np.float64).reshape(-1)
        an = batch["anchors"][it["anchor_offset"]: it["anchor_offset"] + it["n_anchors"]]
        sX = L.sequence_construct2(it["lX"], C.cast(xbuf, C.c_void_p), h.fn_ptr("sequence_getKmer2"),
                                   h.fn_ptr("sequence_sliceNucleotideSequence2"))
        sY = L.sequence_construct2(it["lY"], ev.ctypes.data_as(C.c_void_p), h.fn_ptr("sequence_getEvent"),
                                   h.fn_ptr("sequence_sliceEventSequence2"))
        lst = h.make_anchor_list([(int(x), int(y)) for x, y in an])
        L.cpecan_getVanillaExpectationsUsingAnchors(sm, C.byref(hmm), sX, sY, lst, p, bool(sh["ragged"][0]),
                                                    bool(sh["ragged"][1]))
        L.stList_destruct(lst)
        L.sequence_sequenceDestroy(sX)
        L.sequence_sequenceDestroy(sY)
    L.pairwiseAlignmentBandingParameters_destruct(p)
    L.stateMachine_destruct(sm)
    json.dump([float(v) for v in hmm.kmerSkipBins] + [float(hmm.likelihood)], open(sys.argv[1], "w"))

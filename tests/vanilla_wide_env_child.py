"""Child process of test_vanilla_workgroup_gpu.py's environment-switch test: one wide vanilla read through a plain
vanilla batch with no flags, and the golden template read through getSignalStateMachine3Vanilla +
getAlignedPairsUsingAnchors of libcpecan_host.so with sparse anchors and a wide expansion (a band of 185..504 k-mers),
under whatever CPECAN_WIDE_BANDS the parent set; writes what ran and the pairs to the JSON file named on the command
line."""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(os.path.dirname(HERE), "oracle")]
import host_api as h  # noqa: E402
import pyoracle as o  # noqa: E402
import synth  # noqa: E402
import test_vanilla_workgroup_gpu as t  # noqa: E402
from harness import band_params, cp  # noqa: E402

GOLDEN = os.path.join(HERE, "golden")

batch = synth.make_batch(24, 1, 400, 800, anchor_every=400, distinct_models=False)
bp = band_params(0.01, 200, 40, 300)
ctx = cp.Context(0)
res, b = t.run_vanilla(ctx, batch, t.vanilla_models(batch), bp, (1, 1), 0)
out = dict(info=b.info(), batch_pairs=res[0]["triples"].tolist())
b.close()
ctx.close()

L = h.lib()
rd = o.load_npread(os.path.join(GOLDEN, "ZymoC_ch_1_file1.npRead"))
with open(os.path.join(GOLDEN, "ZymoRef.txt")) as f:
    ref_seq = f.read().strip()
sm = L.getSignalStateMachine3Vanilla(os.path.join(GOLDEN, "template_median68pA.model").encode())
L.emissions_signal_scaleModel(sm, *rd["template_params"])
L.stateMachine3Vanilla_setStrandTransitionsToDefaults(sm, 0)
xbuf = C.create_string_buffer(ref_seq.encode())
ev = np.ascontiguousarray(rd["template_events"], dtype=np.float64).reshape(-1)
lX, lY = len(ref_seq) - 5, ev.size // 3
p = L.pairwiseAlignmentBandingParameters_construct()
# anchors from the un-banded alignment (general kernel either way): a confident pair every 150 k-mers or so
p.contents.threshold = 0.2
pairs = L.getAlignedPairsWithoutBanding(sm, C.cast(xbuf, C.c_void_p), ev.ctypes.data_as(C.c_void_p), lX, lY, p,
                                        h.fn_ptr("sequence_getKmer2"), h.fn_ptr("sequence_getEvent"),
                                        h.fn_ptr("diagonalCalculationPosteriorMatchProbs"), False, False)
first = h.list_to_array(pairs)
L.stList_destruct(pairs)
best = {}
for q, x, y in first:
    if q > 9000000:
        best[int(x)] = int(y)
anchors, py = [], -1
for x in sorted(best)[::150]:
    if best[x] > py:
        anchors.append((x, best[x]))
        py = best[x]
E = 200
p.contents.threshold = 0.01
p.contents.splitMatrixBiggerThanThis = 1 << 40  # one banded alignment, no split
p.contents.diagonalExpansion = E
p.contents.minDiagsBetweenTraceBack = 300
band_l, band_r = cp.band_construct(np.array(anchors, np.int64).reshape(-1, 2), lX, lY, E)
out["host_band_width"] = int(((band_r - band_l) // 2 + 1).max())
sX = L.sequence_construct2(lX, C.cast(xbuf, C.c_void_p), h.fn_ptr("sequence_getKmer2"),
                           h.fn_ptr("sequence_sliceNucleotideSequence2"))
sY = L.sequence_construct2(lY, ev.ctypes.data_as(C.c_void_p), h.fn_ptr("sequence_getEvent"),
                           h.fn_ptr("sequence_sliceEventSequence2"))
lst = h.make_anchor_list(anchors)
pairs = L.getAlignedPairsUsingAnchors(sm, sX, sY, lst, p, h.fn_ptr("diagonalCalculationPosteriorMatchProbs"), True, True)
out["host_pairs"] = h.list_to_array(pairs).tolist()
L.stList_destruct(pairs)
json.dump(out, open(sys.argv[1], "w"))

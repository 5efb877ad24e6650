"""Child process of test_wide_workgroup_gpu.py's environment-switch test: one wide read (band of 249..376 k-mers)
through a plain batch with no flags and through getAlignedPairsUsingAnchors of libcpecan_host.so, under whatever
CPECAN_WIDE_BANDS the parent set; writes what ran and the pairs to the JSON file named on the command line."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(os.path.dirname(HERE), "oracle")]
import host_api as h  # noqa: E402
import synth  # noqa: E402
from harness import band_params, cp, run_gpu  # noqa: E402

batch = synth.make_batch(24, 1, 400, 800, anchor_every=400, distinct_models=False)
bp = band_params(0.01, 200, 40, 300)
ctx = cp.Context(0)
res, b = run_gpu(ctx, batch, bp, kernel=cp.KERNEL_AUTO, flags=0, ragged=(1, 1))
out = dict(info=b.info(), batch_pairs=res[0]["triples"].tolist())
b.close()
ctx.close()

L = h.lib()
sm = L.getStrawManStateMachine3(None)
m, gx, gy = batch["models"][0]
C.memmove(sm.contents.model.EMISSION_MATCH_PROBS, m.ctypes.data, m.nbytes)
C.memmove(sm.contents.model.EMISSION_GAP_Y_PROBS, gy.ctypes.data, gy.nbytes)
p = L.pairwiseAlignmentBandingParameters_construct()
p.contents.diagonalExpansion = 300
p.contents.minDiagsBetweenTraceBack = 200
it = batch["items"][0]
rd = h.Read(batch["x_chars"][it["x_offset"]: it["x_offset"] + it["lX"] + 5],
            batch["events"][it["y_offset"]: it["y_offset"] + it["lY"]])
lst = h.make_anchor_list(batch["anchors"][it["anchor_offset"]: it["anchor_offset"] + it["n_anchors"]])
pairs = L.getAlignedPairsUsingAnchors(sm, rd.sX, rd.sY, lst, p, h.fn_ptr("diagonalCalculationPosteriorMatchProbs"),
                                      True, True)
out["host_pairs"] = h.list_to_array(pairs).tolist()
L.stList_destruct(pairs)
json.dump(out, open(sys.argv[1], "w"))

"""Child process of test_hdp_workgroup_gpu.py's environment-switch test: one wide HDP read through a plain HDP batch
with no flags, under whatever CPECAN_WIDE_BANDS_HDP the parent set; writes what ran, the pairs and the totals to the
JSON file named on the command line."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(os.path.dirname(HERE), "oracle")]
import pyoracle as o  # noqa: E402
import test_hdp_workgroup_gpu as t  # noqa: E402
from harness import cp  # noqa: E402

nhdp = o.load_nhdp(os.path.join(HERE, "golden", "testTemplate.nhdp"))
shape = t.shape_of(6, 0)
batch = t.shape_batch(shape, nhdp)
ctx = cp.Context(0)
res, b = t.run_hdp(ctx, nhdp, batch, t.shape_bp(shape), (1, 1), 0)
out = dict(info=b.info(), pairs=res[0]["triples"].tolist(), totals=[float(v) for v in res[0]["totals"]])
b.close()
ctx.close()
json.dump(out, open(sys.argv[1], "w"))

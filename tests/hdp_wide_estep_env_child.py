"""Child process of test_hdp_workgroup_estep_gpu.py's environment-switch test: one wide HDP read through a plain HDP
batch of expectations with no other flag, under whatever CPECAN_WIDE_BANDS_HDP_ESTEP the parent set; writes what ran,
the assignments with their exponents and the ten sums to the JSON file named on the command line."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(os.path.dirname(HERE), "oracle")]
import pyoracle as o  # noqa: E402
import test_hdp_workgroup_gpu as t  # noqa: E402
from harness import batch_results, cp  # noqa: E402

nhdp = o.load_nhdp(os.path.join(HERE, "golden", "testTemplate.nhdp"))
shape = t.shape_of(6, 0)
batch = t.shape_batch(shape, nhdp)
ctx = cp.Context(0)
ids = t.upload(ctx, nhdp)
b = t.hbatch(ctx, batch, t.shape_bp(shape, 0.05), (1, 1), cp.FLAG_EXPECTATIONS)
b.run()
b.sync()
res = batch_results(b)
out = dict(info=b.info(), assign=res[0]["triples"].tolist(), logp=[float(v) for v in res[0]["logp"]],
           sums=[float(v) for v in b.expectations(ids[0])])
b.close()
ctx.close()
json.dump(out, open(sys.argv[1], "w"))

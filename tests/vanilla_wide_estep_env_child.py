"""Child process of test_vanilla_workgroup_estep_gpu.py's environment-switch test: one wide vanilla read through a plain
vanilla batch of expectations with no other flag, under whatever CPECAN_WIDE_BANDS_VANILLA_ESTEP the parent set; writes
what ran and every model's 61 sums to the JSON file named on the command line."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(os.path.dirname(HERE), "oracle")]
import test_vanilla_workgroup_gpu as t  # noqa: E402
from harness import band_params, cp  # noqa: E402

shape = t.shape_of(6)
batch = t.shape_batch(shape)
bp = band_params(0.01, shape["md"], shape["tb"], shape["e"])
ctx = cp.Context(0)
ids = t.upload(ctx, t.vanilla_models(batch))
b = t.vbatch(ctx, batch, bp, shape["ragged"], cp.FLAG_EXPECTATIONS)
b.run()
b.sync()
out = dict(info=b.info(), sums=[[float(v) for v in b.expectations(m)] for m in ids])
b.close()
ctx.close()
json.dump(out, open(sys.argv[1], "w"))

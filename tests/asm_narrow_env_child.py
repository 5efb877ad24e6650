"""Child process of test_asm_narrow_gpu.py's environment-variable test: the main batch of that file through a plain
strawMan batch with no flags, under whatever CPECAN_ASM_NARROW the parent set; writes what ran and the results (doubles
as their bits) to the JSON file named on the command line.

usage: asm_narrow_env_child.py EXPANSION OUT.json"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(os.path.dirname(HERE), "oracle")]
import test_asm_narrow_gpu as t  # noqa: E402
from harness import cp, run_gpu  # noqa: E402

ctx = cp.Context(0)
res, b = run_gpu(ctx, t.main_batch(), t.main_bp(int(sys.argv[1])), flags=0, ragged=t.RAGGED)
out = dict(info=b.info(), items=[dict(cells=r["cells"], triples=r["triples"].ravel().tolist(),
                                      logp=np.asarray(r["logp"]).view(np.uint64).tolist(), totals_xay=r["totals_xay"].tolist(),
                                      totals=np.asarray(r["totals"]).view(np.uint64).tolist()) for r in res])
b.close()
ctx.close()
json.dump(out, open(sys.argv[2], "w"))

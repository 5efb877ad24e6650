"""The widest band of every shape test_hdp_workgroup_gpu.py uses, from cpecan_band_construct alone (no GPU): which HDP
build of the workgroup family each one asks for under CPECAN_FLAG_WIDE_BANDS_HDP (six or eight waves), how many
traceback windows its reads span, and how many of the fuzz cases land in each class.
Run: python tests/tools/hdp_wide_shapes.py [fuzz scale]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import pyoracle as o  # noqa: E402
import test_hdp_workgroup_gpu as t  # noqa: E402
from harness import cp  # noqa: E402

nhdp = o.load_nhdp(os.path.join(ROOT, "tests", "golden", "testTemplate.nhdp"))


def widest(batch, e):
    w = 0
    for it in batch["items"]:
        an = batch["anchors"][it["anchor_offset"]: it["anchor_offset"] + it["n_anchors"]]
        L, R = cp.band_construct(an, it["lX"], it["lY"], e)
        w = max(w, int(((R - L) // 2 + 1).max()))
    return w


for s in t.SHAPES:
    batch = t.shape_batch(s, nhdp)
    w = widest(batch, s["e"])
    print("shape seed %d: widest band %d -> %s (wanted %d), windows %s" % (
        s["seed"], w, t.build_of(w), s["rows"], [(it["lX"] + it["lY"]) // s["md"] for it in batch["items"]]))
for rows in sorted(t.THRESHOLD_ZERO):
    batch, _, bp = t.threshold_zero_read(rows, nhdp)
    w = widest(batch, bp.diagonalExpansion)
    print("threshold-0 read for %d waves: widest band %d -> %s" % (rows, w, t.build_of(w)))
cases = t.fuzz_cases(24 * (int(sys.argv[1]) if len(sys.argv) > 1 else 1))
ran = {6: 0, 8: 0, None: 0}
for c in cases:
    w = widest(t.fuzz_batch(c, nhdp), c["e"])
    ran[t.build_of(w)] += 1
    print("fuzz seed %d: lX %d every %d e %d -> %d (%s)" % (c["seed"], c["lX"], c["every"], c["e"], w, t.build_of(w)))
print("fuzz: %d cases, %d on six waves, %d on eight, %d elsewhere" % (len(cases), ran[6], ran[8], ran[None]))

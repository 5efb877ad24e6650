"""The widest band of every shape test_vanilla_workgroup_gpu.py uses, from cpecan_band_construct alone (no GPU): which
vanilla build of the workgroup family each one asks for under CPECAN_FLAG_WIDE_BANDS (four, six or eight waves), and
how many of the fuzz cases land in each class.  Run: python tests/tools/vanilla_wide_shapes.py [fuzz scale]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import synth  # noqa: E402
import test_vanilla_workgroup_gpu as t  # noqa: E402
from harness import cp  # noqa: E402


def widest(batch, e):
    w = 0
    for it in batch["items"]:
        an = batch["anchors"][it["anchor_offset"]: it["anchor_offset"] + it["n_anchors"]]
        L, R = cp.band_construct(an, it["lX"], it["lY"], e)
        w = max(w, int(((R - L) // 2 + 1).max()))
    return w


for s in t.SHAPES:
    w = widest(t.shape_batch(s), s["e"])
    print("shape seed %d: widest band %d -> %s (wanted %d)" % (s["seed"], w, t.build_of(w), s["rows"]))
for rows, e in sorted(t.THRESHOLD_ZERO_E.items()):
    w = widest(synth.make_batch(70 + rows, 1, 400, 800, anchor_every=400), e)
    print("threshold-0 read for %d waves: widest band %d -> %s" % (rows, w, t.build_of(w)))
cases = t.fuzz_cases(24 * (int(sys.argv[1]) if len(sys.argv) > 1 else 1))
ran = {4: 0, 6: 0, 8: 0, None: 0}
for c in cases:
    w = widest(t.fuzz_batch(c), c["e"])
    ran[t.build_of(w)] += 1
    print("fuzz seed %d: lX %d every %d e %d -> %d (%s)" % (c["seed"], c["lX"], c["every"], c["e"], w, t.build_of(w)))
print("fuzz: %d cases, %d on four waves, %d on six, %d on eight, %d elsewhere" % (len(cases), ran[4], ran[6], ran[8],
                                                                                 ran[None]))

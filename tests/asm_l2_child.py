"""Child process of test_asm_sweeps_l2_cpu.py (asm_harness imports the generator once per process, so the cells per lane
are fixed by CPECAN_ASM_L in this process's environment): the two-cell assembly sweeps on the instruction emulator, as
test_asm_sweeps_cpu.py runs the three-cell ones -- every forward cell in the ring, every backward cell in the registers
at tail0..2, every refresh folded with the oracle's logAdd, window by window against the oracle's cell dump, the final
state and the cell count.

usage: asm_l2_child.py CASE   (an index into CASES; exit status 0: everything equal)
"""
import math
import os
import sys

import numpy as np

BACKWARD = "cpecan_k_asm_backward_l2"

# (seed, lX, lY, anchor_every, ragged, diagonalExpansion, widest band, windows): widths and window counts asserted below
CASES = [
    (21, 257, 330, 50, (1, 0), 20, 71, 5),        # slots wrap past column 128
    (21, 257, 330, 50, (1, 0), 50, 101, 6),
    (5, 90, 420, 50, (0, 1), 50, 90, 5),          # the band holds every column
    (9, 100, 230, 10 ** 6, (1, 1), 50, 101, 3),   # a k-mer entering on every diagonal
    # the widest band the two-cell sweeps take, ASM2_MAX_WIDTH = 120.  (The same read at an expansion
    # of 69 has a band of 120 too, but the library takes no such batch: it refuses an odd expansion, as the reference
    # does, and with anchors every 50 that band's edges jump by two k-mers and step back, which no register-resident
    # kernel takes.  Anchors every 68 columns and an expansion of 50 give 120 with edges that step by one.)
    (21, 257, 330, 68, (1, 0), 50, 120, 4),
    (21, 257, 330, 50, (1, 0), 0, 51, 4),         # no expansion: the band is what the anchors' spacing leaves
]


def same(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


def forward_rows(img, item, w, F, off):
    xmin, xmax, _, _ = img.bands[item]
    _, ctl = img.plans[item]
    bad = []
    for d in range(w["d0"] + 1, w["top"] + 1):
        row = img.ring_row(item, d)
        full = (int(ctl[d >> 6, 2]) >> (d & 63)) & 1
        for x in range(xmin[d], xmax[d] + 1):
            lane, j = H.slot_of(x)
            base = j * (G.LAYER_BYTES // 8)
            fxy = base + G.OFF_FXY // 8
            got = (row[base + 2 * lane], row[fxy + 2 * lane], row[fxy + 2 * lane + 1])
            want = F[off[d] + x - xmin[d]]
            if not (same(got[0], want[0]) and (not full or (same(got[1], want[1]) and same(got[2], want[2])))):
                bad.append((d, x, got, tuple(want)))
    return bad


def backward_hooks(img, item, cur, B, off, bad):
    xmin, xmax, _, _ = img.bands[item]

    def make(kk):
        def hook(w):
            t = int(w.s[8])
            win = cur[0]
            if t > win["frm"] or t <= win["to"]:
                return
            for x in range(xmin[t], xmax[t] + 1):
                lane, j = H.slot_of(x)

                def rd(r):
                    return np.array([int(w.v[r][lane]) | (int(w.v[r + 1][lane]) << 32)], np.uint64).view(np.float64)[0]

                got = (rd(G.B_M0 + 2 * G.L * kk + 2 * j), rd(G.B_BX0 + 2 * j), rd(G.B_BX0 + 2 * G.L + 2 * j))
                want = B[off[t] + x - xmin[t]]
                if not all(same(g, r) for g, r in zip(got, want)):
                    bad.append((t, x, got, tuple(want)))
        return hook

    return {".L_%s_tail%d" % (BACKWARD, kk): make(kk) for kk in range(3)}


def run(seed, lX, lY, every, ragged, e, widest, windows):
    assert G.L == 2 and H.P == 128 and G.ROW_BYTES == 5120
    batch = synth.make_batch(seed, 1, lX, lY, anchor_every=every)
    bp = band_params(0.01, 150, 40, e)
    img = H.Image(batch, bp, ragged, cp.NANOPORE_TRANSITIONS)
    xmin, xmax, _, _ = img.bands[0]
    wins, _ = img.plans[0]
    width = int((xmax - xmin + 1).max())
    assert width <= G.MAX_WIDTH == 120, width
    for edge in (xmin, xmax):   # what the kernel choice asks of a band before any register-resident kernel takes it
        assert ((np.diff(edge) >= 0) & (np.diff(edge) <= 1)).all(), "band edges do not step by one"
    assert widest is None or width == widest, (width, widest)
    assert windows is None or len(wins) == windows, (len(wins), windows)
    assert len(wins) >= 3
    ref = run_oracle_item(batch, 0, bp, ragged, dump=True)
    F, B, off = ref["F"], ref["B"], ref["offsets"]
    thr = math.log(0.01) - 1e-3
    ladd = pyoracle.lib().orc_logAdd
    totals = {int(a): float(b) for a, b in zip(ref["totals_xay"], ref["totals"])}
    cur, bad_b = [None], []
    watch = backward_hooks(img, 0, cur, B, off, bad_b)
    for wi, w in enumerate(wins):
        H.run_forward(img, wi, 0)
        bad_f = forward_rows(img, 0, w, F, off)
        assert not bad_f, "forward cells, window %d: %r" % (wi, bad_f[:4])
        cur[0] = w
        H.run_backward(img, wi, 0, thr, watch)
        assert not bad_b, "backward cells, window %d: %r" % (wi, bad_b[:4])
        rec = img.state(0)["win"][wi & 3]
        assert rec["valid"] == 3 and rec["top"] == w["top"] and rec["frm"] == w["frm"] and rec["to"] == w["to"]
        n_refresh = len([t for t in range(w["tpost0"], w["to"], -10)])
        assert rec["nRefresh"] == n_refresh
        # the refreshes' terms folded as the post kernel folds them: the cells of t by column, then the cells of t + 1
        for t, lo, hi, nlo, nhi, second, v, wt in img.refreshes(0, n_refresh):
            tot = float("-inf")
            for x in range(lo, hi + 1):
                tot = ladd(tot, float(v[x % H.P]))
            if second:
                acc = float("-inf")
                for x in range(nlo, nhi + 1):
                    acc = ladd(acc, float(wt[x % H.P]))
                tot = ladd(tot, acc)
            assert t in totals and tot == totals[t], "totalProbability of diagonal %d: %r, oracle %r" % (t, tot, totals.get(t))
    st = img.state(0)
    assert st["finished"] == 1 and st["d"] == lX + lY
    assert st["cells"] == int((xmax - xmin + 1).sum())
    print("case ok: widest band %d, %d windows" % (width, len(wins)))


if __name__ == "__main__":   # (the parent imports this file for CASES alone)
    assert os.environ.get("CPECAN_ASM_L") == "2", "run by test_asm_sweeps_l2_cpu.py with CPECAN_ASM_L=2"
    HERE = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [HERE, os.path.join(os.path.dirname(HERE), "oracle")]
    import asm_harness as H
    import pyoracle
    import synth
    from harness import band_params, cp, run_oracle_item
    G = H.G
    run(*CASES[int(sys.argv[1])])

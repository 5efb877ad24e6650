"""The post kernel's totals (cpecan_k_wv_post, phase T): the refresh terms go through an LDS tile, four terms of each
of 256 rows at a time, loaded by the whole workgroup, and every thread folds its own row from the tile in the order it
had.  Totals bit-identical to the oracle's and the pairs the oracle's, on the compiled wave builds (two, three, four
cells per lane, CPECAN_ASM=0) and on the assembly sweeps (three cells, and two behind CPECAN_FLAG_ASM_NARROW_BANDS),
which write the same rows.

What a case has to hold is asserted from the band (cpecan_band_construct) and the oracle's refresh diagonals, before the
GPU is asked: a refresh on diagonal t owns the rows of t (terms x = xmin..xmax of t) and of t + 1, the second one only
where the window reaches that far (the alignment's last diagonal has none above it); a window of n refreshes is 2n
rows, the missing ones counted, folded 256 at a time.

- two rounds of rows: a window of more than 128 refreshes (minDiagsBetweenTraceBack 1700)
- a short final round: a window of 129 refreshes, two rows in its second round (minDiagsBetweenTraceBack 1330)
- rows that wrap: reads of some 600 k-mers (a row's slots are x mod 64 * cells), one beginning within four slots of the
  wrap and running through it
- rows of 1, 2, 3, 4 and 5 terms (the tile's four, one less, one more) and of the widest band: the last refreshes of a
  first window that is traced back from a diagonal = 1 or 3 mod 10 lie on diagonals 1 and 3, whose rows and their
  partners' have 2 to 5 terms; the alignment's last diagonal has one
- rows of unequal length in one round: anchors every 40 or 50 k-mers under an expansion of 60 to 140
- no second row: the refresh on the alignment's last diagonal
- ragged and fixed ends: with fixed ends the cells beside the corners are out of every state's reach, their terms -inf
- the fused E-step's post kernel (the same phase T): totals bit-identical, expectations to 1e-9 (the suite's bar)
"""
import numpy as np
import pytest

import synth
from harness import assert_same_posterior, band_params, cp, run_gpu, run_oracle_item
from test_fuzz_expectations_gpu import (assert_expectations_match, assert_path, assert_same_totals, env, oracle_of,
                                        run_expectations)

pytestmark = pytest.mark.gpu

TILE = 4  # WV_POST_C of cpecan_kernel_wave.hip: the terms of a row the tile holds
# per cells per lane: anchor spacing and expansion that put the widest band in the build's range
SHAPES = {2: dict(every=40, e=60, lo=57, hi=120), 3: dict(every=50, e=100, lo=121, hi=158),
          4: dict(every=50, e=140, lo=185, hi=248)}
# (name, cells per lane, CPECAN_ASM, flags, assembly sweeps expected)
PATHS = [("l2", 2, "0", 0, False), ("l3", 3, "0", 0, False), ("l4", 4, "0", 0, False), ("asm3", 3, None, 0, True),
         ("asm2", 2, None, cp.FLAG_ASM_NARROW_BANDS, True)]
# name: minDiagsBetweenTraceBack, ragged ends; traceBackDiagonals is 40, so the first window is traced back from
# diagonal md - 41
CASES = dict(two_rounds=(1700, (1, 1)), short_final_round=(1330, (0, 0)), rows_of_2_3=(1702, (1, 0)),
             rows_of_4_5=(1704, (0, 1)))
N_READS, LX, LY = 3, 600, 1200


@pytest.fixture(scope="module")
def ctx():
    c = cp.Context(0)
    yield c
    c.close()


_BATCH, _REF = {}, {}


def batch_of(cells):
    if cells not in _BATCH:
        _BATCH[cells] = synth.make_batch(70 + cells, N_READS, LX, LY, anchor_every=SHAPES[cells]["every"],
                                         length_sigma=0.05)
    return _BATCH[cells]


def oracle(cells, case):
    """the oracle's results of a shape's batch under a case's parameters: computed once, shared by the paths"""
    if (cells, case) not in _REF:
        md, ragged = CASES[case]
        batch = batch_of(cells)
        bp = band_params(0.01, md, 40, SHAPES[cells]["e"])
        _REF[cells, case] = [run_oracle_item(batch, i, bp, ragged) for i in range(N_READS)]
    return _REF[cells, case]


def windows_of(batch, i, e, ref):
    """the refresh rows of item i, window by window, in the post kernel's order: [[(lo, hi), ...], ...]"""
    it = batch["items"][i]
    an = batch["anchors"][it["anchor_offset"]: it["anchor_offset"] + it["n_anchors"]]
    L, R = cp.band_construct(an, it["lX"], it["lY"], e)
    t = np.arange(len(L))
    xlo, xhi = (t + L + 1) // 2, (t + R) // 2  # x = (t + (x - y)) / 2 over the band's x - y of diagonal t
    xay = np.asarray(ref["totals_xay"])
    out = []
    for w in np.split(xay, np.flatnonzero(np.diff(xay) > 0) + 1):
        rows = []
        for d in w:
            rows.append((int(xlo[d]), int(xhi[d])))
            # (the partner of the alignment's last diagonal: no row, its slot among the 2n stays empty)
            rows.append((int(xlo[d + 1]), int(xhi[d + 1])) if d + 1 < len(L) else None)
        out.append(rows)
    return out


def assert_case_holds(cells, case, refs):
    """the batch and the parameters give the rows the case is named for"""
    batch, e, P = batch_of(cells), SHAPES[cells]["e"], 64 * cells
    wins = [w for i in range(N_READS) for w in windows_of(batch, i, e, refs[i])]
    rows = [r for w in wins for r in w if r is not None]
    lens = set(hi - lo + 1 for lo, hi in rows)
    assert any(r is None for w in wins for r in w)                                   # a refresh without a second row
    assert any(lo % P >= P - TILE and lo % P + hi - lo >= P for lo, hi in rows)      # begins by the wrap, runs through it
    assert 1 in lens and max(lens) >= SHAPES[cells]["lo"]
    first = [r[1] - r[0] + 1 for r in wins[0][:256] if r is not None]
    assert max(first) - min(first) > 2 * TILE                                        # unequal rows in one round
    if case == "two_rounds":
        assert any(len(w) > 256 + 64 for w in wins)
    elif case == "short_final_round":
        assert any(len(w) % 256 == 2 for w in wins)
    elif case == "rows_of_2_3":
        assert {2, 3} <= lens
    else:
        assert {TILE, TILE + 1} <= lens


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("path", PATHS, ids=lambda p: p[0])
def test_totals_and_pairs_are_the_oracles(ctx, path, case):
    name, cells, asm, flags, assembly = path
    md, ragged = CASES[case]
    batch, shape = batch_of(cells), SHAPES[cells]
    refs = oracle(cells, case)
    assert_case_holds(cells, case, refs)
    bp = band_params(0.01, md, 40, shape["e"])
    with env(CPECAN_ASM=asm):
        res, b = run_gpu(ctx, batch, bp, kernel=cp.KERNEL_AUTO, flags=flags, ragged=ragged)
    info = b.info()
    b.close()
    assert shape["lo"] <= info["max_band_width"] <= shape["hi"], info
    assert info["kernel"] == "systolic" and info["family"] == "wave" and info["cells_per_lane"] == cells, info
    assert (info.get("assembly_sweeps") == 2) == assembly, info
    for i in range(N_READS):
        assert np.array_equal(res[i]["totals"], refs[i]["totals"]), (name, case, i)
        assert_same_posterior(res[i], refs[i], (name, case, i))


@pytest.mark.parametrize("cells", [2, 3])
def test_fused_expectations_through_the_same_fold(ctx, cells):
    """the strawMan E-step summed inside the sweep back: its post kernel settles the window's totals with the same
    phase T before it scales the sums by them"""
    md, ragged = CASES["two_rounds"]
    batch = batch_of(cells)
    bp = band_params(0.01, md, 40, SHAPES[cells]["e"])
    ref_items, ref = oracle_of(("post_fold", cells), batch, bp, ragged, None)
    res, info, got = run_expectations(ctx, batch, bp, ragged, "fused")
    assert_path(info, "fused")
    assert info["cells_per_lane"] == cells, info
    assert_same_totals(res, ref_items, cells)
    for j, (g, r) in enumerate(zip(got, ref)):
        assert_expectations_match(g, r, (cells, j))

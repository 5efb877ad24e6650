"""cpecan_band_extent (C-ABI, no device): the widest diagonal of an item's band and whether its edges step by one,
against the widths and columns read off cpecan_band_construct's own table -- on the vectors of test_geometry.py and on
anchors with one jump, which must land on the builds the stream's class test counts on."""
import numpy as np
import pytest

import stream_api as sa
import synth
from cpecan_load import binding

cp = binding()


def extent_from_table(anchors, lX, lY, e):
    """the same two facts, read off the band's table diagonal by diagonal"""
    L, R = cp.band_construct(anchors, lX, lY, e)
    k = np.arange(L.size, dtype=np.int64)
    widest = int((((R.astype(np.int64) - L) >> 1) + 1).max())
    # matrix columns of the two edges (C division: k + L and k + R are never negative)
    lo, hi = (k + L) // 2, (k + R) // 2
    steps = all(np.all((np.diff(c) >= 0) & (np.diff(c) <= 1)) for c in (lo, hi))
    return widest, bool(steps)


def _random_anchors(rng, lX, lY, step):  # (as test_geometry.py draws them)
    out, x, y = [], -1, -1
    while True:
        x += int(rng.integers(1, step))
        y += int(rng.integers(1, step))
        if x >= lX or y >= lY:
            return out
        out.append((x, y))


def test_extent_of_the_golden_band():
    anchors = [(1, 0), (2, 1), (3, 3)]  # tests/pairwiseAlignerTest.c:74-99
    assert cp.band_extent(anchors, 6, 5, 2) == extent_from_table(anchors, 6, 5, 2) == (4, True)


@pytest.mark.parametrize("seed", range(40))
def test_extent_matches_the_table_on_random_anchors(seed):
    rng = np.random.default_rng(seed)
    lX, lY = int(rng.integers(0, 400)), int(rng.integers(0, 400))
    e = int(rng.integers(0, 30)) * 2
    anchors = _random_anchors(rng, lX, lY, int(rng.integers(2, 60))) if seed % 5 else []
    assert cp.band_extent(anchors, lX, lY, e) == extent_from_table(anchors, lX, lY, e)


def test_extent_edge_cases():
    assert cp.band_extent([], 0, 0, 20) == (1, True)
    assert cp.band_extent([], 0, 7, 2) == extent_from_table([], 0, 7, 2)
    assert cp.band_extent([(4, 4)], 5, 5, 0) == extent_from_table([(4, 4)], 5, 5, 0)
    with pytest.raises(cp.CpecanError) as ei:
        cp.band_extent([(3, 3), (2, 5)], 10, 10, 4)
    assert ei.value.code == cp.EBAND
    with pytest.raises(cp.CpecanError):
        cp.band_extent([], 5, 5, 3)


# one jump of so many k-mers in the anchors of a 360 x 720 strawMan read, expansion 20 -> (kernel, cells per lane)
JUMPS = {0: (cp.KERNEL_SYSTOLIC, 2), 90: (cp.KERNEL_SYSTOLIC, 3), 150: (cp.KERNEL_SYSTOLIC, 4), 260: (cp.KERNEL_GENERAL, 0)}


@pytest.mark.parametrize("jump", sorted(JUMPS))
def test_extent_of_anchors_with_one_jump_and_the_build_it_lands_on(jump):
    rng = np.random.default_rng(synth.SEED0 + 5)
    rd = synth.make_read(rng, synth.synthetic_pore_model()[0], 360, 720, 30)
    anchors = sa.with_jump(rd["anchors"], jump)
    width, steps = cp.band_extent(anchors, 360, 720, 20)
    assert (width, steps) == extent_from_table(anchors, 360, 720, 20)
    plan = cp.plan_dispatch(cp.MACHINE_STRAWMAN, cp.MODE_POSTERIOR, cp.KERNEL_AUTO, cp.FLAG_SMALL_FOOTPRINT, width, steps)
    assert (plan["kernel"], plan["rows"]) == JUMPS[jump], (jump, width, steps, plan)
    assert plan["wave"] == (1 if plan["kernel"] == cp.KERNEL_SYSTOLIC else 0)
    if jump == 260:
        assert width > 248

"""GPU parity of the 4-state machine's one-wave-per-alignment kernels (cpecan_kernel_wave4.hip: cpecan_k_wave4_l1 for
bands up to 64 cells, cpecan_k_wave4_l2 for 65..128) against the oracle, at test_sm4_gpu.run's bar: every
totalProbability refresh and posterior exponent bit-identical, the pairs in the reference's emission order.

Every batch is created with CPECAN_FLAG_SM4_WAVE; each case asserts the widest band the batch reports on the side of
the 64 / 128 boundaries it means to be on, and that cpecan_hip_batch_kernel_family says wave where the width fits."""
import numpy as np
import pytest

import edge_reads as er
import pyoracle as o
import synth
from harness import assert_same_pairs, band_params, batch_results, cp, make_items, orc_params
from stream_api import with_jump
from test_sm4_gpu import models_of

pytestmark = pytest.mark.gpu

FLAG = cp.FLAG_SM4_WAVE
L1, L2 = (1, 64), (65, 128)   # widest band: one cell per lane, two


@pytest.fixture(scope="module")
def ctx():
    c = cp.Context(0)
    yield c
    c.close()


def upload(ctx, models):
    ctx.models_clear()
    ctx.models4_create([(m.transitions, m.match, m.gap_x, m.gap_y) for m in models])


def create(ctx, batch, bp, ragged, width, flags=FLAG):
    """the flagged batch, on the side of the boundaries `width` = (lo, hi) names"""
    b = cp.Batch(ctx, make_items(batch, ragged), batch["x_chars"], batch["events"], batch["anchors"], bp, flags=flags,
                 sm4=True)
    info = b.info()
    assert info["kernel"] == "general" and width[0] <= info["max_band_width"] <= width[1], info
    wave = 1 if width[1] <= 128 and flags & FLAG and not flags & (cp.FLAG_GENERAL_KERNEL | cp.FLAG_UNBANDED) else 0
    assert b.kernel_family()["wave"] == wave and (info.get("family") == "wave (4-state)") == bool(wave), info
    return b


def oracle(batch, models, bp, ragged):
    p = orc_params(bp, split=1 << 60)
    out = []
    for it in batch["items"]:
        x = batch["x_chars"][it["x_offset"]: it["x_offset"] + it["lX"] + 5]
        ev = batch["events"][it["y_offset"]: it["y_offset"] + it["lY"]]
        an = batch["anchors"][it["anchor_offset"]: it["anchor_offset"] + it["n_anchors"]]
        ref = o.aligned_pairs_using_anchors(models[it["model"]], x, it["lX"], ev, an, p, ragged[0], ragged[1])
        ref["triples"], ref["logp"] = ref["triples"][::-1], ref["logp"][::-1]
        out.append(ref)
    return out


def assert_matches(b, refs):
    got = batch_results(b)
    assert len(got) == len(refs)
    for g, ref in zip(got, refs):
        assert np.array_equal(g["totals_xay"], ref["totals_xay"])
        assert np.array_equal(g["totals"], ref["totals"])
        assert_same_pairs(g, ref)
    return got


def run(ctx, batch, models, bp, ragged, width, flags=FLAG):
    upload(ctx, models)
    b = create(ctx, batch, bp, ragged, width, flags)
    b.run()
    b.sync()
    got = assert_matches(b, oracle(batch, models, bp, ragged))
    b.close()
    return got


# (n, lX, lY, every): several traceback windows each; the widest band by the expansion
NARROW = dict(n=3, lX=120, lY=250, every=25, e=20, md=60, tb=10, width=L1)       # 46 cells
DRIVER = dict(n=3, lX=300, lY=610, every=50, e=50, md=100, tb=40, width=L2)      # 102: the driver's expansion
MARGIN = dict(n=2, lX=200, lY=410, every=40, e=30, md=12, tb=10, width=L2)       # windows shorter than the margin
MARGIN1 = dict(MARGIN, e=20, width=L1)


def synth_batch(case, seed=31):
    return synth.make_batch(seed, case["n"], case["lX"], case["lY"], anchor_every=case["every"])


@pytest.mark.parametrize("ragged", [(0, 0), (0, 1), (1, 0), (1, 1)], ids=lambda r: "ragged%d%d" % r)
@pytest.mark.parametrize("case", [NARROW, DRIVER, MARGIN, MARGIN1], ids=["l1", "l2", "margin-l2", "margin-l1"])
def test_banded_matches_oracle(ctx, case, ragged):
    batch = synth_batch(case)
    assert len(batch["models"]) > 1   # a model per read
    got = run(ctx, batch, models_of(batch), band_params(0.01, case["md"], case["tb"], case["e"]), ragged, case["width"])
    assert all(len(g["triples"]) > 0 and len(g["totals"]) > 3 for g in got)


@pytest.mark.parametrize("thr", [1e-4, 0.0])
@pytest.mark.parametrize("case", [NARROW, DRIVER], ids=["l1", "l2"])
def test_thresholds(ctx, case, thr):
    """threshold 0 emits every cell of the band: more pairs than the first run's buffer holds, so the re-run"""
    batch = synth_batch(case, seed=35)
    got = run(ctx, batch, models_of(batch), band_params(thr, case["md"], case["tb"], case["e"]), (1, 1), case["width"])
    if thr == 0.0:
        assert all(len(g["triples"]) > 4 * (it["lX"] + it["lY"]) + 64 for g, it in zip(got, batch["items"]))


EDGE = {name: er.signal_family(name) for name in ("upper", "lower", "cross", "upper-out", "w64", "w65")}
EDGE["upper100"] = dict(er.FAMILY, place="upper", lX=300, lY=450, width=100, md=150, tb=40, ragged=(0, 1))
EDGE["lower128"] = dict(er.FAMILY, place="lower", lX=300, lY=450, width=128, md=150, tb=40, ragged=(1, 1))
EDGE["cross100"] = dict(er.FAMILY, place="cross", cross=(0.45, 0.5), lX=300, lY=450, width=100, md=60, tb=30,
                        ragged=(1, 0), frac=0.05)
EDGE["upper129"] = dict(er.FAMILY, place="upper", lX=300, lY=450, width=129, md=150, tb=40, ragged=(1, 1))


@pytest.mark.parametrize("name", sorted(EDGE))
def test_band_edges(ctx, name):
    """the posterior mass on the band's first and last cells (tests/edge_reads.py), where a slot that changes hands or
    a wrong neighbour guard shows; at both kernels' widest bands and one cell past each"""
    f = EDGE[name]
    batch = er.edge_batch(f["seed"], 2, f["lX"], f["lY"], f["place"], f["offset"], every=f["every"], e=f["e"],
                          width=f["width"], cross=f["cross"], skip=f["skip"])
    w = f["width"] if f["width"] is not None else 43
    models = models_of(batch)
    for thr in (0.01, 1e-4, 0.0):
        got = run(ctx, batch, models, band_params(thr, f["md"], f["tb"], batch["e"]), f["ragged"], (w, w))
        assert all(len(g["triples"]) > 0 for g in got)


def test_a_jump_in_the_anchors(ctx):
    """an anchor-free stretch: the band widens there and narrows again behind it"""
    batch = synth_batch(dict(n=2, lX=200, lY=410, every=20))
    parts, items = [], []
    for it in batch["items"]:
        an = with_jump(batch["anchors"][it["anchor_offset"]: it["anchor_offset"] + it["n_anchors"]], 45)
        items.append(dict(it, anchor_offset=sum(len(p) for p in parts), n_anchors=len(an)))
        parts.append(an)
    batch = dict(batch, items=items, anchors=np.concatenate(parts))
    run(ctx, batch, models_of(batch), band_params(0.01, 80, 20, 20), (0, 1), L2)


def test_degenerate_items_beside_normal_ones(ctx):
    batch = synth.make_batch(32, 3, 80, 170, anchor_every=30)
    base = batch["items"][0]
    batch["items"] += [dict(base, lX=0, n_anchors=0), dict(base, lY=0, n_anchors=0), dict(base, lX=1, lY=1, n_anchors=0)]
    # a k-mer that is none in the middle of the second read
    x = bytearray(batch["x_chars"])
    x[batch["items"][1]["x_offset"] + 40] = ord("N")
    batch["x_chars"] = bytes(x)
    for e, width in ((20, L1), (50, L2)):
        got = run(ctx, batch, models_of(batch), band_params(0.01, 60, 20, e), (0, 0), width)
        assert all(len(g["triples"]) > 0 for g in got[:3]) and not len(got[3]["triples"]) and not len(got[4]["triples"])
        run(ctx, batch, models_of(batch), band_params(0.01, 60, 20, e), (1, 1), width)


def thin_anchors(batch, i, keep):
    """item i keeps every keep-th anchor: its band widens between them"""
    parts, items = [], []
    for k, it in enumerate(batch["items"]):
        an = batch["anchors"][it["anchor_offset"]: it["anchor_offset"] + it["n_anchors"]]
        an = an[::keep] if k == i else an
        items.append(dict(it, anchor_offset=sum(len(p) for p in parts), n_anchors=len(an)))
        parts.append(an)
    return dict(batch, items=items, anchors=np.concatenate(parts))


def test_the_widest_item_decides(ctx):
    """one item at 139 cells beside two at 77: the whole batch on the general kernel, the results the oracle's; the
    same reads without that item's wide stretch on the wave kernel"""
    narrow = synth.make_batch(31, 3, 150, 310, anchor_every=25)
    mixed = thin_anchors(narrow, 0, 4)
    bp = band_params(0.01, 100, 40, 50)
    run(ctx, mixed, models_of(mixed), bp, (1, 1), (129, 140))
    run(ctx, narrow, models_of(narrow), bp, (1, 1), L2)


def test_unbanded_general_kernel_and_no_flag_stay_general(ctx):
    batch = synth_batch(NARROW)
    models, bp = models_of(batch), band_params(0.01, 60, 10, 20)
    upload(ctx, models)
    for flags in (0, FLAG | cp.FLAG_GENERAL_KERNEL, FLAG | cp.FLAG_UNBANDED):
        b = cp.Batch(ctx, make_items(batch, (0, 0)), batch["x_chars"], batch["events"], batch["anchors"], bp, flags=flags,
                     sm4=True)
        assert b.info()["kernel"] == "general" and b.kernel_family()["wave"] == 0 and "family" not in b.info()
        b.close()
    # ... and such a batch, flag and all, is the general kernel's: the same results
    got = run(ctx, batch, models, bp, (0, 0), L1, flags=FLAG | cp.FLAG_GENERAL_KERNEL)
    assert all(len(g["triples"]) > 0 for g in got)


def raw(b):
    return [(g["triples"].tobytes(), g["logp"].tobytes(), g["totals_xay"].tobytes(), g["totals"].tobytes())
            for g in batch_results(b)]


@pytest.mark.parametrize("case", [NARROW, DRIVER], ids=["l1", "l2"])
def test_schedule(ctx, case):
    """one batch run twice gives the same bytes; a second flagged batch, of another context, chained behind the first
    with run(after=...) is the oracle's, as is the first"""
    first, second = synth_batch(case, seed=36), synth_batch(dict(case, n=2), seed=37)
    bp = band_params(0.01, case["md"], case["tb"], case["e"])
    m1, m2 = models_of(first), models_of(second)
    other = cp.Context(0)
    try:
        upload(ctx, m1)
        upload(other, m2)
        b1, b2 = create(ctx, first, bp, (1, 1), case["width"]), create(other, second, bp, (0, 1), case["width"])
        b1.run()
        b1.sync()
        once = raw(b1)
        b1.run()
        b2.run(after=b1)
        b2.sync()
        b1.sync()
        assert raw(b1) == once
        assert_matches(b1, oracle(first, m1, bp, (1, 1)))
        assert_matches(b2, oracle(second, m2, bp, (0, 1)))
        b2.close()
        b1.close()
    finally:
        other.close()

"""(CPU) The edge reads of tests/edge_reads.py do what they claim, on the oracle's cell dump: the posterior mass sits on
the targeted edge of the band, the widest band is the build limit the case is named for, and the A-record cases give a
slot of the wave kernels two columns within one refresh segment.  Also: synth's and harness's generators still make,
byte for byte, the reads every other test was written against."""
import hashlib
import os

import numpy as np
import pytest

import edge_reads as er
import harness
import pyoracle as o
import synth
from harness import band_params


def _digest(*parts):
    h = hashlib.sha256()
    for a in parts:
        h.update(a if isinstance(a, bytes) else a.encode() if isinstance(a, str) else np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


# (make_batch arguments, digest): smoke()'s two batches, a band-edge batch of test_fuzz_expectations_gpu.py, an
# assembly-shaped batch of reads of different lengths, a batch with one shared model
GENERATOR_DIGESTS = [
    (dict(config_id=1, n_reads=3, lX=200, lY=420, anchor_every=40), "0415b56ec8e5c9ca", True),
    (dict(config_id=2, n_reads=2, lX=700, lY=1400, anchor_every=50), "df59710142ae4577", True),
    (dict(config_id=703, n_reads=2, lX=300, lY=600, anchor_every=50), "99a299d5d6304f53", True),
    (dict(config_id=5000, n_reads=3, lX=600, lY=1300, anchor_every=50, length_sigma=0.2), "b5ecc6cccc3ce8d3", False),
    (dict(config_id=9001, n_reads=3, lX=300, lY=500, anchor_every=20, distinct_models=False, length_sigma=0.3),
     "f301c95d428de0d2", False),
]


@pytest.mark.parametrize("args,digest,full", GENERATOR_DIGESTS, ids=[str(a["config_id"]) for a, _, _ in GENERATOR_DIGESTS])
def test_make_batch_unchanged(args, digest, full):
    b = synth.make_batch(**args)
    parts = [b["x_chars"], b["events"], b["anchors"]]
    if full:
        parts += [np.array([list(it.values()) for it in b["items"]])] + [m[0] for m in b["models"]]
    else:
        parts += [b["models"][0][0]] if not args.get("distinct_models", True) else []
    assert _digest(*parts) == digest


def test_hdp_batch_unchanged(golden_dir):
    nhdp = o.load_nhdp(os.path.join(golden_dir, "testTemplate.nhdp"))
    b, _ = harness.hdp_batch(4242, 2, 200, 50, nhdp)
    assert _digest(b["x_chars"], b["events"], b["anchors"]) == "cf346ec0a04874ef"


def family_masses(name):
    f = er.FAMILIES[name]
    batch = er.family_batch(name)
    bp = band_params(0.01, f["md"], f["tb"], batch["e"])
    out = []
    for i, it in enumerate(batch["items"]):
        an = batch["anchors"][it["anchor_offset"]: it["anchor_offset"] + it["n_anchors"]]
        out.append((er.widest(an, it["lX"], it["lY"], batch["e"]), er.edge_mass(batch, i, bp, f["ragged"])))
    return f, batch, out


@pytest.mark.parametrize("name", list(er.FAMILIES))
def test_family_puts_mass_on_the_edge(name):
    """on at least the family's stated fraction of the decoded diagonals (mean over the batch's reads), the targeted
    edge cell or the one next to it holds posterior >= 0.01; the first read's widest band is the family's width and no
    read's is wider; the A-record families meet the A-record condition.

    The posterior here is the cell's, summed over its three states (edge_fraction kind 'cell'), not the match state's
    alone: a match step moves two diagonals and a stay or a skip one, so a path has match mass on only about
    lX / (lX + lY) of the diagonals however sharp it is (the match-only figure of these families is 8-37 %).  A kernel's
    edge error spoils every state of the cell.  The families whose path runs outside the band ('-out') put little
    mass on the edge: no alignment in the band follows the events there, and the model takes the best one inside,
    seldom along the edge cell; they are kept for the paths they give the kernels, with a bar to match."""
    f, batch, out = family_masses(name)
    if f["place"] == "cross":  # the path runs on the lower edge, then crosses to the upper one within a window
        lo = np.mean([er.edge_fraction(m, "lower", 0.01, kind="cell") for _, m in out])
        hi = np.mean([er.edge_fraction(m, "upper", 0.01, kind="cell") for _, m in out])
        assert lo >= f["frac"] and hi >= f["frac"], (lo, hi)
    else:
        fr = np.mean([er.edge_fraction(m, f["place"], 0.01, kind="cell") for _, m in out])
        assert fr >= f["frac"], fr
    if f["width"] is not None:
        assert out[0][0] == f["width"] and max(w for w, _ in out) == f["width"], [w for w, _ in out]
    if f["arec"] is not None:
        assert any(er.a_record_slots(m, f["arec"]) for _, m in out)


@pytest.mark.parametrize("name", ["upper", "w120"])
def test_edge_reads_far_above_the_fuzz_inputs(name):
    """the point of the generator: the fuzz sweep's inputs (test_fuzz_gpu.py::cases) put mass on an edge cell on a
    few diagonals in a hundred; an edge family on most of them (both measured the same way: the cell's posterior,
    all states, on either edge for the fuzz inputs)"""
    import test_fuzz_gpu as tf
    old = []
    for c in tf.cases(4, 20251004):
        b = synth.make_batch(c["seed"], 1, c["lX"], c["lY"], anchor_every=c["every"])
        m = er.edge_mass(b, 0, band_params(0.01, c["md"], c["tb"], c["e"]), c["ragged"])
        old.append(max(er.edge_fraction(m, "lower", 0.01, kind="cell"), er.edge_fraction(m, "upper", 0.01, kind="cell")))
    _, _, out = family_masses(name)
    new = np.mean([er.edge_fraction(m, "upper", 0.01, kind="cell") for _, m in out])
    assert new >= 0.5 and new > 10 * max(max(old), 0.01), (new, old)


# the existing families and the HDP form, pinned before the generator gained the DNA and wide families
FAMILY_DIGESTS = [("upper", "c194b2177262fed2"), ("w184", "52dcae084963502e"), ("arec120", "1b9af137ef8d3b93"),
                  ("cross", "dc044a6c361142d1")]


@pytest.mark.parametrize("name,digest", FAMILY_DIGESTS, ids=[n for n, _ in FAMILY_DIGESTS])
def test_edge_family_unchanged(name, digest):
    b = er.family_batch(name)
    assert _digest(b["x_chars"], b["events"], b["anchors"], np.array([list(it.values()) for it in b["items"]]),
                   *[m[0] for m in b["models"]]) == digest


def test_edge_hdp_family_unchanged(golden_dir):
    nhdp = o.load_nhdp(os.path.join(golden_dir, "testTemplate.nhdp"))
    b = er.family_batch("w248", hdp=(nhdp, o.HdpModel(nhdp)))
    assert _digest(b["x_chars"], b["events"], b["anchors"]) == "5933f77e595bd8c3" and b["e"] == 244


def _edge_fractions(m, place):
    places = ("lower", "upper") if place == "cross" else (place,)
    return [er.edge_fraction(m, p, 0.01, kind="cell") for p in places]


@pytest.mark.parametrize("name", list(er.DNA_FAMILIES))
def test_dna_family_puts_mass_on_the_edge(name):
    """the DNA families on the oracle's 5-state cell dump (posterior summed over the five states): the targeted edge
    cell or the one next to it holds posterior >= 0.01 on at least the family's stated fraction of the decoded
    diagonals (mean over the batch; both edges for 'cross'); the first read's widest band is the family's width, no
    read's is wider"""
    f = er.DNA_FAMILIES[name]
    b = er.dna_batch(name)
    bp = band_params(0.01, f["md"], f["tb"], b["e"])
    widths = [er.widest(a, len(x), len(y), b["e"]) for x, y, a in b["seqs"]]
    fr = np.mean([_edge_fractions(er.dna_edge_mass(x, y, a, bp, f["ragged"]), f["place"]) for x, y, a in b["seqs"]],
                 axis=0)
    assert np.all(fr >= f["frac"]), fr
    if f["width"] is not None:
        assert widths[0] == f["width"] and max(widths) == f["width"], widths
    assert all(len(x) == f["lX"] for x, _, _ in b["seqs"])


def test_dna_centred_batch_keeps_the_band():
    """the stale-state cases' centred batch: the same x and anchors as the edge batch, its mass off the edge"""
    b, c = er.dna_batch("w128"), er.dna_batch("w128", centred=True)
    f = er.DNA_FAMILIES["w128"]
    bp = band_params(0.01, f["md"], f["tb"], b["e"])
    assert c["e"] == b["e"]
    for (x, y, a), (cx, cy, ca) in zip(b["seqs"], c["seqs"]):
        assert cx == x and np.array_equal(ca, a) and len(cy) == len(y)
        edge = er.edge_fraction(er.dna_edge_mass(x, y, a, bp, f["ragged"]), "upper", 0.01, kind="cell")
        mid = er.edge_fraction(er.dna_edge_mass(cx, cy, ca, bp, f["ragged"]), "upper", 0.01, kind="cell")
        assert mid < 0.1 < edge, (mid, edge)


# 4-state machine: (family, bar); the machine follows the strawMan path a little less closely
SM4_FAMILIES = [("upper", 0.5), ("lower", 0.25), ("cross", 0.02), ("upper-out", 0.1), ("w256", 0.5), ("w257", 0.5)]


@pytest.mark.parametrize("name,frac", SM4_FAMILIES, ids=[n for n, _ in SM4_FAMILIES])
def test_sm4_family_puts_mass_on_the_edge(name, frac):
    """as test_family_puts_mass_on_the_edge, on the oracle's 4-state cell dump (posterior summed over the four
    states), for the families the 4-state GPU tests run"""
    f = er.signal_family(name)
    b = er.signal_batch(name)
    bp = band_params(0.01, f["md"], f["tb"], b["e"])
    p = harness.orc_params(bp, split=1 << 60)
    fr, widths = [], []
    for it in b["items"]:
        m, _, gy = b["models"][it["model"]]
        x = b["x_chars"][it["x_offset"]: it["x_offset"] + it["lX"] + 5]
        ev = b["events"][it["y_offset"]: it["y_offset"] + it["lY"]]
        an = b["anchors"][it["anchor_offset"]: it["anchor_offset"] + it["n_anchors"]]
        widths.append(er.widest(an, it["lX"], it["lY"], b["e"]))
        d = o.banded_dump(o.Sm4Model(m, gy), x, it["lX"], ev, an, p, f["ragged"][0], f["ragged"][1])
        fr.append(_edge_fractions(er._cell_mass(d), f["place"]))
    fr = np.mean(fr, axis=0)
    assert np.all(fr >= frac), fr
    if f["width"] is not None:
        assert widths[0] == f["width"] and max(widths) == f["width"], widths


# echelon machine: no edge families.  Its match emission carries almost nothing of the event's level (the sum of
# emissions_signal_multipleKmerMatchProb starts at 0.0, not at log zero: log(1 + density) - log(n)), so its posterior
# follows no path the reads are built on: at threshold 0.01 it spreads over 4-10 cells per event, a few cells inside
# the upper edge on narrow bands and far from either edge on wide ones, whatever the path.  Its reads serve the
# general kernel's widths only (64 and 256 k-mers and one past): every cell of those bands enters the totals.
ECHELON_WIDTHS = ["w64", "w65", "w256", "w257"]


@pytest.mark.parametrize("name", ECHELON_WIDTHS)
def test_echelon_reads_have_the_family_width(name):
    """edge_reads.echelon_reads keeps the batch's sequences, anchors and expansion: the first read's widest band is
    the family's width, no read's is wider; the durations lie where test_echelon_gpu.reads draws them"""
    f = er.signal_family(name)
    b = er.signal_batch(name)
    rds = er.echelon_reads(b, f["seed"])
    widths = [er.widest(r["anchors"], len(r["seq"]) - 5, len(r["events"]), b["e"]) for r in rds]
    for r in rds:
        r["machine"].close()
        assert np.all((r["events"][:, 2] >= 0.0008) & (r["events"][:, 2] < 0.012))
    assert widths[0] == f["width"] and max(widths) == f["width"], widths

"""The inputs of test_vanilla_fused_fuzz_gpu.py, and of the A-record, lower-edge and zero-bin cases that
test_vanilla_wide_fused_expectations_gpu.py and test_vanilla_workgroup_estep_gpu.py gained with it, on the oracle alone
(CPU).  What the GPU tests rely on and cannot see from their own side is asserted here, so that the inputs cannot drift.

A records.  The vanilla fused E-step keeps, per slot, the sums (beta, alpha) of the one column the slot points at and that
column's skip bin.  When the slot moves to another column inside one refresh segment and its sums are non-zero, the kernel
stores them as the segment's A record (cpecan_kernel_wave.hip `x != cA[j]`, cpecan_kernel_systolic.hip
`x + 1 != gCol`), the post kernel adds it to the model's bins, and every flush resets the next segment's A records.  That
takes a band within about ten k-mers of the slot period (WV_P = 128 / 192, SY_P = 256 / 384 / 512) that moves fast, with
gap-X mass on the column the slot leaves: edge_reads.a_record_slots finds such instances on the oracle's cell dump of the
vanilla machine.  For the workgroup kernels the rule was read from the code: SY_SLOT(x) = x % SY_P holds the forward cell
of column x and points at gCol = x + 1, a fixed shift of one, so two columns share a slot exactly when they lie SY_P apart,
as under the wave kernels' shift of none.

Held here for arec120 / arec184 (vanilla models) and varec248 / 376 / 504: an instance exists at the floor of 1e-3; the
column the slot leaves (the higher one, which the sweep back meets first) holds at least 1e-6 of the sum of its model's
60 oracle sums (measured: 3e-6 and up), so a lost record moves a bin by a thousand times the bar of 1e-9; in a wave family
and in a workgroup family the two columns of an instance fall in different skip bins (a record stored with the new
column's bin lands in the wrong bin); every model vector is finite with a negative likelihood.

Zero skip bins.  A model whose 30 skip-bin probabilities are all zero (log zero on every transition into gap X) is allowed
by the model file format, and the reference's vanilla M-step can emit a zero bin: vanillaHmm_normalizeKmerSkipBins
(impl/continuousHmm.c:424-433) divides each of the 60 sums by the total of all 60, so a bin no read visited becomes
exactly 0 when the hmm was seeded with a pseudo-count of 0.0 -- as the reference's own training test seeds it
(tests/signalPairwiseTest.c:1758) and as the loader does (:546) -- and the writer prints the bins with "%f"
(:498-500), so any bin below 5e-7 of the total reads back as 0.000000.  Only NaN is checked for (:48-58).  What the
oracle answers to such a model: with more k-mers than events every alignment needs a skip, so some refreshes of the
total give log zero (5 of 11 on the small reads here) and the E-step divides by it -- NaN in the bins those segments
touch, a likelihood of -inf; with more events than k-mers no alignment needs one: 60 exact zeros and a finite
likelihood.  With zeros in bins 0-4 only, no bin
is NaN on these reads (skips across larger level differences carry the alignment): the ten bins are exact zeros, the
others finite."""
import numpy as np
import pytest

import edge_reads as er
import pyoracle as o
import synth
from harness import band_params
from test_band_edges_machines_gpu import cached
from test_fuzz_expectations_gpu import RAGGED
from test_fuzz_expectations_machines_gpu import (N_CASES, VANILLA, W2, W3, assert_sane, bp_of, case_id, signal_width,
                                                 vanilla_batch, vanilla_oracle, vanilla_posteriors)
from test_vanilla_gpu import skip_bins
from test_vanilla_workgroup_gpu import build_of

FLOOR = 1e-3
# family -> the slot period of the build that runs it
AREC = {"arec120": 128, "arec184": 192, "varec248": 256, "varec376": 384, "varec504": 512}
LOWER = {"vlower248": 248, "vlower376": 376, "vlower504": 504}
# the wave builds' band-edge families (each with its own ragged pair): w185 is one k-mer past the three-cell build
EDGE_FAMILIES = ["upper", "upper1", "upper-out", "lower", "lower1", "lower-out", "cross", "w120", "w121", "w184", "w185"]


def family_case(name, centred=False):
    """(key, batch, models, band parameters, ragged) of an edge family under the vanilla machine: one model per read
    with skip bins of its own (o.VanillaModel(match_i, skip_bins(i), gap_y_i)); centred: the same band, the mass down
    its middle"""
    f = er.signal_family(name)
    key = ("vf-family", name, centred)
    batch = cached(key, lambda: er.signal_batch(name, centred=centred))
    models = [o.VanillaModel(m, skip_bins(i), gy) for i, (m, _, gy) in enumerate(batch["models"])]
    return key, batch, models, band_params(0.01, f["md"], f["tb"], batch["e"]), f["ragged"]


def oracle_sums(key, batch, models, bp, ragged):
    return cached(key + ("e",), lambda: vanilla_oracle(batch, models, bp, ragged))


def oracle_posteriors(key, batch, models, bp, ragged):
    return cached(key + ("post",), lambda: vanilla_posteriors(batch, models, bp, ragged))


def a_record_instances(name):
    """per item: [(segment's top diagonal, slot, higher column, its gap-X mass, lower column, the two columns' skip
    bins)] at the period of the build that runs the family"""
    key, batch, models, bp, ragged = family_case(name)

    def find():
        out = []
        for i, it in enumerate(batch["items"]):
            m = er.vanilla_edge_mass(batch, i, models[it["model"]], bp, ragged)
            seq = batch["x_chars"][it["x_offset"]: it["x_offset"] + it["lX"] + 5]
            match = batch["models"][it["model"]][0]
            out.append([inst + ((er.column_skip_bin(seq, match, inst[2]), er.column_skip_bin(seq, match, inst[4])),)
                        for inst in er.a_record_slots(m, AREC[name], FLOOR)])
        return out
    return cached(key + ("arec",), find)


@pytest.mark.parametrize("name", list(AREC))
def test_a_record_families_on_the_oracle(name):
    key, batch, models, bp, ragged = family_case(name)
    f = er.signal_family(name)
    assert signal_width(batch, batch["e"]) == f["width"] and er.slot_period(f["arec"]) == AREC[name]
    assert 0 < AREC[name] - f["width"] <= 10
    ref = oracle_sums(key, batch, models, bp, ragged)
    for v in ref:
        assert np.all(np.isfinite(v)) and v[60] < 0
    inst = a_record_instances(name)
    assert sum(len(x) for x in inst) >= 1, inst
    for it, found in zip(batch["items"], inst):
        total = ref[it["model"]][:60].sum()
        assert total <= it["lX"]  # (a column's gap-X posterior summed over a segment is at most 1)
        for top, slot, hi, mass, lo, bins in found:
            print("%s: segment %d slot %d columns %d -> %d, mass %.3g (%.3g of the model's sums), bins %s" % (
                name, top, slot, hi, lo, mass, mass / total, bins))
            assert hi - lo == AREC[name] and hi % AREC[name] == slot
            assert mass >= FLOOR and mass >= 1e-6 * total


def test_a_record_columns_in_different_skip_bins():
    """an instance whose two columns fall in different skip bins, in a wave family and in a workgroup family: an A
    record stored with the bin of the column the slot moves to would land there"""
    for names in (("arec120", "arec184"), ("varec248", "varec376", "varec504")):
        assert any(bins[0] != bins[1] for n in names for found in a_record_instances(n) for *_, bins in found), names


def test_a_records_take_the_band_near_the_period():
    """the upper-edge reads the fused tests ran before have no instance at any period: the path has to cross a stretch
    of skipped k-mers for a slot to change column within ten diagonals"""
    from test_vanilla_workgroup_estep_cases_cpu import edge_case
    key, batch, models, bp, ragged = edge_case(248)
    for i, it in enumerate(batch["items"]):
        m = er.vanilla_edge_mass(batch, i, models[it["model"]], bp, ragged)
        assert er.a_record_slots(m, 256, FLOOR) == []


def test_centred_batches_keep_the_band_and_have_no_a_record():
    """the stale-record pair: the centred batch has the A-record batch's sequences, anchors and so its band, and none of
    its instances"""
    for name in AREC:
        _, batch, _, _, _ = family_case(name)
        key, centred, models, bp, ragged = family_case(name, centred=True)
        assert centred["e"] == batch["e"] and centred["x_chars"] == batch["x_chars"]
        assert np.array_equal(centred["anchors"], batch["anchors"])
        for i, it in enumerate(centred["items"]):
            m = er.vanilla_edge_mass(centred, i, models[it["model"]], bp, ragged)
            assert er.a_record_slots(m, AREC[name], FLOOR) == []
        for v in oracle_sums(key, centred, models, bp, ragged):
            assert np.all(np.isfinite(v)) and v[60] < 0


@pytest.mark.parametrize("name", list(LOWER))
def test_lower_edge_families_on_the_oracle(name):
    """the widest band is the build's; the vectors are usable.  Under the vanilla machine these long reads put mass on
    the lower edge cell (or one of the four next to it) of one to four diagonals in a hundred only (the strawMan
    machine: 1 to 26): the model prefers a path of fewer stays.  They are kept for the band they give the kernels -- its
    lower edge moves where the upper-edge reads' upper edge does -- with a bar to match, as the '-out' families are."""
    key, batch, models, bp, ragged = family_case(name)
    assert signal_width(batch, batch["e"]) == LOWER[name] and build_of(LOWER[name]) in (4, 6, 8)
    for v in oracle_sums(key, batch, models, bp, ragged):
        assert np.all(np.isfinite(v)) and v[60] < 0 and np.count_nonzero(v[:60]) == 60
    fr = np.mean([er.edge_fraction(er.vanilla_edge_mass(batch, i, models[it["model"]], bp, ragged), "lower", 0.01,
                                   reach=4, kind="cell") for i, it in enumerate(batch["items"])])
    print(name, "lower-edge fraction", fr)
    assert fr >= 0.01, fr


@pytest.mark.parametrize("name", EDGE_FAMILIES)
def test_wave_edge_families_on_the_oracle(name):
    key, batch, models, bp, ragged = family_case(name)
    f = er.signal_family(name)
    if f["width"] is not None:
        assert signal_width(batch, batch["e"]) == f["width"]
    else:
        assert signal_width(batch, batch["e"]) <= W2
    seen = 0
    for v in oracle_sums(key, batch, models, bp, ragged):
        assert np.all(np.isfinite(v)) and v[60] < 0
        seen += np.count_nonzero(v[:60])
    assert seen > 20


def test_fuzz_cases_stay_sane():
    """the sweep's sixteen vanilla cases (test_fuzz_expectations_machines_gpu.VANILLA), which the fused sweep runs with
    the flag: finite vectors, a negative likelihood, a third of the sums in use; at least three on each fused build and
    two past 184 k-mers, where the batch must leave the fused builds"""
    widths = []
    for c in VANILLA[:N_CASES]:
        batch, models = vanilla_batch(c)
        widths.append(signal_width(batch, c["e"]))
        assert_sane(cached((case_id(c), "e"), lambda: vanilla_oracle(batch, models, bp_of(c), c["ragged"])), case_id(c))
    assert sum(w <= W2 for w in widths) >= 3 and sum(W2 < w <= W3 for w in widths) >= 3, widths
    assert sum(w > W3 for w in widths) >= 2, widths
    assert sum(w <= W2 for w in widths[::4]) >= 2  # rows3: a narrow band on the three-cell build
    assert sum(w <= W3 for w in widths[1::2]) >= 3  # the every-other-window variant on fused builds


# ---------------------------------------------------- zero skip bins ----------------------------------------------------

ZERO = np.zeros(30)
ZERO_BP = (0.01, 30, 10, 20)


def some_bins_zero(seed):
    s = skip_bins(seed)
    s[:5] = 0.0
    return s


def zero_bin_case(name):
    """(key, batch, models, band parameters): 'nan' more k-mers than events under models whose 30 bins are zero;
    'zero' more events than k-mers under the same; 'mixed' the first with an ordinary model on the second read;
    'partial' bins 0-4 (beta and alpha) zero on reads with skips; 'wide-nan' 'nan' at 700 k-mers with a band of 218
    (the four-wave workgroup builds)"""
    key = ("v-zero-bins", name)
    if name in ("nan", "mixed"):
        batch = synth.make_batch(7, 2, 60, 40, anchor_every=10 ** 6)
        bins = [ZERO, ZERO if name == "nan" else skip_bins(1)]
        bp = ZERO_BP
    elif name == "zero":
        batch, bins, bp = synth.make_batch(7, 2, 40, 60, anchor_every=10 ** 6), [ZERO, ZERO], ZERO_BP
    elif name == "partial":
        batch, bins, bp = synth.make_batch(8, 2, 150, 310, anchor_every=30), [some_bins_zero(0), some_bins_zero(1)], \
            (0.01, 60, 10, 20)
    else:
        assert name == "wide-nan"
        batch, bins, bp = synth.make_batch(9, 2, 700, 600, anchor_every=150), [ZERO, ZERO], (0.01, 150, 40, 80)
    models = [o.VanillaModel(m, s, gy) for (m, _, gy), s in zip(batch["models"], bins)]
    return key, batch, models, band_params(*bp)


ZERO_CASES = ["nan", "zero", "mixed", "partial"]


@pytest.mark.parametrize("ragged", [(1, 1), (0, 0)], ids=["r11", "r00"])
def test_zero_bins_on_the_oracle(ragged):
    def vectors(name):
        key, batch, models, bp = zero_bin_case(name)
        return oracle_sums(key + (ragged,), batch, models, bp, ragged), \
            oracle_posteriors(key + (ragged,), batch, models, bp, ragged)

    for name in ("nan", "wide-nan"):
        ref, post = vectors(name)
        for v, r in zip(ref, post):
            assert np.count_nonzero(np.isnan(v[:60])) >= 1 and (np.isnan(v[60]) or v[60] == -np.inf), (name, v[60])
            assert np.any(np.isneginf(r["totals"])) and not np.any(np.isnan(r["totals"]))
    ref, post = vectors("zero")
    for v, r in zip(ref, post):
        assert np.count_nonzero(v[:60] == 0) == 60 and np.isfinite(v[60]) and v[60] < 0
        assert np.all(np.isfinite(r["totals"]))
    ref, _ = vectors("mixed")
    assert np.count_nonzero(np.isnan(ref[0])) == 38 and ref[0][60] == -np.inf
    assert np.all(np.isfinite(ref[1])) and ref[1][60] < 0 and np.count_nonzero(ref[1][:60]) > 20
    ordinary = zero_bin_case("mixed")
    alone = vanilla_oracle(dict(ordinary[1], items=[dict(ordinary[1]["items"][1], model=0)]), ordinary[2][1:],
                           ordinary[3], ragged)
    assert np.array_equal(alone[0], ref[1])  # the ordinary model's sums are its read's alone
    ref, _ = vectors("partial")
    for v in ref:  # no bin is NaN: the ten zeroed bins are exact zeros, most others in use
        assert np.all(np.isfinite(v)) and v[60] < 0
        assert not np.any(v[:5]) and not np.any(v[30:35]) and np.count_nonzero(v[:60]) > 30


def test_zero_bin_cases_reach_the_builds_they_are_for():
    for name in ZERO_CASES:
        _, batch, _, bp = zero_bin_case(name)
        assert signal_width(batch, bp.diagonalExpansion) <= W2
    _, batch, _, bp = zero_bin_case("wide-nan")
    assert build_of(signal_width(batch, bp.diagonalExpansion)) == 4 and batch["items"][0]["lX"] == 700
    assert set(RAGGED) >= {(1, 1), (0, 0)}

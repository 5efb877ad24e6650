"""The cases of tests/test_hdp_four_cells_fused_estep_gpu.py held to what they are there for, on the oracle alone (no
device): which fuzz cases land on four cells per lane by themselves, that they bring several thresholds and a
transition set with the gap Y -> gap X switch, that the low-threshold reads outgrow the four-cell candidate list and
the first pair capacity, and that the host test's read has a band the four-cell build takes."""
from harness import cp
from test_band_edges_machines_gpu import cached
from test_fuzz_expectations_machines_gpu import HDP, W2, W3, W4, hdp_case_batch, hdp_oracle, nhdp, signal_width
from test_hdp_fused_estep_gpu import LOW, low_case, ring_diagonals
from test_hdp_four_cells_fused_estep_gpu import FORCED, FUZZ, HOST_READ, OWN, RESWEEP

__all__ = ["nhdp"]  # (the fuzz file's fixture)

WIDTHS = {2: 190, 3: 221, 4: 196, 12: 199, 14: 193}


def test_the_fuzz_cases_that_land_on_four_cells(nhdp):
    """of the sixteen HDP fuzz cases exactly cases 2, 3, 4, 12 and 14 have a widest band of 185..248 k-mers"""
    assert len(HDP) >= 16
    widths = dict((c["k"], signal_width(hdp_case_batch(c, nhdp), c["e"])) for c in HDP[:16])
    assert sorted(k for k, w in widths.items() if W3 < w <= W4) == OWN == sorted(WIDTHS)
    assert dict((k, widths[k]) for k in OWN) == WIDTHS
    own = [c for c, v in FUZZ if v == "auto"]
    assert [c["k"] for c in own] == OWN and len(own) >= 4
    assert sorted(set(c["thr"] for c in own)) == [0.01, 0.05, 0.5]                 # at least two thresholds
    tsets = set(t for c in own for t in c["tsets"])
    assert "switch" in tsets and "trained" in tsets and "defaults" in tsets         # the _sw and the plain kernels
    forced = [c for c, v in FUZZ if v == "rows4"]
    assert [c["k"] for c in forced] == FORCED and len(forced) >= 2
    assert all(widths[c["k"]] <= W3 for c in forced)                                # narrower: forced there
    swept = set(c["k"] for c, _, _ in RESWEEP)
    assert len(swept) >= 3 and set(r for _, _, r in RESWEEP) == {"1", "2"}
    assert any(t != "defaults" for c, _, _ in RESWEEP for t in c["tsets"])          # one with the switch


def test_the_low_threshold_reads_outgrow_the_four_cell_list(nhdp):
    """overflow: more assignments per read than the list's 4 x 4 x ring diagonals = 4096 records (the read is one
    window); capacity: more than 16 (lX + lY) + 64 for some read"""
    want = dict(overflow=[14034, 12563], capacity=[22973, 23093])
    for name in LOW:
        batch, model, bp = low_case(name, nhdp)
        assert signal_width(batch, 40) <= W2                                        # forced onto four cells
        assert ring_diagonals(batch) == 256
        reads, _ = cached(("hf-low", name, "e"), lambda: hdp_oracle(batch, [model], bp, (1, 1)))
        counts = [len(r["assign"]) for r in reads]
        assert counts == want[name]
        for it, n in zip(batch["items"], counts):
            assert it["lX"] + it["lY"] < bp.minDiagsBetweenTraceBack                # one window
            if name == "overflow":
                assert n > 4 * 4 * ring_diagonals(batch) == 4096
            else:
                assert n > 16 * (it["lX"] + it["lY"]) + 64


def test_the_host_tests_read_has_a_four_cell_band(nhdp):
    from harness import hdp_batch
    seed, lX, every, e = HOST_READ
    batch, _ = hdp_batch(seed, 1, lX, every, nhdp)
    it = batch["items"][0]
    bl, br = cp.band_construct(batch["anchors"], it["lX"], it["lY"], e)
    assert W3 < int(((br - bl) // 2 + 1).max()) == 231 <= W4

"""vanillaAlign --echelon: the reference's performSignalAlignmentP for the echelon machine (vanillaAlign.c:179-255: the
target padded, diagonalCalculationMultiPosteriorMatchProbs) writes the same TSV rows as the host API called directly;
expectations and HMM files are refused under the machine (the reference has no expectation function for it)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import echelon_dp as e
import host_api as h
import test_vanilla_align_cli_gpu as cli


def test_echelon_expectations_are_refused(golden_dir, tmp_path):
    model = os.path.join(golden_dir, "template_median68pA.model")
    r = subprocess.run([cli.EXE, "--echelon", "-T", model, "-C", model, "-q", os.path.join(golden_dir, "ZymoC_ch_1_file1.npRead"),
                        "-r", os.path.join(golden_dir, "ZymoRef.txt"), "-t", str(tmp_path / "t.exp"),
                        "-c", str(tmp_path / "c.exp")], input="", capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "echelon machine has no expectations" in r.stderr


@pytest.mark.gpu
def test_cli_echelon_alignment_matches_the_host_api(golden_dir, zymo_read, template_model, tmp_path):
    L = e.lib()
    pts, ops, cigar = cli._guide(zymo_read, template_model)
    npread, zymo_read = cli._npread_with_forward_complement(golden_dir, zymo_read, tmp_path)
    tsv = str(tmp_path / "out.tsv")
    models = [os.path.join(golden_dir, "template_median68pA.model"),
              os.path.join(golden_dir, "complement_median68pA_pop2.model")]
    cmd = [cli.EXE, "--echelon", "-T", models[0], "-C", models[1], "-q", npread, "-r",
           os.path.join(golden_dir, "ZymoRef.txt"), "-u", tsv, "-L", "zymo_read", "-x", "50"]
    r = subprocess.run(cmd, input=cigar, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "using echelon model" in r.stderr
    got = [l for l in open(tsv).read().split("\n") if l]

    ref = zymo_read["reference"]
    x0, x1, r0 = pts[0][0], pts[-1][0], pts[0][1]
    trimmed = ref[x0:x1]
    rc = "".join({"A": "T", "C": "G", "G": "C", "T": "A"}[c] for c in reversed(trimmed))
    unmapped = h.make_anchor_list(cli._anchors_from_ops(pts, ops))
    filtered = L.filterToRemoveOverlap(unmapped)
    want_tsv = str(tmp_path / "want.tsv")
    counts = []
    for strand, model, params, events, emap, target, rshift in (
            (0, models[0], zymo_read["template_params"], zymo_read["template_events"], zymo_read["template_map"],
             trimmed, x0),
            (1, models[1], zymo_read["complement_params"], zymo_read["complement_events"],
             zymo_read["complement_map"], rc, x1)):
        emap = np.ascontiguousarray(emap, dtype=np.int64)
        ev = np.ascontiguousarray(events, dtype=np.float64).reshape(-1).copy()
        s, end = int(emap[pts[0][1]]), int(emap[pts[-1][1]])
        sm = L.getStateMachineEchelon(model.encode())
        L.emissions_signal_scaleModel(sm, *params)
        remapped = L.nanopore_remapAnchorPairsWithOffset(filtered, emap.ctypes.data_as(C.POINTER(C.c_int64)), r0)
        anchors = L.filterToRemoveOverlap(remapped)
        xbuf = C.create_string_buffer(target.encode())
        sX = L.sequence_construct2(len(target) - 5, C.cast(xbuf, C.c_void_p), h.fn_ptr("sequence_getKmer2"),
                                   h.fn_ptr("sequence_sliceNucleotideSequence2"))
        L.sequence_padSequence(sX)
        sub = ev[3 * s:]
        sY = L.sequence_construct2(end - s, sub.ctypes.data_as(C.c_void_p), h.fn_ptr("sequence_getEvent"),
                                   h.fn_ptr("sequence_sliceEventSequence2"))
        p = L.pairwiseAlignmentBandingParameters_construct()
        p.contents.diagonalExpansion = 50
        pairs = L.getAlignedPairsUsingAnchors(sm, sX, sY, anchors, p,
                                              h.fn_ptr("diagonalCalculationMultiPosteriorMatchProbs"), True, True)
        counts.append(L.stList_length(pairs))
        L.writePosteriorProbs(want_tsv.encode(), b"zymo_read", sm.contents.model.EMISSION_MATCH_PROBS, params[0],
                              params[1], ev.ctypes.data_as(C.POINTER(C.c_double)), target.encode(), True, b"ZYMO",
                              s, rshift, pairs, strand)
        for lst in (pairs, anchors, remapped):
            L.stList_destruct(lst)
        L.sequence_sequenceDestroy(sX)
        L.sequence_sequenceDestroy(sY)
        L.pairwiseAlignmentBandingParameters_destruct(p)
        L.stateMachine_destruct(sm)
    want = [l for l in open(want_tsv).read().split("\n") if l]
    assert counts[0] > 100 and counts[1] > 0
    assert len(got) == len(want) == sum(counts)
    for label in ("t", "c"):
        assert sorted(l for l in got if l.split("\t")[4] == label) == \
            sorted(l for l in want if l.split("\t")[4] == label)

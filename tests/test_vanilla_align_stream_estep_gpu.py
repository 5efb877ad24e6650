"""vanillaAlign --npReadDir --stream --templateExpectations / --complementExpectations: the E-step over a directory of
reads through two expectation streams writes, per strand, the element-wise sum of the files the single-read driver
writes for each read.  Every file is "%f" text (six decimals): a value of the directory's file is half a unit of the
sixth decimal from the sum it rounds, and so is each of the three it is compared with -- (3 + 1) x 0.5e-6 absolute."""
import os
import subprocess

import numpy as np
import pytest

from test_vanilla_align_cli_gpu import EXE, _guide, _npread_with_forward_complement

pytestmark = pytest.mark.gpu

BAR = (3 + 1) * 0.5e-6
NAMES = ["readA", "readB", "readC"]


def _directory(golden_dir, zymo_read, template_model, tmp_path):
    """three names over the shipped read, the second with the short guide (test_vanilla_align_stream_gpu.py's way)"""
    pts, ops, cigar = _guide(zymo_read, template_model)
    npread, _ = _npread_with_forward_complement(golden_dir, zymo_read, tmp_path)
    short_ops, n_x, n_r = [], 0, 0
    for op, k in ops[:len(ops) // 2]:
        short_ops.append((op, k))
        n_x += k if op != "I" else 0
        n_r += k if op != "D" else 0
    short = "cigar: read %d %d + ZYMO %d %d + 100 %s\n" % (pts[0][1], pts[0][1] + n_r, pts[0][0], pts[0][0] + n_x,
                                                            " ".join("%s %d" % o_ for o_ in short_ops))
    reads_dir = tmp_path / "reads"
    reads_dir.mkdir()
    guides = dict(zip(NAMES, [cigar, short, cigar]))
    for name, g in guides.items():
        (reads_dir / (name + ".npRead")).write_text(open(npread).read())
        (reads_dir / (name + ".cigar")).write_text(g)
    return reads_dir, npread, guides


def _common(machine, golden_dir):
    nhdp = os.path.join(golden_dir, "testTemplate.nhdp")
    flags = {"strawMan": ["--strawMan"], "vanilla": [], "sm3Hdp": ["--sm3Hdp", "-v", nhdp, "-w", nhdp]}[machine]
    return [EXE] + flags + ["-T", os.path.join(golden_dir, "template_median68pA.model"), "-C",
                            os.path.join(golden_dir, "complement_median68pA_pop2.model"), "-r",
                            os.path.join(golden_dir, "ZymoRef.txt"), "-x", "50"]


def _lines(path):
    return [line.split() for line in open(path).read().split("\n")]


@pytest.mark.parametrize("machine", ["strawMan", "vanilla", "sm3Hdp"])
def test_the_directorys_files_are_the_sums_of_the_single_read_files(machine, golden_dir, zymo_read, template_model, tmp_path):
    reads_dir, npread, guides = _directory(golden_dir, zymo_read, template_model, tmp_path)
    common = _common(machine, golden_dir)
    alone = {}
    for name in NAMES:
        t, c = str(tmp_path / (name + ".t")), str(tmp_path / (name + ".c"))
        r = subprocess.run(common + ["-q", npread, "-L", name, "-t", t, "-c", c], input=guides[name], capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        alone[name] = (_lines(t), _lines(c))
    t, c = str(tmp_path / "all.t"), str(tmp_path / "all.c")
    r = subprocess.run(common + ["--npReadDir", str(reads_dir), "--stream", "--streamReads", "2", "-t", t, "-c", c],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "SUCCESS" in r.stderr and "0 strands refused" in r.stderr, r.stderr[-2000:]
    for st, path in enumerate((t, c)):
        got = _lines(path)
        per_read = [alone[name][st] for name in NAMES]
        sums = np.array(got[1], float)
        want = sum(np.array(f[1], float) for f in per_read)
        assert sums.shape == want.shape and sums.size == {"strawMan": 10, "vanilla": 61, "sm3Hdp": 10}[machine]
        print(machine, "strand", st, "largest difference of the sums line", np.abs(sums - want).max())
        assert np.abs(sums - want).max() <= BAR and want[:-1].min() >= 3 * 0.0001 - BAR and want[:-1].max() > 1 and want[-1] < 0
        if machine == "strawMan":
            assert got[0] == per_read[0][0] == ["2", "3", "4096"]
            gaps, want_gaps = np.array(got[2], float), sum(np.array(f[2], float) for f in per_read)
            assert gaps.size == 4096 and np.abs(gaps - want_gaps).max() <= BAR and want_gaps.max() > 1
        elif machine == "vanilla":
            assert got[0] == per_read[0][0]
            # the match tables of the first read in name order
            assert got[2] == per_read[0][2] and got[3] == per_read[0][3] and len(got[2]) == 1 + 4096 * 5
        else:
            counts = [int(f[0][3]) for f in per_read]
            assert got[0][:3] == per_read[0][0][:3] and int(got[0][3]) == sum(counts) and min(counts) > 20
            assert len(got[2]) == len(got[3]) == sum(counts)
            assert sorted(zip(got[3], got[2])) == sorted((k, m) for f in per_read for k, m in zip(f[3], f[2]))


def test_without_stream_the_directorys_e_step_is_refused(golden_dir, tmp_path):
    (tmp_path / "reads").mkdir()
    r = subprocess.run(_common("strawMan", golden_dir) + ["--npReadDir", str(tmp_path / "reads"), "-t", str(tmp_path / "t"),
                                                         "-c", str(tmp_path / "c")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--stream" in r.stderr and not os.path.exists(str(tmp_path / "t")), r.stderr
    for flag, text in (("--fourState", "fourState machine has no expectations"), ("--echelon", "echelon machine has no expectations")):
        r = subprocess.run(_common("strawMan", golden_dir) + [flag, "--npReadDir", str(tmp_path / "reads"), "--stream", "-t",
                                                             str(tmp_path / "t"), "-c", str(tmp_path / "c")],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and text in r.stderr, r.stderr

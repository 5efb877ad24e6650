"""vanillaAlign --npReadDir --stream: the directory of reads through the host library's stream, chunk after chunk, must
write what the same directory writes as one batch -- every <name>.tsv and stdout byte for byte."""
import os
import subprocess

import pytest

from test_vanilla_align_cli_gpu import EXE, _guide, _npread_with_forward_complement

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("machine", ["strawMan", "vanilla"])
def test_cli_directory_of_reads_through_the_stream(machine, golden_dir, zymo_read, template_model, tmp_path):
    """the directory of test_cli_directory_of_reads_as_one_batch with five names, two of them with the short guide;
    --streamReads 2 cuts the ten strands into five chunks or more"""
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
    guides = {"readA": cigar, "readB": short, "readC": cigar, "readD": short, "readE": cigar}
    for name, g in guides.items():
        (reads_dir / (name + ".npRead")).write_text(open(npread).read())
        (reads_dir / (name + ".cigar")).write_text(g)
    flags = ["--strawMan"] if machine == "strawMan" else []
    common = ["-T", os.path.join(golden_dir, "template_median68pA.model"), "-C",
              os.path.join(golden_dir, "complement_median68pA_pop2.model"), "-r", os.path.join(golden_dir, "ZymoRef.txt"),
              "-x", "50", "--npReadDir", str(reads_dir)]
    runs = {}
    for how, extra in (("batch", []), ("stream", ["--stream", "--streamReads", "2"])):
        out_dir = tmp_path / how
        out_dir.mkdir()
        r = subprocess.run([EXE] + flags + common + ["--outDir", str(out_dir)] + extra, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        runs[how] = (r, out_dir)
    assert "as one batch" not in runs["stream"][0].stderr and "stream: " in runs["stream"][0].stderr
    assert runs["stream"][0].stdout == runs["batch"][0].stdout and len(runs["batch"][0].stdout.split("\n")) == 6
    for name in guides:
        want = open(str(runs["batch"][1] / (name + ".tsv")), "rb").read()
        got = open(str(runs["stream"][1] / (name + ".tsv")), "rb").read()
        assert got == want and want.count(b"\n") > 100, name

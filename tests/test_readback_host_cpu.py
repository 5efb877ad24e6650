"""The three rules of the readback that need no device (csrc/cpecan_readback_host.h): the verdict of one exponent with
the host libm, the cut of a batch's items into runs for the host threads, the reference's order of the HDP machine's event
assignments.  tests/c/readback_host_test.cpp, which includes that header alone, is built with the address and
undefined-behaviour sanitizers and run as a child process: cases in, results out, the expectations here."""
import math
import os
import random
import shutil
import subprocess

import pytest

from cpecan_load import ROOT

SRC = os.path.join(ROOT, "tests", "c", "readback_host_test.cpp")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined"]
THRESHOLDS = (0.0, 1e-13, 0.01, 0.9)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("readback_host")
    probe = d / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    built = subprocess.run([gxx] + FLAGS + [str(probe), "-o", str(d / "probe")], capture_output=True)
    if built.returncode != 0 or subprocess.run([str(d / "probe")], capture_output=True).returncode != 0:
        pytest.skip("no sanitizer runtime here: an empty program does not build and run with " + " ".join(FLAGS))
    exe = str(d / "readback_host_test")
    subprocess.run([gxx] + FLAGS + ["-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "cpecan-signal_amd", "csrc"),
                                    SRC, "-o", exe], check=True)
    return exe


def ask(program, text):
    r = subprocess.run([program], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]  # (a sanitizer report lands on stderr)
    return r.stdout.splitlines()


def verdict(e, thr):
    p = math.exp(e)
    return -2 if not (p >= thr) else int(math.floor(min(p, 1.0) * 1e7))


def test_verdicts_of_exponents(program):
    rng = random.Random(1401)
    cases = [(thr, rng.uniform(-40.0, 1e-12)) for _ in range(1000) for thr in THRESHOLDS]
    by_hand = [0.0, 3.6e-15, -8.9e-16, -math.inf, math.nan]
    cases += [(thr, e) for e in by_hand for thr in THRESHOLDS]
    got = [int(l) for l in ask(program, "".join("v %s %s\n" % (thr.hex(), e.hex()) for thr, e in cases))]
    assert got == [verdict(e, thr) for thr, e in cases]
    hand = dict(((thr, repr(e)), v) for (thr, e), v in zip(cases, got))
    # exp(0) is 1; exp(3.6e-15) = 1 + 16 ulp is clamped to 1; exp(-8.9e-16) = 1 - 8 ulp, and 1e7 times it still lies
    # below 1e7 (by five of its ulps there)
    assert hand[(0.9, "0.0")] == 10000000 and hand[(0.9, "3.6e-15")] == 10000000 and hand[(0.9, "-8.9e-16")] == 9999999
    # a threshold of 0 keeps a pair of probability 0; a positive one drops it; NaN is below every threshold, 0 too
    assert hand[(0.0, "-inf")] == 0 and all(hand[(thr, "-inf")] == -2 for thr in THRESHOLDS[1:])
    assert all(hand[(thr, "nan")] == -2 for thr in THRESHOLDS)
    assert -2 in got and 0 in got and max(got) == 10000000 and len(set(got)) > 500


def cut_restated(base, n_items, nt):
    total = base[n_items]
    cut = [0]
    for t in range(nt):
        want = total * (t + 1) // nt
        i1 = cut[-1]
        while i1 < n_items and (base[i1 + 1] <= want or t == nt - 1):
            i1 += 1
        cut.append(i1)
    cut[-1] = n_items
    return cut


def prefix(sizes):
    base = [0]
    for s in sizes:
        base.append(base[-1] + s)
    return base


def test_cut_of_items_into_runs(program):
    rng = random.Random(1402)
    cases = [(nt, [0] * 5) for nt in (1, 3, 5)]  # no candidate at all
    for where in (0, 4, 8):  # one item holds every candidate: first, in the middle, last
        cases += [(nt, [300000 if i == where else 0 for i in range(9)]) for nt in (1, 2, 7)]
    cases.append((7, [rng.randrange(0, 5000) for _ in range(7)]))  # as many runs as items
    thousand = [rng.choice((0, 1, rng.randrange(0, 4000), rng.randrange(0, 400000))) for _ in range(1000)]
    cases += [(nt, thousand) for nt in (1, 2, 7, 32)]
    text = "".join("c %d %d %s\n" % (nt, len(s), " ".join(map(str, prefix(s)))) for nt, s in cases)
    got = [[int(v) for v in l.split()] for l in ask(program, text)]
    assert len(got) == len(cases)
    for (nt, sizes), cut in zip(cases, got):
        assert cut == cut_restated(prefix(sizes), len(sizes), nt)
        assert len(cut) == nt + 1 and cut[0] == 0 and cut[-1] == len(sizes)
        assert all(a <= b for a, b in zip(cut, cut[1:]))
    # and the runs of the large case are about even: none holds more than its share plus one item's candidates
    base = prefix(thousand)
    for nt, cut in ((nt, c) for (nt, s), c in zip(cases, got) if s is thousand):
        assert max(base[b] - base[a] for a, b in zip(cut, cut[1:])) <= base[-1] // nt + max(thousand)


def test_order_of_hdp_assignments(program):
    rng = random.Random(1403)
    cases = []
    for n in (0, 1, 2, 1000):
        keys = set()
        while len(keys) < n:  # (window, x, y, from-state): distinct records have distinct places in the order
            keys.add((rng.randrange(3), rng.randrange(40), rng.randrange(60), rng.randrange(3)))
        recs = [(w, x, y, f, -rng.random() * 30.0) for w, x, y, f in keys]
        rng.shuffle(recs)
        cases.append(recs)
    cases.append([(2, 7, 9, 1, -0.5)])  # one record alone: its tag comes off too
    text = "".join("a %d\n" % len(recs) + "".join("%d %d %d %s\n" % (f + 4 * w, x, y, e.hex()) for w, x, y, f, e in recs)
                   for recs in cases)
    lines = ask(program, text)
    assert len(lines) == sum(len(recs) for recs in cases)
    for recs in cases:
        got = [(int(f), int(x), int(y), float.fromhex(e)) for f, x, y, e in (l.split() for l in lines[:len(recs)])]
        lines = lines[len(recs):]
        want = sorted(recs, key=lambda r: (r[0], -(r[1] + r[2]), r[1], r[3]))
        assert got == [(f, x, y, e) for w, x, y, f, e in want]

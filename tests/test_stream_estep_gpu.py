"""The stream in expectation mode (cpecan_stream_open_expectations, include/cpecan_api.h): the struct it adds to holds
the host sum of the single-read E-step calls over the same reads, whatever the chunks -- to the suite's bars for sums
taken in another order (rtol 1e-9 / atol 1e-12, likelihood rtol 1e-12: test_fuzz_expectations_machines_gpu.py,
test_host_api.py); the HDP machine's assignments are those of the calls on each read alone, in their order, tagged;
reads are classed by the kernel an E-step of each alone runs on; the budget holds, a chunk cut in half has added
nothing, and a refused read leaves the struct as it was."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import stream_api as sa
import stream_estep_api as se
from harness import cp
from test_stream_gpu import CLASS_JUMPS, MIXED, _limit_reads

pytestmark = pytest.mark.gpu

_CASES = {}


def case(kind):
    """(machine, reads, parameters, per read: the Target of the single-read call on it alone), once per process"""
    if kind not in _CASES:
        p = sa.params()
        if kind == "hdp":
            sm, _nh, reads = sa.hdp_machine_and_reads(41, [lx for lx, _ in MIXED])
        elif kind == "dna5":
            p.contents.minDiagsBetweenTraceBack = 60
            p.contents.traceBackDiagonals = 10
            sm, reads = sa.dna_machine_and_reads(43, [180, 260, 210, 300])
        else:
            sm, get_x = sa.machine(kind)
            reads = sa.synthetic_reads(41, MIXED, get_x)
        _CASES[kind] = (sm, reads, p, [se.Target(kind).alone(sm, rd, p) for rd in reads])
    return _CASES[kind]


def host_sum(alone):
    total = alone[0].vector()
    for t in alone[1:]:
        total = total + t.vector()
    return total


def all_done_once(out, n, refused=False):
    assert sorted(t for t, _ in out["done"]) == list(range(n)) and all(r == refused for _, r in out["done"]), out["done"]


@pytest.mark.parametrize("kind", ["strawman", "vanilla", "hdp", "dna5"])
def test_the_struct_holds_the_sum_of_the_single_read_calls(kind):
    sm, reads, p, alone = case(kind)
    n = len(reads)
    target = se.Target(kind)
    out = se.run_stream(sm, reads, p, target, maxReadsPerChunk=4, slots=3)
    se.assert_vectors_match(target.vector(), host_sum(alone), kind)
    all_done_once(out, n)
    # (the 5-state machine's four reads are one chunk of four: run below in four chunks as well)
    assert out["n_chunks"] >= (3 if n == 12 else 1) and out["n_refused"] == 0 and len(out["chunks"]) == out["n_chunks"]
    assert sum(c["nReads"] for c in out["chunks"]) == n and all(c["nReads"] <= 4 for c in out["chunks"])
    if n < 12:
        target = se.Target(kind)
        out = se.run_stream(sm, reads, p, target, maxReadsPerChunk=1, slots=3)
        se.assert_vectors_match(target.vector(), host_sum(alone), kind)
        all_done_once(out, n)
        assert out["n_chunks"] == 4 and out["n_refused"] == 0


def test_hdp_assignments_are_those_of_the_reads_alone_in_their_order_and_tagged():
    sm, reads, p, alone = case("hdp")
    tags = [1000 + 7 * i for i in range(12)]
    target = se.Target("hdp")
    out = se.run_stream(sm, reads, p, target, tags=tags, maxReadsPerChunk=4, slots=3)
    assert sorted(t for t, _ in out["done"]) == tags and out["n_refused"] == 0
    got = target.assignments()
    want = {tags[i]: [(tags[i],) + a[1:] for a in t.assignments()] for i, t in enumerate(alone)}
    assert all(a[0] == 0 for t in alone for a in t.assignments())  # (the single-read call's third field: read 0)
    assert sum(len(v) for v in want.values()) == len(got) and len(got) > 600
    assert sorted(got) == sorted(a for v in want.values() for a in v)
    for tag in tags:  # a read's own assignments: the alone call's, in its order
        assert [a for a in got if a[0] == tag] == want[tag], tag
    assert {a[0] for a in got} == set(tags)


def _kernels(chunks):
    return sorted({(c["kernel"], c["wave"], c["rows"]) for c in chunks})


def test_reads_are_classed_by_the_kernel_an_e_step_of_each_runs_on_alone():
    p = sa.params()
    sm, get_x = sa.machine("strawman")
    reads = sa.synthetic_reads(45, [(360, 720)] * 12, get_x, jumps=CLASS_JUMPS)
    # what batch creation answers for an E-step of each read alone, under the flags the host library's create call passes
    want = []
    for rd in reads:
        w, step = cp.band_extent(rd.anchors, rd.lX, rd.lY, 20)
        d = cp.plan_dispatch(cp.MACHINE_STRAWMAN, cp.MODE_EXPECTATIONS, cp.KERNEL_AUTO, cp.FLAG_SMALL_FOOTPRINT, w, step)
        want.append((d["kernel"], d["wave"], d["rows"]) if d["kernel"] == sa.KERNEL_SYSTOLIC else (sa.KERNEL_GENERAL, 0, 0))
    assert len(set(want)) >= 2, want
    alone = [se.Target("strawman").alone(sm, rd, p) for rd in reads]
    target = se.Target("strawman")
    out = se.run_stream(sm, reads, p, target, slots=3)
    all_done_once(out, 12)
    assert _kernels(out["chunks"]) == sorted(set(want))
    # no chunk mixes classes: one chunk per class here, of that class's number of reads
    assert sorted(c["nReads"] for c in out["chunks"]) == sorted(want.count(k) for k in set(want))
    se.assert_vectors_match(target.vector(), host_sum(alone), "grouped")
    one = se.Target("strawman")
    out1 = se.run_stream(sm, reads, p, one, slots=3, oneClass=1)
    all_done_once(out1, 12)
    assert len(_kernels(out1["chunks"])) == 1 and [t for t, _ in out1["done"]] == list(range(12))
    se.assert_vectors_match(one.vector(), host_sum(alone), "oneClass")


@pytest.fixture(scope="module")
def limit():
    case16, sm, reads = _limit_reads()
    p = sa.params(expansion=int(case16["bp"].diagonalExpansion), min_diags=int(case16["bp"].minDiagsBetweenTraceBack))
    return case16["L"], sm, reads, p, host_sum([se.Target("strawman").alone(sm, rd, p) for rd in reads])


def test_the_budget_holds_and_a_halved_chunk_adds_nothing_twice(limit):
    """L is the posterior test's own limit (stream_api.limit_case: what a 4-read posterior batch needs, with the
    allocator's slack).  The budget starts at 2 L and is lowered until a chunk is cut in half; at every budget tried
    the peak and the chunks hold it and the sums are the single-read calls'."""
    L, sm, reads, p, want = limit
    halved = False
    for budget in (2 * L, L, L // 2):
        target = se.Target("strawman")
        out = se.run_stream(sm, reads, p, target, slots=2, deviceBytes=budget)
        print("budget %d: %d chunks %r, peak %d, refused %d" % (
            budget, out["n_chunks"], [(c["nReads"], c["halvings"], c["deviceBytes"]) for c in out["chunks"]], out["peak"],
            out["n_refused"]))
        assert out["peak"] <= budget and all(c["deviceBytes"] <= budget // 2 for c in out["chunks"])
        all_done_once(out, 16)
        assert out["n_refused"] == 0
        se.assert_vectors_match(target.vector(), want, budget)
        halved = any(c["halvings"] > 0 for c in out["chunks"])
        if halved:
            break
    assert halved


def test_a_budget_below_one_read_refuses_every_read_and_leaves_the_struct_as_it_was(limit):
    _L, sm, reads, p, _want = limit
    target = se.Target("strawman")
    pattern = np.random.default_rng(7).integers(0, 256, C.sizeof(target.obj), dtype=np.uint8).tobytes()
    C.memmove(C.addressof(target.obj), pattern, len(pattern))
    out = se.run_stream(sm, reads, p, target, slots=2, deviceBytes=2 * 4096)
    all_done_once(out, 16, refused=True)
    assert len(out["done"]) == 16 and out["n_refused"] == 16 and out["n_chunks"] == 0
    assert C.string_at(C.addressof(target.obj), C.sizeof(target.obj)) == pattern


def test_a_four_state_read_is_refused_by_submit():
    """(in a child process: the refusal ends the process, as the batch call's does)"""
    code = ("import stream_api as sa, stream_estep_api as se\n"
            "p = sa.params(); sm, gx = sa.machine('sm4')\n"
            "reads = sa.synthetic_reads(1, [(100, 200)], gx)\n"
            "se.run_stream(sm, reads, p, se.Target('strawman'), slots=2)\n")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(sys.path))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 1 and "the 4-state machine has no expectations" in r.stderr, (r.returncode, r.stderr[-1000:])

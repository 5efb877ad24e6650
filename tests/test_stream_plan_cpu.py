"""The chunking rule of the stream (csrc/host/cpecan_stream_plan.c) as a pure function, through its exported test hook
and from a stand-alone C program; and the stream's names in the header and the library.  No device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import host_api as h
import stream_api as sa
from cpecan_load import ROOT


def check_plan(classes, cells, max_reads, budget, one_class):
    chunk_of, rank_of, n_chunks = sa.plan_chunks(classes, cells, max_reads, budget, one_class)
    n = len(classes)
    assert chunk_of.min(initial=0) >= 0 and chunk_of.max(initial=-1) < n_chunks  # every read in exactly one chunk
    assert set(chunk_of.tolist()) == set(range(n_chunks))                       # and no chunk without a read
    last_closed = -1
    for c in range(n_chunks):
        members = np.flatnonzero(chunk_of == c)  # (in submission order)
        assert rank_of[members].tolist() == list(range(len(members)))  # the chunk holds them in that order
        if not one_class:
            assert len(set(classes[members].tolist())) == 1
        assert len(members) <= max_reads
        assert len(members) == 1 or cells[members].sum() <= budget
        last_closed = max(last_closed, members[-1])
    if one_class:  # chunks in submission order: consecutive runs of reads
        assert np.all(np.diff(chunk_of) >= 0)
    else:
        # a group closes when its class's next read does not fit: that read is then the first of a later chunk
        for c in range(n_chunks):
            members = np.flatnonzero(chunk_of == c)
            later = np.flatnonzero((classes == classes[members[0]]) & (np.arange(n) > members[-1]))
            if later.size:
                nxt = later[0]
                assert chunk_of[nxt] > c
                assert len(members) + 1 > max_reads or cells[members].sum() + cells[nxt] > budget
    return n_chunks


def test_chunking_rule_on_random_sequences():
    rng = np.random.default_rng(30)
    for case in range(300):
        n = int(rng.integers(0, 200))
        classes = rng.integers(0, int(rng.integers(1, 6)), n).astype(np.int32)
        cells = rng.integers(1, 1000, n).astype(np.int64)
        check_plan(classes, cells, int(rng.integers(1, 13)), int(rng.integers(1, 6000)), case % 3 == 0)


def test_chunking_rule_named_cases():
    # three classes interleaved, four reads each, room for two: six chunks of two, closed as their third read arrives
    classes = np.array([0, 1, 2] * 4, np.int32)
    cells = np.full(12, 10, np.int64)
    chunk_of, rank_of, n = sa.plan_chunks(classes, cells, 2, 10 ** 9)
    assert n == 6 and chunk_of.tolist() == [0, 1, 2, 0, 1, 2, 3, 4, 5, 3, 4, 5]
    assert rank_of.tolist() == [0, 0, 0, 1, 1, 1, 0, 0, 0, 1, 1, 1]
    # the same with one class: submission order
    chunk_of, rank_of, n = sa.plan_chunks(classes, cells, 2, 10 ** 9, one_class=True)
    assert n == 6 and chunk_of.tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5] and rank_of.tolist() == [0, 1] * 6
    # the cell budget closes a group, and a read larger than the budget still gets a chunk of its own
    chunk_of, rank_of, n = sa.plan_chunks(np.zeros(5, np.int32), np.array([40, 40, 40, 500, 10], np.int64), 100, 100)
    assert n == 4 and chunk_of.tolist() == [0, 0, 1, 2, 3] and rank_of.tolist() == [0, 1, 0, 0, 0]


def test_chunking_rule_from_a_stand_alone_c_program(tmp_path):
    """tests/c/stream_plan_test.c with cpecan_stream_plan.c, under the address and undefined-behaviour sanitizers where
    gcc links them (a plain build otherwise)"""
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = [os.path.join(ROOT, "tests", "c", "stream_plan_test.c"),
           os.path.join(ROOT, "cpecan-signal_amd", "csrc", "host", "cpecan_stream_plan.c")]
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cpecan-signal_amd", "csrc", "host")]
    exe = str(tmp_path / "stream_plan_test")
    base = [gcc, "-std=gnu99", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + inc
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + src + ["-o", exe],
                         capture_output=True, text=True)
    if san.returncode != 0:
        # a plain build only where the sanitizers' runtime libraries are not there to link; anything else is a failure
        missing = re.search(r"cannot find -l(asan|ubsan)|cannot find .*lib(asan|ubsan)|unrecognized .*-fsanitize", san.stderr)
        assert missing, san.stderr
        subprocess.run(base + src + ["-o", exe], check=True)
    print("stream_plan_test built %s the sanitizers" % ("with" if san.returncode == 0 else "WITHOUT"))
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "0 failures" in run.stdout


def test_stream_and_memory_names_are_declared_exported_and_bound():
    api = open(os.path.join(ROOT, "include", "cpecan_api.h")).read()
    hip = open(os.path.join(ROOT, "include", "cpecan_hip.h")).read()
    L = C.CDLL(h.LIB_PATH)
    for name in sa.STREAM_EXPORTS:
        assert re.search(r"\b%s\s*\(" % name, api) and hasattr(L, name), name
    from cpecan_load import binding
    cp = binding()
    hl = C.CDLL(cp.LIB_PATH)
    for name in ("cpecan_hip_batch_device_bytes", "cpecan_hip_ctx_memory", "cpecan_hip_ctx_set_memory_limit",
                 "cpecan_band_extent"):
        assert re.search(r"\b%s\s*\(" % name, hip) and name in cp.EXPORTS and hasattr(hl, name), name
    assert cp.ELIMIT == -6 and re.search(r"#define CPECAN_ELIMIT \(-6\)", hip)
    assert all(hasattr(cp.Context, m) for m in ("set_memory_limit", "memory")) and hasattr(cp.Batch, "device_bytes")

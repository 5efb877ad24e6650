"""CPU-only checks of bench.py's host-side pieces: the all-core CPU baseline (a pool of forked oracle workers)
agrees with single calls, and the command line keeps the contract's flags."""
import os
import subprocess
import sys

import numpy as np

import synth
from harness import band_params, run_oracle_item

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_all_core_cpu_baseline_counts_the_same_cells():
    batch = synth.make_batch(3, 6, 200, 410, anchor_every=50)
    out = bench.cpu_all_cores(batch, 100, 3, 2)
    cells = sum(run_oracle_item(batch, i, band_params(0.01, 1000, 40, 100), (1, 1))["cells"] for i in range(6))
    assert out["cores"] == 2 and out["kind"] == "port" and out["unit"] == "Gcells/s"
    assert out["cells"] == cells and out["value"] > 0


def test_gpus_2_starts_its_own_two_ranks():
    """`python bench.py --gpus 2` from a plain command line: the process starts two workers itself (one per rank,
    torch.distributed.run on 127.0.0.1); --rehearse keeps them off the GPU (gloo, host band geometry as the step), so
    the plumbing -- rendezvous, shard by rank, barrier, max-over-ranks time, summed cells, ONE JSON line from rank 0 --
    runs here."""
    import json
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--rehearse", "--reads", "6", "--events",
           "400", "--kmers", "200", "--steps", "2", "--warmup", "1", "--master-port", str(29500 + os.getpid() % 2000)]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 2 and out["scaling"] == "weak" and out["value"] is None
    assert "REHEARSAL" in out["data"]
    # every rank has its own reads (seeded by rank): the all-rank sum is rank 0's cells plus another rank's
    one = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--rehearse", "--reads", "6",
                          "--events", "400", "--kmers", "200", "--steps", "1", "--warmup", "0"],
                         capture_output=True, text=True, env=env, timeout=600)
    solo = json.loads([l for l in one.stdout.splitlines() if l.startswith("{")][0])
    assert solo["n_gpus"] == 1 and solo["config"]["cells_rank0"] == out["config"]["cells_rank0"]
    assert out["config"]["cells_all_ranks"] > out["config"]["cells_rank0"] > 0
    assert out["config"]["cells_all_ranks"] != 2 * out["config"]["cells_rank0"]


def test_command_line_contract():
    h = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True)
    assert h.returncode == 0
    for flag in ("--gpus", "--steps", "--warmup", "--mode", "--inflight", "--single-steps", "--full"):
        assert flag in h.stdout


def test_only_full_runs_what_the_headline_does_not_need():
    """a plain run: no CPU baseline, no oracle check, no single-batch measurement, whatever their sizes say; --full
    runs them at the sizes given"""
    for argv in ([], ["--mode", "em"], ["--cpu-reads", "5", "--check", "3", "--single-steps", "4"]):
        a = bench.parse_args(argv)
        assert not a.full and (a.cpu_reads, a.check, a.single_steps) == (0, 0, 0), argv
    a = bench.parse_args(["--full"])
    assert (a.cpu_reads, a.check, a.single_steps) == (60, 2, 12)
    a = bench.parse_args(["--full", "--cpu-reads", "5", "--check", "0", "--single-steps", "4"])
    assert (a.cpu_reads, a.check, a.single_steps) == (5, 0, 4)


def test_steps_and_warmup_are_what_the_command_line_says():
    assert (bench.parse_args([]).steps, bench.parse_args([]).warmup) == (20, 3)
    a = bench.parse_args(["--mode", "hdp"])
    assert (a.steps, a.warmup) == (5, 1)
    for argv in (["--mode", "hdp", "--steps=7", "--warmup=2"], ["--mode", "hdp", "--steps", "7", "--warmup", "2"],
                 ["--steps", "7", "--warmup", "2"]):
        a = bench.parse_args(argv)
        assert (a.steps, a.warmup) == (7, 2), argv


class _FakeBatch:
    """the three result calls of binding.Batch that dump_outputs uses, on made-up per-read results"""

    def __init__(self, n, pairs_per_read):
        rng = np.random.default_rng(7)
        self.np = np.full(n, pairs_per_read, np.int64)
        self.nt = rng.integers(0, 5, n)
        self.tri = [rng.integers(0, 10 ** 7, (pairs_per_read, 3)) for _ in range(n)]
        self.lp = [rng.standard_normal(pairs_per_read) for _ in range(n)]
        self.tot = [(rng.integers(0, 10 ** 4, k), rng.standard_normal(k)) for k in self.nt]

    def counts(self):
        return self.np, self.nt, 10 * self.np

    def pairs(self, i, n):
        assert n == self.np[i]
        return self.tri[i], self.lp[i]

    def totals(self, i, n):
        assert n == self.nt[i]
        return self.tot[i]


def test_dump_outputs_writes_float64_arrays_of_a_fixed_sample(tmp_path):
    fb = _FakeBatch(300, 40)
    bench.dump_outputs(str(tmp_path / "a"), fb)
    bench.dump_outputs(str(tmp_path / "b"), fb)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["counts.npy", "pairs.npy", "pairs_logp.npy", "sample_reads.npy", "totals.npy"]
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float64 and np.array_equal(a, b), n
    reads = np.load(tmp_path / "a" / "sample_reads.npy").astype(int)
    assert len(reads) == 128 and np.all(np.diff(reads) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "counts.npy")[:, 0], fb.np)
    pairs = np.load(tmp_path / "a" / "pairs.npy")
    assert np.array_equal(pairs[:, 1:], np.concatenate([fb.tri[i] for i in reads]))
    assert np.array_equal(pairs[:, 0], np.repeat(reads, 40))
    assert np.array_equal(np.load(tmp_path / "a" / "pairs_logp.npy"), np.concatenate([fb.lp[i] for i in reads]))
    totals = np.load(tmp_path / "a" / "totals.npy")
    assert np.array_equal(totals[:, 2], np.concatenate([fb.tot[i][1] for i in reads]))


def test_dump_outputs_stays_within_its_budget(tmp_path):
    fb = _FakeBatch(50, 1000)
    bench.dump_outputs(str(tmp_path), fb, budget=200000)
    size = sum(os.path.getsize(tmp_path / n) for n in os.listdir(tmp_path))
    reads = np.load(tmp_path / "sample_reads.npy").astype(int)
    assert size <= 200000 + 4096 and 0 < len(reads) < 50
    assert len(np.load(tmp_path / "pairs.npy")) == 1000 * len(reads)

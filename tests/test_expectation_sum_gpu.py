"""cpecan_hip_batch_sum_expectations: a batch's per-model blocks of Baum-Welch sums added on the device, in ascending
model id from block 0's value on.  The order is the contract, so there is no tolerance: the call's answer equals, bit
for bit (a NaN for a NaN), the left-to-right host sum of what cpecan_hip_batch_fetch_expectations returns for ids
0 .. n - 1, and asking twice gives the same bytes.

Shapes: tiny reads (about 40 k-mers x 80 events) with a model each.  1, 3 and 257 models put the model loop below, at
and far past the kernel's eight loads in flight (257 = 1 + 32 * 8: no remainder; 3: the remainder loop alone); the
strawMan machine's 4106 doubles need 17 blocks of 256 threads, the last one partly idle; the other machines' 61, 10
and 106 doubles fit one partly idle block."""
import os
import subprocess
import sys

import numpy as np
import pytest

import expectation_sum_cases as ec
import pyoracle as o
from harness import cp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = cp.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def nhdp(golden_dir):
    return o.load_nhdp(os.path.join(golden_dir, "testTemplate.nhdp"))


def check(b, n_models, length):
    b.run()
    b.sync()
    want, got, again = ec.fetched_and_summed(b, n_models)
    assert want.shape == (length,) and got.shape == (length,)
    assert np.array_equal(got, want, equal_nan=True), np.flatnonzero(got != want)[:10]
    assert got.tobytes() == again.tobytes()
    assert np.count_nonzero(want) >= 3 and want[-1] < 0  # (sums and likelihood of a run, not a cleared buffer)
    return got


@pytest.mark.parametrize("n_models", [1, 3, 257])
@pytest.mark.parametrize("kind", ["strawman", "vanilla"])
def test_signal_batches_with_a_model_per_read(ctx, kind, n_models):
    b = ec.signal_batch(ctx, kind, n_models)
    if kind == "strawman":
        assert b.info()["fused_expectations"] == 1, b.info()  # (what AUTO gives a narrow band: the wave kernels)
    check(b, n_models, cp.EXPECTATION_LEN if kind == "strawman" else cp.EXPECTATIONV_LEN)
    b.close()


@pytest.mark.parametrize("n_models", [1, 2])
def test_hdp_batches(ctx, nhdp, n_models):
    b = ec.hdp_estep_batch(ctx, nhdp, n_models)
    check(b, n_models, cp.EXPECTATIONH_LEN)
    b.close()


@pytest.mark.parametrize("n_models", [1, 2])
def test_dna_batches(ctx, n_models):
    b = ec.dna_estep_batch(ctx, n_models)
    check(b, n_models, cp.EXPECTATION5_LEN)
    b.close()


def test_the_ring_path_fills_the_blocks_as_well():
    """CPECAN_EXPECT_FUSED=0 is read when a batch is created, per process in the tests' way: the three-model strawMan
    case in a child process on the ring of backward cells (the parametrised test above ran it on the fused pass)"""
    env = dict(os.environ, CPECAN_EXPECT_FUSED="0")
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, ec.__file__], env=env, capture_output=True,
                       text=True, timeout=400)
    assert r.returncode == 0 and "fused_expectations 0" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])


def test_a_posterior_batch_is_refused(ctx):
    import synth
    from harness import band_params, make_items
    data = synth.make_batch(311, 1, ec.LX, ec.LY, anchor_every=ec.EVERY)
    ctx.models_clear()
    ctx.models_create([(cp.NANOPORE_TRANSITIONS,) + tuple(data["models"][0])])
    b = cp.Batch(ctx, make_items(data, (1, 1)), data["x_chars"], data["events"], data["anchors"], band_params(*ec.BP))
    b.run()
    b.sync()
    with pytest.raises(cp.CpecanError) as e:
        b.sum_expectations()
    assert e.value.code == cp.EINVAL
    b.close()


def test_the_memory_limit_refuses_the_buffer_and_the_call_can_be_made_again():
    c = cp.Context(0)
    b = ec.signal_batch(c, "strawman", 3)
    b.run()
    b.sync()
    want = ec.left_to_right([b.expectations(k) for k in range(3)])
    held = b.device_bytes()
    c.set_memory_limit(c.memory()["live"])
    with pytest.raises(cp.CpecanError) as e:
        b.sum_expectations()
    assert e.value.code == cp.ELIMIT and b.device_bytes() == held
    c.set_memory_limit(0)
    got = b.sum_expectations()
    assert np.array_equal(got, want, equal_nan=True)
    assert held < b.device_bytes() <= held + 2 * 8 * cp.EXPECTATION_LEN + 4096  # the result buffer, on the batch's account
    b.close()
    c.close()

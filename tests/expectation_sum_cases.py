"""The E-step batches of test_expectation_sum_gpu.py: tiny reads (about 40 k-mers x 80 events) with a model per read,
for each of the four machines that have an E-step, and what cpecan_hip_batch_sum_expectations is held to: the
left-to-right host sum of cpecan_hip_batch_fetch_expectations over ids 0 .. n - 1.

Run as a program it is that test's child process: the strawMan case of three models under whatever environment the
parent set (CPECAN_EXPECT_FUSED=0: the ring of backward cells instead of the sums inside the sweep back; the switch is
read when a batch is created), exit status 0 where the device sum equals the host sum bit for bit, with the pass the
batch took on stdout."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [q for q in (HERE, os.path.join(os.path.dirname(HERE), "oracle")) if q not in sys.path]
import pyoracle as o  # noqa: E402
import synth  # noqa: E402
from harness import band_params, cp, hdp_batch, make_items, with_gap_switch  # noqa: E402

LX, LY, EVERY = 40, 80, 10
BP = (0.01, 60, 10, 20)  # threshold, minDiagsBetweenTraceBack, traceBackDiagonals, diagonalExpansion


def left_to_right(blocks):
    """((e[0] + e[1]) + e[2]) + ...: one IEEE addition per element and model, in model order, from block 0's value"""
    acc = np.array(blocks[0], np.float64, copy=True)
    for e in blocks[1:]:
        acc = acc + e
    return acc


def signal_batch(ctx, kind, n_models, flags=0):
    """a strawMan or vanilla E-step batch of n_models reads, each with the pore model scaled for it on the device"""
    data = synth.make_batch(310 + n_models, n_models, LX, LY, anchor_every=EVERY)
    match, gap_x, gap_y = data["base_model"]
    ctx.models_clear()
    bp = band_params(*BP)
    if kind == "strawman":
        ids = ctx.models_create_scaled((cp.NANOPORE_TRANSITIONS, match, gap_x, gap_y), data["scalings"])
        b = cp.Batch(ctx, make_items(data, (1, 1)), data["x_chars"], data["events"], data["anchors"], bp,
                     cp.MODE_EXPECTATIONS, cp.KERNEL_AUTO, flags)
    else:
        skip = np.sort(np.random.default_rng(5).uniform(0.05, 0.4, 30))[::-1].copy()
        base = o.VanillaModel(match, skip, gap_y)
        ids = ctx.modelsv_create_scaled((base.scalars, base.match, base.skip, base.gap_y), data["scalings"])
        b = cp.Batch(ctx, make_items(data, (1, 1)), data["x_chars"], data["events"], data["anchors"], bp,
                     flags=cp.FLAG_EXPECTATIONS | flags, vanilla=True)
    assert list(ids) == list(range(n_models))
    return b


def hdp_estep_batch(ctx, nhdp, n_models):
    """two reads per model of the shipped HDP, the models' transitions apart"""
    data, _ = hdp_batch(77, 2 * n_models, LX, EVERY, nhdp)
    data = dict(data, items=[dict(it, model=i % n_models) for i, it in enumerate(data["items"])])
    ts = [cp.NANOPORE_TRANSITIONS, with_gap_switch(cp.NANOPORE_TRANSITIONS, 0.05)][:n_models]
    ctx.models_clear()
    ids = ctx.modelsh_create([(t, nhdp["alphabet"], nhdp["grid"], nhdp["y"], nhdp["slope"], nhdp["kmer_row"])
                              for t in ts])
    assert list(ids) == list(range(n_models))
    return cp.Batch(ctx, make_items(data, (1, 1)), data["x_chars"], data["events"], data["anchors"],
                    band_params(0.05, 60, 10, 20), flags=cp.FLAG_EXPECTATIONS, hdp=True)


def dna_estep_batch(ctx, n_models):
    """two pairs of sequences of 60 to 90 bases per model of the 5-state machine, the second model's tables apart"""
    rng = np.random.default_rng(4500)
    d = o.Sm5Model()
    tables = [(list(d.c.t), d.match.copy(), d.gx.copy(), d.gy.copy()),
              (list(d.c.t), d.match.copy(), np.log([0.3, 0.2, 0.2, 0.3]), np.log([0.2, 0.3, 0.3, 0.2]))][:n_models]
    ctx.models_clear()
    ids = ctx.models5_create(tables)
    assert list(ids) == list(range(n_models))
    n = 2 * n_models
    items = np.zeros(n, cp.ITEM_DTYPE)
    xs = ys = ""
    for i in range(n):
        x = "".join(rng.choice(list("ACGT"), 60 + 10 * i))
        y = "".join(ch if rng.random() > 0.15 else rng.choice(list("ACGT")) for ch in x)
        items[i] = (len(xs), len(x), len(ys), len(y), 0, 0, ids[i % n_models], 1, 1, 0)
        xs += x
        ys += y
    return cp.Batch(ctx, items, xs, None, np.zeros((0, 2), np.int64), band_params(0.01, 40, 8, 10),
                    flags=cp.FLAG_EXPECTATIONS, y_chars=ys)


def fetched_and_summed(b, n_models):
    """(left-to-right host sum of the fetched blocks, the device's sum, the device's sum asked for again) of a batch
    that has run"""
    want = left_to_right([b.expectations(k) for k in range(n_models)])
    return want, b.sum_expectations(), b.sum_expectations()


def main():
    ctx = cp.Context(0)
    b = signal_batch(ctx, "strawman", 3)
    b.run()
    b.sync()
    want, got, again = fetched_and_summed(b, 3)
    print("fused_expectations %d" % b.info()["fused_expectations"])
    ok = np.array_equal(got, want, equal_nan=True) and got.tobytes() == again.tobytes() and np.count_nonzero(want) > 50
    b.close()
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

"""Child process of test_readback_gpu.py's test of CPECAN_HOST_FINALISE and CPECAN_PACK_LATER (both read once per
process): a fixed list of batches under whatever the parent set, their triples, exponents, totals and counts written
to the .npz file named on the command line.  runs() is the list; the parent compares the files with each other and
with the oracle's expected values (expected())."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(os.path.dirname(HERE), "oracle")]
import readback_cases as rc  # noqa: E402
from harness import band_params  # noqa: E402


def runs():
    """[(name, batch, band parameters, [the oracle's threshold-0 result per item])]"""
    shape = rc.strawman_shape()
    refs0 = rc.refs_at_zero("strawman-child", rc.sm3_models(shape["batch"]), shape)
    cases = rc.threshold_cases(refs0[0])
    out = [("threshold-%d" % j, shape["batch"], rc.shape_bp(shape, cases[j][2]), refs0) for j in (0, 2, 5)]
    fb, frefs, _ = rc.floor_batch()
    out.append(("floor", fb, band_params(0.01, **rc.FLOOR_BP), frefs))
    sb, names = rc.compose(rc.SMALL_OVER)
    out.append(("over-capacity", sb, band_params(0.0, **rc.CAP_BP), [rc.cap_read(n)["ref0"] for n in names]))
    # threshold 0 emits every cell of the band: more than the first pair allocation, so the batch is run again
    for it, r in zip(shape["batch"]["items"], refs0):
        assert len(r["triples"]) > rc.first_pair_allocation(it["lX"], it["lY"]), len(r["triples"])
    out.append(("re-run", shape["batch"], rc.shape_bp(shape, 0.0), refs0))
    return out


def expected(run):
    name, batch, bp, refs0 = run
    return [rc.expected_at(r, bp.threshold) for r in refs0]


def main(path):
    from harness import batch_results, cp, make_items
    ctx = cp.Context(0)
    arrays = {}

    def keep(name, res):
        for i, g in enumerate(res):
            for key in ("triples", "logp", "totals_xay", "totals"):
                arrays["%s/%d/%s" % (name, i, key)] = np.asarray(g[key])
            arrays["%s/%d/cells" % (name, i)] = np.array([g["cells"]], np.int64)
    all_runs = runs()
    for name, batch, bp, _ in all_runs:
        ctx.models_clear()
        ctx.models_create([(cp.NANOPORE_TRANSITIONS, m, gx, gy) for m, gx, gy in batch["models"]])
        b = cp.Batch(ctx, make_items(batch), batch["x_chars"], batch["events"], batch["anchors"], bp)
        b.run()
        b.sync()
        keep(name, batch_results(b))
        if name == "threshold-0":  # the same batch run twice, read after each run
            b.run()
            b.sync()
            keep("twice", batch_results(b))
        b.close()
    ctx.close()
    np.savez(path, **arrays)


if __name__ == "__main__":
    main(sys.argv[1])

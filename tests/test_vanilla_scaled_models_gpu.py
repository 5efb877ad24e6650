"""Vanilla signal machine: per-read models scaled on the device (cpecan_hip_modelsv_create_scaled), the table that
lives on the device only, the skip bins rewritten in place (cpecan_hip_modelsv_set_skip_probs) and the persistent
E-step built on them (em.PersistentVanillaEStep).

Tables are compared bit for bit with cpecan_hip_modelsv_create on tables scaled on the host in numpy with the
operations of emissions_signal_scaleModel (impl/stateMachine.c:631-651), one IEEE operation each and in its order
(synth.scale_model): both sides do the same IEEE operations and the same libm calls, so there is no tolerance.
Expectations are compared to 1e-9 relative, the standing tolerance for sums taken in another order and with the
device's exp; posterior pairs, exponents and totals exactly."""
import os

import numpy as np
import pytest

import pyoracle as o
import synth
from cpecan_load import em
from harness import assert_same_pairs, band_params, batch_results, cp, orc_params
from test_vanilla_gpu import skip_bins

pytestmark = pytest.mark.gpu

# stateMachine3Vanilla_setStrandTransitionsToDefaults: (m_to_y_not_x, e_to_e) of the template and the complement strand
FUDGE = ((float(np.float32(0.17)), float(np.float32(0.55))), (float(np.float32(0.14)), float(np.float32(0.49))))
STRIDE = 160 + 4097 * 12
BINS = slice(8, 8 + 150)


def scalings(zymo_read):
    rng = np.random.default_rng(11)
    rnd = np.column_stack([rng.uniform(0.9, 1.1, 3), rng.uniform(-6, 6, 3), rng.uniform(0.8, 1.3, 3),
                           rng.uniform(0.8, 1.3, 3), rng.uniform(0.7, 1.4, 3)])
    return np.vstack([
        [1.0, 0.0, 1.0, 1.0, 1.0],
        zymo_read["template_params"],
        zymo_read["complement_params"],
        [1.0, 0.0, 0.0, 1.0, 1.0],            # level sd 0: K = -inf
        [1.0, 0.0, 1.0, 1.0, 0.0],            # noise lambda 0: its log = -inf
        [1.0, 0.0, 1e-310, 1.0, 1e-320],      # level sd and noise lambda subnormal
        rnd,
    ])


def vanilla(match, skip, gap_y, strand=0):
    return o.VanillaModel(match, skip, gap_y, *FUDGE[strand])


def as_tuple(m, match=None, skip=None):
    return (m.scalars, m.match if match is None else match, m.skip if skip is None else skip, m.gap_y)


def host_scaled(m, sc, skip=None):
    """the model's tuple with its match table scaled on the host"""
    with np.errstate(all="ignore"):  # (the noise sd scale_model also takes, which no vanilla row holds, may overflow)
        return as_tuple(m, synth.scale_model(m.match, *[float(v) for v in sc]), skip)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_same_bits(got, want, what=""):
    assert got.size == want.size == STRIDE
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, (what, bad[:5], got[bad[:5]], want[bad[:5]])


def source_model(source, golden_dir):
    if source == "synthetic":
        match, _, gap_y = synth.synthetic_pore_model()
        return vanilla(match, skip_bins(3), gap_y, 0)
    strand = 0 if source.startswith("template") else 1
    match, skip, gap_y = o.load_pore_model(os.path.join(golden_dir, source + ".model"))
    return vanilla(match, skip, gap_y, strand)


@pytest.mark.parametrize("source", ["synthetic", "template_median68pA", "complement_median68pA_pop2"])
def test_device_blocks_are_bit_identical(source, golden_dir, zymo_read):
    m = source_model(source, golden_dir)
    S = scalings(zymo_read)
    assert len(S) >= 5
    ctx = cp.Context(0)
    ids = ctx.modelsv_create_scaled(as_tuple(m), S)
    assert list(ids) == list(range(len(S)))
    got = [ctx.modelsv_download(i) for i in ids]
    ctx.models_clear()
    ids = ctx.modelsv_create([host_scaled(m, sc) for sc in S])
    assert list(ids) == list(range(len(S)))
    for i, sc in zip(ids, S):
        assert_same_bits(got[i], ctx.modelsv_download(i), sc)
    # the cases are what they are meant to be: scaling moved the match half, the degenerate ones hit -inf and subnormals
    rows = [g[160:].reshape(4097, 12) for g in got]
    assert not np.array_equal(rows[1][:4096, :6], rows[0][:4096, :6])
    assert np.array_equal(bits(rows[1][:, 6:]), bits(rows[0][:, 6:]))
    assert np.all(np.isneginf(rows[3][:4096, 2])) and np.all(rows[3][:4096, 1] == 0.0)
    assert np.all(np.isneginf(rows[4][:4096, 5])) and np.all(rows[4][:4096, 4] == 0.0)
    tiny = np.finfo(np.float64).tiny  # (where the model allows it: a base value that is positive)
    for col in (1, 4):
        positive = rows[0][:4096, col] > 0
        assert positive.any() and np.all((rows[5][:4096, col][positive] > 0) & (rows[5][:4096, col][positive] < tiny))
    ctx.close()


def test_both_entry_points_append_to_one_device_table(zymo_read):
    m = source_model("synthetic", None)
    S = scalings(zymo_read)
    ctx = cp.Context(0)
    a = ctx.modelsv_create([host_scaled(m, S[1]), as_tuple(m)])
    first = [ctx.modelsv_download(i) for i in a]
    b = ctx.modelsv_create_scaled(as_tuple(m), S[1:4])
    for i in a:  # the table grew on the device: what was there is where it was
        assert_same_bits(ctx.modelsv_download(i), first[i], "after create_scaled")
    c = ctx.modelsv_create([host_scaled(m, S[2])])
    assert list(a) + list(b) + list(c) == list(range(6))
    for i in a:
        assert_same_bits(ctx.modelsv_download(i), first[i], "after the second create")
    want = [host_scaled(m, S[1]), as_tuple(m), host_scaled(m, S[1]), host_scaled(m, S[2]), host_scaled(m, S[3]),
            host_scaled(m, S[2])]
    got = [ctx.modelsv_download(i) for i in range(6)]
    ctx.models_clear()
    with pytest.raises(cp.CpecanError):
        ctx.modelsv_download(0)
    again = ctx.modelsv_create(want)
    assert list(again) == list(range(6))  # models_clear reset the ids
    for i in range(6):
        assert_same_bits(got[i], ctx.modelsv_download(i), i)
    assert list(ctx.modelsv_create_scaled(as_tuple(m), S[:1])) == [6]
    ctx.close()


def two_strand_batch(seed, n, lX, lY, every):
    """reads of a synth batch dealt to the two strands in turn: (batch, the two unscaled models, strand per read, the
    oracle's host-scaled model per read under skip bins `skip` -- a function of skip)"""
    batch = synth.make_batch(seed, n, lX, lY, anchor_every=every)
    match, _, gap_y = batch["base_model"]
    bases = [vanilla(match, skip_bins(s), gap_y, s) for s in (0, 1)]
    strand_of = [i % 2 for i in range(n)]

    def oracle_models(skip=None):
        return [o.VanillaModel(synth.scale_model(match, *batch["scalings"][i]),
                               bases[strand_of[i]].skip if skip is None else skip, gap_y, *FUDGE[strand_of[i]])
                for i in range(n)]
    return batch, bases, strand_of, oracle_models


def create_scaled_per_strand(ctx, batch, bases, strand_of):
    """one cpecan_hip_modelsv_create_scaled call per strand; returns the items with every read's model id"""
    items = np.zeros(len(batch["items"]), cp.ITEM_DTYPE)
    for s, base in enumerate(bases):
        mine = [i for i in range(len(strand_of)) if strand_of[i] == s]
        ids = ctx.modelsv_create_scaled(as_tuple(base), batch["scalings"][mine])
        for i, mid in zip(mine, ids):
            it = batch["items"][i]
            items[i] = (it["x_offset"], it["lX"], it["y_offset"], it["lY"], it["anchor_offset"], it["n_anchors"], mid,
                        1, 1, 0)
    return items


def oracle_posterior(batch, i, model, bp):
    it = batch["items"][i]
    x = batch["x_chars"][it["x_offset"]: it["x_offset"] + it["lX"] + 5]
    ev = batch["events"][it["y_offset"]: it["y_offset"] + it["lY"]]
    an = batch["anchors"][it["anchor_offset"]: it["anchor_offset"] + it["n_anchors"]]
    ref = o.aligned_pairs_using_anchors(model, x, it["lX"], ev, an, orc_params(bp, split=1 << 60), 1, 1)
    ref["triples"], ref["logp"] = ref["triples"][::-1], ref["logp"][::-1]
    return ref


def oracle_expectations(batch, models, bp):
    """the 61 sums over all reads"""
    hmm = o.OrcExpectationsV()
    p = orc_params(bp, split=1 << 60)
    for i, it in enumerate(batch["items"]):
        x = batch["x_chars"][it["x_offset"]: it["x_offset"] + it["lX"] + 5]
        ev = batch["events"][it["y_offset"]: it["y_offset"] + it["lY"]]
        an = batch["anchors"][it["anchor_offset"]: it["anchor_offset"] + it["n_anchors"]]
        o.expectations_v_using_anchors(models[i], x, it["lX"], ev, an, p, hmm, True, True)
    return hmm.as_array()


def assert_posterior_is_the_oracles(b, batch, models, bp):
    for i, g in enumerate(batch_results(b)):
        ref = oracle_posterior(batch, i, models[i], bp)
        assert len(g["triples"]) > 0
        assert np.array_equal(g["totals_xay"], ref["totals_xay"])
        assert np.array_equal(g["totals"], ref["totals"])
        assert_same_pairs(g, ref)


def rel_err(got, ref):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.abs(got - ref) / np.abs(ref)
    return np.where(got == ref, 0.0, r)


SHAPES = {
    "v2": dict(n=4, lX=150, lY=310, every=30, md=60, tb=10, e=20, general=False),      # two cells per lane
    "v3": dict(n=4, lX=700, lY=1500, every=50, md=300, tb=40, e=100, general=False),   # three (band 101-156)
    "general": dict(n=4, lX=150, lY=310, every=30, md=60, tb=10, e=20, general=True),
}


def check_kernel(b, shape, name):
    info = b.info()
    if shape["general"]:
        assert info["kernel"] == "general", info
    else:
        assert info["kernel"] == "systolic" and info["family"] == "wave", info
        assert info["cells_per_lane"] == int(name[1]), info


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_alignments_on_device_scaled_models_match_the_oracle(name):
    sh = SHAPES[name]
    batch, bases, strand_of, oracle_models = two_strand_batch(61, sh["n"], sh["lX"], sh["lY"], sh["every"])
    bp = band_params(0.01, sh["md"], sh["tb"], sh["e"])
    ctx = cp.Context(0)
    items = create_scaled_per_strand(ctx, batch, bases, strand_of)
    b = cp.Batch(ctx, items, batch["x_chars"], batch["events"], batch["anchors"], bp,
                 flags=cp.FLAG_GENERAL_KERNEL if sh["general"] else 0, vanilla=True)
    check_kernel(b, sh, name)
    b.run()
    b.sync()
    assert_posterior_is_the_oracles(b, batch, oracle_models(), bp)
    b.close()
    ctx.close()


NEW_BINS = np.concatenate([skip_bins(7), skip_bins(8) * 0.8])


def test_skip_bins_in_place_tables():
    """(a): every block after the call equals that of a fresh context built with the new bins"""
    batch, bases, strand_of, _ = two_strand_batch(62, 4, 150, 310, 30)
    ctx = cp.Context(0)
    items = create_scaled_per_strand(ctx, batch, bases, strand_of)
    ids = ctx.modelsv_create([host_scaled(bases[1], batch["scalings"][0])])  # one made the other way, complement
    assert list(ids) == [4]
    before = [ctx.modelsv_download(i) for i in range(5)]
    ctx.modelsv_set_skip_probs(NEW_BINS)
    got = [ctx.modelsv_download(i) for i in range(5)]
    fresh = cp.Context(0)
    strand = {int(items[i]["model_id"]): strand_of[i] for i in range(4)}
    for mid in range(4):
        read = [i for i in range(4) if int(items[i]["model_id"]) == mid][0]
        fresh.modelsv_create([host_scaled(bases[strand[mid]], batch["scalings"][read], NEW_BINS)])
    fresh.modelsv_create([host_scaled(bases[1], batch["scalings"][0], NEW_BINS)])
    for mid in range(5):
        assert_same_bits(got[mid], fresh.modelsv_download(mid), mid)
        keep = np.ones(STRIDE, bool)
        keep[BINS] = False
        assert np.array_equal(bits(got[mid][keep]), bits(before[mid][keep]))  # nothing but the bins moved
        assert not np.array_equal(got[mid][BINS], before[mid][BINS])
    # the two strands' sets differ in log a_mm and log a_my only
    t = got[int(items[0]["model_id"])][BINS].reshape(30, 5)  # read 0: template, read 1: complement
    c = got[int(items[1]["model_id"])][BINS].reshape(30, 5)
    assert np.array_equal(t[:, [0, 1, 3]], c[:, [0, 1, 3]]) and not np.any(t[:, [2, 4]] == c[:, [2, 4]])
    fresh.close()
    ctx.close()


@pytest.mark.parametrize("name", ["v2", "general"])
def test_skip_bins_in_place_expectations(name):
    """(b): the same expectation batch run again after the call gives the oracle's sums under the new bins"""
    sh = SHAPES[name]
    batch, bases, strand_of, oracle_models = two_strand_batch(63, sh["n"], sh["lX"], sh["lY"], sh["every"])
    bp = band_params(0.01, sh["md"], sh["tb"], sh["e"])
    ctx = cp.Context(0)
    items = create_scaled_per_strand(ctx, batch, bases, strand_of)
    b = cp.Batch(ctx, items, batch["x_chars"], batch["events"], batch["anchors"], bp,
                 flags=cp.FLAG_EXPECTATIONS | (cp.FLAG_GENERAL_KERNEL if sh["general"] else 0), vanilla=True)
    check_kernel(b, sh, name)
    refs = [oracle_expectations(batch, oracle_models(), bp), oracle_expectations(batch, oracle_models(NEW_BINS), bp)]
    assert not np.allclose(refs[0], refs[1], rtol=1e-3, atol=0)  # the new bins are other bins
    for k, ref in enumerate(refs):
        if k == 1:
            ctx.modelsv_set_skip_probs(NEW_BINS)
        b.run()
        b.sync()
        got = sum(b.expectations(mid) for mid in range(sh["n"]))
        err = rel_err(got, ref)
        print("%s run %d: largest relative error of the 61 sums %.3g" % (name, k, err.max()))
        assert np.count_nonzero(ref[:60]) > 20 and ref[-1] < 0
        assert np.all(err <= 1e-9), (k, np.flatnonzero(err > 1e-9), got, ref)
    b.close()
    ctx.close()


def test_skip_bins_in_place_posterior():
    """(c): a decode batch created before the call and run again after it gives the oracle's pairs under the new bins"""
    sh = SHAPES["v2"]
    batch, bases, strand_of, oracle_models = two_strand_batch(64, sh["n"], sh["lX"], sh["lY"], sh["every"])
    bp = band_params(0.01, sh["md"], sh["tb"], sh["e"])
    ctx = cp.Context(0)
    items = create_scaled_per_strand(ctx, batch, bases, strand_of)
    b = cp.Batch(ctx, items, batch["x_chars"], batch["events"], batch["anchors"], bp, vanilla=True)
    check_kernel(b, sh, "v2")
    b.run()
    b.sync()
    assert_posterior_is_the_oracles(b, batch, oracle_models(), bp)
    old = batch_results(b)
    ctx.modelsv_set_skip_probs(NEW_BINS)
    b.run()
    b.sync()
    assert_posterior_is_the_oracles(b, batch, oracle_models(NEW_BINS), bp)
    assert any(not np.array_equal(g["totals"], q["totals"]) for g, q in zip(batch_results(b), old))
    b.close()
    ctx.close()


def test_persistent_loop_equals_rebuilt_loop():
    """Three iterations of em.PersistentVanillaEStep with a fixed sequence of bins against, per iteration, a context
    cleared and rebuilt through cpecan_hip_modelsv_create from host-scaled tables with those bins and the same batch
    created on it and run: 1e-9 relative on the 61 sums, likelihood included.  Tables and kernels are the same on both
    sides and the 61-double blocks of the models are added up the same way, so equality is expected; the test prints
    which it was.  Measured on the MI355X: within the bound but not equal, 3.4e-16 .. 3.5e-16 relative on all three
    iterations -- the E-step kernels add their partial sums with double-precision atomics, whose order is not
    fixed."""
    import torch
    sh = SHAPES["v2"]
    batch, bases, strand_of, _ = two_strand_batch(65, 6, sh["lX"], sh["lY"], sh["every"])
    bp = band_params(0.01, sh["md"], sh["tb"], sh["e"])
    rng = np.random.default_rng(9)
    sequence = [bases[0].skip.copy(), NEW_BINS,
                np.sort(rng.uniform(0.03, 0.45, 60).reshape(2, 30))[:, ::-1].reshape(60).copy()]
    ctx = cp.Context(0)
    step = em().PersistentVanillaEStep(cp, [ctx], batch, bp, range(6), [as_tuple(m) for m in bases], strand_of)
    check_kernel(step.batches[0][1], sh, "v2")
    rebuilt = cp.Context(0)
    equal = []
    for k, skip in enumerate(sequence):
        got = step(skip)
        assert got.shape == (61,)
        rebuilt.models_clear()
        ids = rebuilt.modelsv_create([host_scaled(bases[strand_of[i]], batch["scalings"][i], skip) for i in range(6)])
        items = np.zeros(6, cp.ITEM_DTYPE)
        for i, it in enumerate(batch["items"]):
            items[i] = (it["x_offset"], it["lX"], it["y_offset"], it["lY"], it["anchor_offset"], it["n_anchors"],
                        ids[i], 1, 1, 0)
        b = cp.Batch(rebuilt, items, batch["x_chars"], batch["events"], batch["anchors"], bp,
                     flags=cp.FLAG_EXPECTATIONS, vanilla=True)
        b.run()
        b.sync()
        ptr, n = b.expectations_device_ptr()  # added up as the persistent step adds them: one sum on the device
        want = torch.as_tensor(em()._DeviceDoubles(ptr, n), device="cuda:0").view(-1, 61).sum(0).cpu().numpy()
        b.close()
        err = rel_err(got, want)
        equal.append(bool(np.array_equal(bits(got), bits(want))))
        print("iteration %d: persistent %s rebuilt (largest relative difference %.3g), likelihood %.17g" % (
            k, "==" if equal[-1] else "!=", err.max(), got[-1]))
        assert np.count_nonzero(want[:60]) > 20 and want[-1] < 0
        assert np.all(err <= 1e-9), (k, err.max())
        if k:
            assert not np.allclose(got, previous, rtol=1e-3, atol=0)  # the bins did change the sums
        previous = got
    step.close()
    rebuilt.close()
    ctx.close()


def test_refusals_leave_the_context_usable(zymo_read):
    m = source_model("synthetic", None)
    S = scalings(zymo_read)
    ctx = cp.Context(0)

    def refused(call):
        with pytest.raises(cp.CpecanError) as ei:
            call()
        assert ei.value.code == cp.EINVAL
        assert cp.lib().cpecan_hip_last_error().decode().strip() != ""

    refused(lambda: ctx.modelsv_set_skip_probs(NEW_BINS))  # no vanilla models yet
    refused(lambda: ctx.modelsv_create_scaled(as_tuple(m), S[:0]))  # n = 0
    desc = cp.VanillaModelDesc()
    desc.m_to_y_not_x, desc.e_to_e = FUDGE[0]
    desc.match_probs, desc.skip_probs, desc.gap_y_probs = None, m.skip.ctypes.data, m.gap_y.ctypes.data
    ids = np.zeros(1, np.int32)
    one = np.ascontiguousarray(S[:1])
    L = cp.lib()

    def raw(rc):  # a call made past the binding's own argument handling
        if rc != cp.OK:
            raise cp.CpecanError(rc, L.cpecan_hip_last_error().decode())

    refused(lambda: raw(L.cpecan_hip_modelsv_create_scaled(ctx.h, cp.C.byref(desc), one.ctypes.data, 1, 1,
                                                           ids.ctypes.data)))  # NULL table
    refused(lambda: raw(L.cpecan_hip_modelsv_create_scaled(ctx.h, None, one.ctypes.data, 1, 1, ids.ctypes.data)))
    refused(lambda: ctx.modelsv_download(0))  # still no model
    assert list(ctx.modelsv_create_scaled(as_tuple(m), S[:2])) == [0, 1]
    refused(lambda: ctx.modelsv_download(2))
    refused(lambda: ctx.modelsv_download(-1))
    refused(lambda: raw(L.cpecan_hip_modelsv_set_skip_probs(ctx.h, None)))
    # ... and the context works: the blocks are right and the bins can be set
    want = cp.Context(0)
    want.modelsv_create([host_scaled(m, S[1], NEW_BINS)])
    ctx.modelsv_set_skip_probs(NEW_BINS)
    assert_same_bits(ctx.modelsv_download(1), want.modelsv_download(0))
    want.close()
    ctx.close()

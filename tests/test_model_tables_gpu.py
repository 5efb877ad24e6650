"""The model tables of a context (ModelTable, cpecan_models.hip), the same checks on all six machines: a table that grows
keeps what it held, a batch outlives a later create call, the threaded creates pack their pinned slots right, and
cpecan_hip_models_clear starts every table again from id 0.

Tiny shapes (30 k-mers against 45 events, 40 against 40 bases for DNA), default bands.  Tables and results of two
contexts that hold the same models are compared bit for bit: both ran the same code on the same inputs.  Against the
oracle every machine keeps the bar of its own test file (test_parity_general_gpu, test_dna5_gpu, test_vanilla_gpu,
test_hdp_gpu, test_sm4_gpu, test_echelon_gpu): totalProbability refreshes, exponents, pairs, their order and integer
posteriors identical."""
import os

import numpy as np
import pytest

import pyoracle as o
import synth
from harness import assert_same_pairs, band_params, batch_results, cp, hdp_batch, orc_params
from test_dna5_gpu import evolve
from test_echelon_gpu import host_piece, reads as echelon_reads
from test_vanilla_gpu import skip_bins

pytestmark = pytest.mark.gpu

MACHINES = ["strawman", "dna5", "vanilla", "hdp", "sm4", "echelon"]
BP = band_params()
RAGGED = (1, 1)
FUDGE = ((float(np.float32(0.17)), float(np.float32(0.55))), (float(np.float32(0.14)), float(np.float32(0.49))))
CLEARED = "cpecan_hip_models_clear was called on the context after this batch was created"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class Kit:
    """three reads and three distinct models of one machine: read i belongs to model i.
    models: what the machine's create call takes; create(ctx, models) -> ids; batch(ctx, reads, ids) -> a Batch of those
    reads, read reads[k] on model ids[k]; oracle(read, model) -> the reference result; same(got, ref) asserts the
    machine's bar; download(ctx, id) (strawMan and vanilla) -> the device block"""
    download = None

    def __init__(self):
        self._refs = {}

    def ref(self, read, model=None):
        key = (read, read if model is None else model)
        if key not in self._refs:
            self._refs[key] = self.oracle(*key)
        return self._refs[key]

    def same(self, got, ref):
        assert np.array_equal(got["totals_xay"], ref["totals_xay"])
        assert np.array_equal(bits(got["totals"]), bits(ref["totals"]))
        assert_same_pairs(got, ref)
        assert len(got["triples"]) > 0


class SignalKit(Kit):
    """the machines that align k-mers to events and have their reference in the oracle"""

    def __init__(self, data, models, oracle_models, create, **kind):
        super().__init__()
        self.data, self.models, self.oracle_models, self.create, self.kind = data, models, oracle_models, create, kind

    def batch(self, ctx, reads, ids):
        items = np.zeros(len(reads), cp.ITEM_DTYPE)
        for k, (r, mid) in enumerate(zip(reads, ids)):
            it = self.data["items"][r]
            items[k] = (it["x_offset"], it["lX"], it["y_offset"], it["lY"], it["anchor_offset"], it["n_anchors"], mid,
                        RAGGED[0], RAGGED[1], 0)
        return cp.Batch(ctx, items, self.data["x_chars"], self.data["events"], self.data["anchors"], BP, **self.kind)

    def oracle(self, read, model):
        it = self.data["items"][read]
        x = self.data["x_chars"][it["x_offset"]: it["x_offset"] + it["lX"] + 5]
        ev = self.data["events"][it["y_offset"]: it["y_offset"] + it["lY"]]
        an = self.data["anchors"][it["anchor_offset"]: it["anchor_offset"] + it["n_anchors"]]
        r = o.aligned_pairs_using_anchors(self.oracle_models[model], x, it["lX"], ev, an, orc_params(BP, split=1 << 60),
                                          RAGGED[0], RAGGED[1])
        r["triples"], r["logp"] = r["triples"][::-1], r["logp"][::-1]  # emission order
        return r


def strawman_kit(golden_dir):
    data = synth.make_batch(71, 3, 30, 45, anchor_every=10)  # a model per read: the pore model scaled for it
    kit = SignalKit(data, [(cp.NANOPORE_TRANSITIONS, m, gx, gy) for m, gx, gy in data["models"]],
                    [o.Sm3Model(m, gy, gx) for m, gx, gy in data["models"]], lambda ctx, ms: ctx.models_create(ms))
    kit.download = lambda ctx, i: ctx.models_download(i)
    return kit


def vanilla_models(data_models):
    return [o.VanillaModel(m, skip_bins(i), gy, *FUDGE[i % 2]) for i, (m, _, gy) in enumerate(data_models)]


def vanilla_kit(golden_dir):
    data = synth.make_batch(72, 3, 30, 45, anchor_every=10)
    oms = vanilla_models(data["models"])
    kit = SignalKit(data, [(m.scalars, m.match, m.skip, m.gap_y) for m in oms], oms,
                    lambda ctx, ms: ctx.modelsv_create(ms), vanilla=True)
    kit.download = lambda ctx, i: ctx.modelsv_download(i)
    return kit


def sm4_kit(golden_dir):
    data = synth.make_batch(73, 3, 30, 45, anchor_every=10)
    oms = [o.Sm4Model(m, gy) for m, _, gy in data["models"]]
    return SignalKit(data, [(m.transitions, m.match, m.gap_x, m.gap_y) for m in oms], oms,
                     lambda ctx, ms: ctx.models4_create(ms), sm4=True)


def hdp_kit(golden_dir):
    """one HDP, three sets of transitions: match -> gap Y opens with one, three and five times the default probability
    (the match row renormalised; no switch between the gaps, as the default has none)"""
    nhdp = o.load_nhdp(os.path.join(golden_dir, "testTemplate.nhdp"))
    data, _ = hdp_batch(74, 3, 30, 10, nhdp)
    ts = []
    for k in range(3):
        t = list(cp.NANOPORE_TRANSITIONS)
        open_x, open_y = np.exp(t[3]), np.exp(t[4]) * (1 + 2 * k)
        t[0], t[4] = float(np.log(1.0 - open_x - open_y)), float(np.log(open_y))
        ts.append(tuple(t))
    return SignalKit(data, [(t, nhdp["alphabet"], nhdp["grid"], nhdp["y"], nhdp["slope"], nhdp["kmer_row"]) for t in ts],
                     [o.HdpModel(nhdp, t) for t in ts], lambda ctx, ms: ctx.modelsh_create(ms), hdp=True)


class DnaKit(Kit):
    """40 against about 40 bases, no anchors; the models differ in the match state's self transition"""

    def __init__(self):
        super().__init__()
        rng = np.random.default_rng(75)
        self.seqs = [evolve(rng, 40)[:2] for _ in range(3)]
        self.oracle_models = []
        for k in range(3):
            m = o.Sm5Model()
            m.c.t[0] -= 0.3 * k
            self.oracle_models.append(m)
        self.models = [(list(m.c.t), m.match, m.gx, m.gy) for m in self.oracle_models]

    def create(self, ctx, models):
        return ctx.models5_create(models)

    def batch(self, ctx, reads, ids):
        xs, ys, off = "", "", []
        for x, y in self.seqs:
            off.append((len(xs), len(ys)))
            xs, ys = xs + x, ys + y
        items = np.zeros(len(reads), cp.ITEM_DTYPE)
        for k, (r, mid) in enumerate(zip(reads, ids)):
            items[k] = (off[r][0], len(self.seqs[r][0]), off[r][1], len(self.seqs[r][1]), 0, 0, mid, RAGGED[0],
                        RAGGED[1], 0)
        return cp.Batch(ctx, items, xs, None, np.zeros((0, 2), np.int64), BP, y_chars=ys)

    def oracle(self, read, model):
        x, y = self.seqs[read]
        r = o.aligned_pairs_using_anchors(self.oracle_models[model], x, len(x), y, np.zeros((0, 2), np.int64),
                                          orc_params(BP, split=1 << 60), RAGGED[0], RAGGED[1])
        r["triples"], r["logp"] = r["triples"][::-1], r["logp"][::-1]
        return r

    def same(self, got, ref):
        assert got["cells"] == ref["cells"]
        super().same(got, ref)


class EchelonKit(Kit):
    """reads with a machine of their own (test_echelon_gpu.reads); the reference is the host library's cell function"""

    def __init__(self):
        super().__init__()
        self.rds = echelon_reads(76, 3, 30, 45, anchor_every=10)
        self.models = [r["machine"].gpu_model() for r in self.rds]

    def create(self, ctx, models):
        return ctx.modelse_create(models)

    def batch(self, ctx, reads, ids):
        xs, evs, ans, off = b"", [], [], []
        for r in self.rds:
            off.append((len(xs), sum(len(v) for v in evs), sum(len(a) for a in ans)))
            xs += r["seq"]
            evs.append(r["events"])
            ans.append(np.asarray(r["anchors"], np.int64).reshape(-1, 2))
        items = np.zeros(len(reads), cp.ITEM_DTYPE)
        for k, (r, mid) in enumerate(zip(reads, ids)):
            items[k] = (off[r][0], 30, off[r][1], 45, off[r][2], len(ans[r]), mid, RAGGED[0], RAGGED[1], 0)
        return cp.Batch(ctx, items, xs, np.concatenate(evs), np.concatenate(ans), BP, echelon=True)

    def oracle(self, read, model):
        rd = dict(self.rds[read], machine=self.rds[model]["machine"])
        return host_piece(rd, 0, 0, 30, 45, rd["anchors"], RAGGED[0], RAGGED[1], BP)

    def same(self, got, ref):  # (the bar of test_echelon_gpu.same)
        assert np.array_equal(got["totals_xay"], ref["totals_xay"])
        assert np.array_equal(got["totals"], ref["totals"])
        assert got["triples"].shape == ref["triples"].shape and len(ref["triples"]) > 0
        assert np.array_equal(got["triples"], ref["triples"])


BUILDERS = dict(strawman=strawman_kit, dna5=lambda g: DnaKit(), vanilla=vanilla_kit, hdp=hdp_kit, sm4=sm4_kit,
                echelon=lambda g: EchelonKit())
_KITS = {}


@pytest.fixture(params=MACHINES)
def kit(request, golden_dir):
    """built once per machine and shared by the tests, with the references it has computed so far"""
    if request.param not in _KITS:
        _KITS[request.param] = BUILDERS[request.param](golden_dir)
    return _KITS[request.param]


def run(b):
    b.run()
    b.sync()
    return batch_results(b)


def assert_identical(a, b):
    """two results of one item, bit for bit"""
    assert a["cells"] == b["cells"]
    assert np.array_equal(a["triples"], b["triples"]) and np.array_equal(bits(a["logp"]), bits(b["logp"]))
    assert np.array_equal(a["totals_xay"], b["totals_xay"]) and np.array_equal(bits(a["totals"]), bits(b["totals"]))


def three_reads_on_their_models(kit, ctx):
    b = kit.batch(ctx, [0, 1, 2], [0, 1, 2])
    got = run(b)
    b.close()
    for i in range(3):
        kit.same(got[i], kit.ref(i))
    return got


def test_the_models_differ(kit):
    """(what the other tests lean on) a read run on another read's model gives other pairs"""
    for i in range(3):
        mine, other = kit.ref(i), kit.ref(i, (i + 1) % 3)
        assert not np.array_equal(mine["triples"], other["triples"])


def test_growth_keeps_what_was_there_and_a_batch_outlives_it(kit):
    A, B = cp.Context(0), cp.Context(0)
    assert list(kit.create(A, kit.models)) == [0, 1, 2]
    assert list(kit.create(B, kit.models[:1])) == [0]
    early = kit.batch(B, [0], [0])  # created before the table grows, run before and after
    before = run(early)
    first = kit.download(B, 0) if kit.download else None
    assert list(kit.create(B, kit.models[1:])) == [1, 2]
    after = run(early)
    assert_identical(after[0], before[0])
    kit.same(after[0], kit.ref(0))
    early.close()
    if kit.download:
        assert np.array_equal(bits(kit.download(B, 0)), bits(first))
        for i in range(3):
            a, b = kit.download(A, i), kit.download(B, i)
            assert a.size == b.size > 0 and np.array_equal(bits(a), bits(b)), i
        assert not np.array_equal(kit.download(A, 0), kit.download(A, 1))
    for a, b in zip(three_reads_on_their_models(kit, A), three_reads_on_their_models(kit, B)):
        assert_identical(a, b)
    B.close()
    A.close()


def test_clear_starts_every_table_again(kit):
    ctx = cp.Context(0)
    assert list(kit.create(ctx, kit.models[::-1])) == [0, 1, 2]  # the models the other way round, to be forgotten
    old = kit.batch(ctx, [0], [2])
    kit.same(run(old)[0], kit.ref(0))
    ctx.models_clear()
    assert list(kit.create(ctx, kit.models[:2])) == [0, 1]
    assert list(kit.create(ctx, kit.models[2:])) == [2]
    three_reads_on_their_models(kit, ctx)
    with pytest.raises(cp.CpecanError) as ei:  # ids of before the clear are refused, whatever the tables hold now
        old.run()
    assert ei.value.code == cp.EINVAL and CLEARED in str(ei.value)
    old.close()
    ctx.close()


# ---- slot packing of the threaded creates: every host thread fills two pinned slots in turn

def alone(create, download, model):
    ctx = cp.Context(0)
    assert list(create(ctx, [model])) == [0]
    block = download(ctx, 0)
    ctx.close()
    return block


@pytest.fixture(scope="module")
def nine_vanilla():
    """nine distinct vanilla models and the block of each created alone in a fresh context"""
    match, _, gap_y = synth.synthetic_pore_model()
    ms = [o.VanillaModel(synth.scale_model(match, 1.0 + 0.01 * i, i - 4.0, 1.0 + 0.02 * i, 1.0, 1.0), skip_bins(i), gap_y,
                         *FUDGE[i % 2]) for i in range(9)]
    models = [(m.scalars, m.match, m.skip, m.gap_y) for m in ms]
    return models, [alone(lambda c, q: c.modelsv_create(q), lambda c, i: c.modelsv_download(i), m) for m in models]


@pytest.mark.parametrize("threads", [1, 2])
def test_vanilla_slots_hold_up_to_four_models(nine_vanilla, threads):
    """one thread: slots of 4, 4 and 1 models, the third in the slot of the first; two threads: slots of two models,
    the first thread's third slot holds one"""
    models, want = nine_vanilla
    ctx = cp.Context(0)
    assert list(ctx.modelsv_create(models, threads=threads)) == list(range(9))
    for i in range(9):
        got = ctx.modelsv_download(i)
        assert got.size == want[i].size and np.array_equal(bits(got), bits(want[i])), i
    assert not np.array_equal(want[0], want[8])
    ctx.close()


def test_strawman_slot_is_reused_on_the_third_turn():
    kit = _KITS.get("strawman") or strawman_kit(None)
    want = [alone(kit.create, kit.download, m) for m in kit.models]
    ctx = cp.Context(0)
    assert list(ctx.models_create(kit.models, threads=1)) == [0, 1, 2]
    for i in range(3):
        got = ctx.models_download(i)
        assert got.size == want[i].size and np.array_equal(bits(got), bits(want[i])), i
    assert not np.array_equal(want[0], want[2])
    ctx.close()

"""The readback (candidate cut in every kernel, cpecan_k_pack_pairs, ensure_counts, cpecan_hip_batch_fetch_pairs) on
the inputs of readback_cases.py, against the oracle at the project's bar: cells, totals, exponents and pairs
array_equal.  The inputs are proven on the CPU by test_readback_cases_cpu.py.

1. 18 thresholds placed on three real candidates (on the cell, one ulp above, inside and outside the pack kernel's
   1e-9 margin, inside the kernels' 1e-3 slack), on every decode path of the strawMan, vanilla, HDP, DNA, 4-state
   and echelon machines.
2. tiny items whose posterior sits next to a multiple of 1e-7, and next to 1, on the wave and workgroup families and
   the general kernel.
3. batches whose close calls fall below and above the list's 65 536 entries, with the threaded host scan, and on the
   capacity itself.
4. sequences of 65 535 (packed coordinates) and 65 536 elements (16-byte records)."""
import re

import numpy as np
import pytest

import pyoracle as o
import readback_cases as rc
from harness import assert_same_posterior, batch_results, band_params, cp, make_items

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = cp.Context(0)
    yield c
    c.close()


# ------------------------------------------------- 1. thresholds -------------------------------------------------

WG, WIDE, GEN, SCAN = cp.FLAG_WORKGROUP_KERNELS, cp.FLAG_WIDE_BANDS, cp.FLAG_GENERAL_KERNEL, cp.FLAG_SCAN_DECODE


def wave(cells, asm=None):
    def check(info):
        assert info["kernel"] == "systolic" and info["family"] == "wave" and info["cells_per_lane"] == cells, info
        if asm is not None:
            assert info["assembly_sweeps"] == asm, info
    return check


def workgroup(rows):
    def check(info):
        assert info["kernel"] == "systolic" and info["family"] == "workgroup", info
        assert info["waves_per_workgroup"] == rows, info
    return check


def general(info):
    assert info["kernel"] == "general" and info.get("family") is None, info


def wave5(info):
    assert info["kernel"] == "general" and info.get("family") == "wave (5-state)", info


# (machine, shape, flags, environment, the route info() must show)
PATHS = {
    "sm3-wave2": ("sm3", "w120", 0, {}, wave(2)),
    "sm3-wave3-compiled": ("sm3", "w158", 0, {"CPECAN_ASM": "0"}, wave(3, asm=0)),
    "sm3-wave3-asm": ("sm3", "w158", 0, {}, wave(3, asm=2)),
    "sm3-wave3-asm-small-footprint": ("sm3", "w158", cp.FLAG_SMALL_FOOTPRINT, {}, wave(3, asm=2)),
    "sm3-wave4": ("sm3", "w248", 0, {}, wave(4)),
    "sm3-wave2-scan": ("sm3", "w120", SCAN, {}, wave(2)),
    "sm3-wg6-scan": ("sm3", 376, WIDE | SCAN, {}, workgroup(6)),
    "sm3-wg1": ("sm3", "w56", WG, {}, workgroup(1)),
    "sm3-wg2": ("sm3", "w120", WG, {}, workgroup(2)),
    "sm3-wg3": ("sm3", "w184", WG, {}, workgroup(3)),
    "sm3-wg4": ("sm3", "w248", WG, {}, workgroup(4)),
    "sm3-wg6": ("sm3", 376, WIDE, {}, workgroup(6)),
    "sm3-wg8": ("sm3", 504, WIDE, {}, workgroup(8)),
    "sm3-general": ("sm3", "w120", GEN, {}, general),
    "vanilla-wave2": ("vanilla", "w120", 0, {}, wave(2)),
    "vanilla-wave3": ("vanilla", "w184", 0, {}, wave(3)),
    "vanilla-v4": ("vanilla", "w248", WIDE, {}, workgroup(4)),
    "vanilla-v6": ("vanilla", 376, WIDE, {}, workgroup(6)),
    "vanilla-v8": ("vanilla", 504, WIDE, {}, workgroup(8)),
    "vanilla-general": ("vanilla", "w120", GEN, {}, general),
    "hdp-wave2": ("hdp", "w120", 0, {}, wave(2)),
    "hdp-wave3": ("hdp", "w184", 0, {}, wave(3)),
    "hdp-wave4": ("hdp", "w248", 0, {}, wave(4)),
    "hdp-h6": ("hdp", 376, cp.FLAG_WIDE_BANDS_HDP, {}, workgroup(6)),
    "hdp-h8": ("hdp", 504, cp.FLAG_WIDE_BANDS_HDP, {}, workgroup(8)),
    "hdp-general": ("hdp", "w120", GEN, {}, general),
    "dna-wave": ("dna", "w128", 0, {"CPECAN_WAVE5_PAIRED": "0"}, wave5),
    "dna-pair": ("dna", "w128", 0, {"CPECAN_WAVE5_PAIRED": "1"}, wave5),
    "dna-general": ("dna", "w128", GEN, {}, general),
    "sm4-general": ("sm4", "w120", 0, {}, general),
}


def hdp_pair():
    nhdp = rc.load_nhdp()
    return nhdp, rc.cached("hdp-model", lambda: o.HdpModel(nhdp))


def signal_shape(machine, name):
    """the shape (cached) and its oracle models, one per batch model"""
    hdp = hdp_pair() if machine == "hdp" else None
    key = ("shape", "hdp" if hdp else "signal", name)
    shape = rc.cached(key, lambda: rc.wide_shape(name, hdp) if isinstance(name, int) else rc.family_shape(name, hdp))
    if machine == "hdp":
        return shape, [hdp[1]]
    make = dict(sm3=rc.sm3_models, vanilla=rc.vanilla_models, sm4=rc.sm4_models)[machine]
    return shape, rc.cached(("models", machine, name), lambda: make(shape["batch"]))


def upload(ctx, machine, models):
    ctx.models_clear()
    if machine == "sm3":
        ctx.models_create([(cp.NANOPORE_TRANSITIONS, m.match, m.gap_x, m.gap_y) for m in models])
    elif machine == "vanilla":
        ctx.modelsv_create([(m.scalars, m.match, m.skip, m.gap_y) for m in models])
    elif machine == "sm4":
        ctx.models4_create([(m.transitions, m.match, m.gap_x, m.gap_y) for m in models])
    elif machine == "hdp":
        nhdp = rc.load_nhdp()
        ctx.modelsh_create([(cp.NANOPORE_TRANSITIONS, nhdp["alphabet"], nhdp["grid"], nhdp["y"], nhdp["slope"],
                             nhdp["kmer_row"])])


def signal_batch(ctx, machine, shape, bp, flags):
    b = shape["batch"]
    kind = dict(sm3={}, vanilla=dict(vanilla=True), sm4=dict(sm4=True), hdp=dict(hdp=True))[machine]
    if machine == "sm3" and flags & GEN:  # the strawMan create call takes the kernel as an argument of its own
        kind, flags = dict(kernel=cp.KERNEL_GENERAL), flags & ~GEN
    return cp.Batch(ctx, make_items(b, shape["ragged"]), b["x_chars"], b["events"], b["anchors"], bp, flags=flags, **kind)


def dna_case(name):
    import edge_reads as er
    f = er.DNA_FAMILIES[name]
    batch = rc.cached(("dna", name), lambda: er.dna_batch(name))
    model = rc.cached("sm5", o.Sm5Model)
    shape = dict(md=f["md"], tb=f["tb"], e=batch["e"], ragged=f["ragged"])

    def refs():
        bp = rc.shape_bp(shape, 0.0)
        return [rc.with_p(rc.oracle_item(model, (x, len(x), y, a), bp, f["ragged"])) for x, y, a in batch["seqs"]]
    return shape, batch, model, rc.cached(("ref0", "dna", name), refs)


@pytest.mark.parametrize("path", list(PATHS))
def test_threshold_on_a_candidate(ctx, path, monkeypatch):
    machine, name, flags, env, route = PATHS[path]
    for k in ("CPECAN_ASM", "CPECAN_WAVE5_PAIRED"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if machine == "dna":
        from test_band_edges_machines_gpu import dna_items
        shape, batch, model, refs0 = dna_case(name)
        _, _, items, xs, ys, anchors = dna_items(ctx, batch["seqs"], shape["ragged"])
        make = lambda bp: cp.Batch(ctx, items, xs, None, anchors, bp, flags=flags, y_chars=ys)
    else:
        shape, models = signal_shape(machine, name)
        refs0 = rc.refs_at_zero((machine, name), models, shape)
        upload(ctx, machine, models)
        make = lambda bp: signal_batch(ctx, machine, shape, bp, flags)
    cases = rc.threshold_cases(refs0[0])
    assert len(cases) == 18 and [c[3] for c in cases] == list(rc.KEEPS) * 3
    for j, (k, e, thr, keeps) in enumerate(cases):
        b = make(rc.shape_bp(shape, thr))
        route(b.info())
        b.run()
        b.sync()
        res = batch_results(b)
        b.close()
        for i, g in enumerate(res):
            assert_same_posterior(g, rc.expected_at(refs0[i], thr), (path, j, i))
        cell = tuple(refs0[0]["triples"][k, 1:])
        assert any(tuple(t[1:]) == cell for t in res[0]["triples"]) == keeps, (path, j)


def test_threshold_on_a_candidate_echelon(ctx):
    """cpecan_k_generale: the 18 thresholds on three states' exponents of item 0 (the host DP's, read from its cells);
    a state inside the kernel's slack emits its s candidates, which the readback drops"""
    import test_echelon_gpu as te
    pieces, refs0 = rc.echelon_case()
    cases = rc.threshold_cases(refs0[0])
    assert len(cases) == 18 and [c[3] for c in cases] == list(rc.KEEPS) * 3
    for j, (k, e, thr, keeps) in enumerate(cases):
        res = te.run_batch(ctx, pieces, band_params(thr, **rc.ECHELON_BP))
        for i, g in enumerate(res):
            want = rc.expected_at(refs0[i], thr)
            te.same(g, want)
            assert np.array_equal(g["logp"], want["logp"]), (j, i)
        n0 = np.count_nonzero(refs0[0]["logp"] == e)
        assert np.count_nonzero(res[0]["logp"] == e) == (n0 if keeps else 0), (j, n0)


# ------------------------------------------- 2. multiples of 1e-7, next to 1 -------------------------------------------


@pytest.mark.parametrize("family", [0, WG, GEN], ids=["wave", "workgroup", "general"])
def test_posteriors_on_multiples_of_1e_7_and_next_to_1(ctx, family):
    batch, refs, classes = rc.floor_batch()
    upload(ctx, "sm3", rc.sm3_models(batch))
    for thr in (0.01, 0.0):
        b = cp.Batch(ctx, make_items(batch), batch["x_chars"], batch["events"], batch["anchors"],
                     band_params(thr, **rc.FLOOR_BP), kernel=cp.KERNEL_GENERAL if family == GEN else cp.KERNEL_AUTO,
                     flags=family & ~GEN)
        info = b.info()
        assert info["kernel"] == ("general" if family == GEN else "systolic"), info
        if family != GEN:
            assert info["family"] == ("workgroup" if family else "wave"), info
        b.run()
        b.sync()
        res = batch_results(b)
        b.close()
        for i, g in enumerate(res):
            assert_same_posterior(g, rc.expected_at(refs[i], thr), (thr, i))


# ------------------------------------------------ 3. the list's capacity ------------------------------------------------


def run_counted(ctx, names, threshold, monkeypatch, capfd):
    """compose(names) at `threshold` on the default kernels: every item against the oracle result of the read it
    copies, and the (candidates, close calls) ensure_counts printed"""
    batch, names = rc.compose(names)
    upload(ctx, "sm3", rc.sm3_models(batch))
    b = cp.Batch(ctx, make_items(batch), batch["x_chars"], batch["events"], batch["anchors"],
                 band_params(threshold, **rc.CAP_BP))
    b.run()
    b.sync()
    capfd.readouterr()
    monkeypatch.setenv("CPECAN_TIMING", "1")
    b.counts()
    monkeypatch.delenv("CPECAN_TIMING")
    printed = re.findall(r"ensure_counts: (\d+) candidates, (\d+) left to the host", capfd.readouterr().err)
    assert len(printed) == 1, printed
    res = batch_results(b)
    b.close()
    want = {n: rc.expected_at(rc.cap_read(n)["ref0"], threshold) for n in set(names) if n is not None}
    for i, (n, g) in enumerate(zip(names, res)):
        if n is None:
            assert len(g["triples"]) == 0, i
        else:
            assert_same_posterior(g, want[n], (i, n))
    return int(printed[0][0]), int(printed[0][1])


def test_threaded_scan_with_the_list(ctx, monkeypatch, capfd):
    n, m = run_counted(ctx, rc.LARGE, rc.LARGE_LIST_THRESHOLD, monkeypatch, capfd)
    print("candidates %d, close calls %d" % (n, m))
    assert n > rc.THREADED_ABOVE and 1000 < m < rc.UNDECIDED_CAP // 2


def test_threaded_scan_item_by_item(ctx, monkeypatch, capfd):
    n, m = run_counted(ctx, rc.LARGE, 0.0, monkeypatch, capfd)
    print("candidates %d, close calls %d" % (n, m))
    assert n > rc.THREADED_ABOVE and m > 2 * rc.UNDECIDED_CAP


def test_small_batch_over_the_capacity(ctx, monkeypatch, capfd):
    n, m = run_counted(ctx, rc.SMALL_OVER, 0.0, monkeypatch, capfd)
    print("candidates %d, close calls %d" % (n, m))
    assert n < rc.THREADED_ABOVE and m > rc.UNDECIDED_CAP + 1000


@pytest.mark.parametrize("target", [rc.UNDECIDED_CAP, rc.UNDECIDED_CAP + 1])
def test_close_calls_on_the_capacity_itself(ctx, target, monkeypatch, capfd):
    n, m = run_counted(ctx, rc.exact_cap_names(target), 0.0, monkeypatch, capfd)
    assert m == target, (n, m)


# ------------------------------------------------ 4. 65 535 / 65 536 ------------------------------------------------


@pytest.mark.parametrize("name", list(rc.LONG_CASES))
def test_coordinates_at_65535_and_65536(ctx, name):
    axis, length, _, packed = rc.LONG_CASES[name]
    batch, refs = rc.long_batch(name)
    upload(ctx, "sm3", rc.sm3_models(batch))
    b = cp.Batch(ctx, make_items(batch), batch["x_chars"], batch["events"], batch["anchors"],
                 band_params(rc.LONG_THRESHOLD, **rc.LONG_BP))
    assert b.info()["kernel"] == "systolic" and b.info()["family"] == "wave", b.info()
    b.run()
    b.sync()
    res = batch_results(b)
    b.close()
    for i, (g, r) in enumerate(zip(res, refs)):
        assert_same_posterior(g, r, (name, i))
    col = res[0]["triples"][:, 1 if axis == "x" else 2]
    assert np.count_nonzero(col >= length - 10) >= 5 and col.max() == length - 1
    assert (col.max() >= 65535) == (not packed)


# ------------------------------------ 5. CPECAN_HOST_FINALISE, CPECAN_PACK_LATER ------------------------------------


def test_host_finalise_and_pack_later_change_nothing(tmp_path):
    """both switches are read once per process: readback_env_child.py runs its fixed list of batches in three fresh
    processes (plain, every pair through the host libm, candidates packed when first asked for), one after the other;
    the three files are equal array for array, and equal to the oracle's expected values"""
    import os
    import subprocess
    import sys
    import readback_env_child as child
    files = {}
    for name, var in (("plain", None), ("host", "CPECAN_HOST_FINALISE"), ("later", "CPECAN_PACK_LATER")):
        env = {k: v for k, v in os.environ.items() if k not in ("CPECAN_HOST_FINALISE", "CPECAN_PACK_LATER")}
        if var is not None:
            env[var] = "1"
        path = str(tmp_path / (name + ".npz"))
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, child.__file__, path], env=env,
                           capture_output=True, text=True, timeout=400)
        assert r.returncode == 0, (name, r.stderr[-2000:])
        files[name] = dict(np.load(path))
    for name in ("host", "later"):
        assert sorted(files[name]) == sorted(files["plain"])
        for key, a in files["plain"].items():
            assert a.dtype == files[name][key].dtype and a.tobytes() == files[name][key].tobytes(), (name, key)
    got = files["plain"]
    for run in child.runs():
        for i, want in enumerate(child.expected(run)):
            g = {key: got["%s/%d/%s" % (run[0], i, key)] for key in ("triples", "logp", "totals_xay", "totals")}
            g["cells"] = int(got["%s/%d/cells" % (run[0], i)][0])
            assert_same_posterior(g, want, (run[0], i))
            if run[0] == "threshold-0":
                assert np.array_equal(got["twice/%d/triples" % i], want["triples"])
                assert np.array_equal(got["twice/%d/logp" % i], want["logp"])

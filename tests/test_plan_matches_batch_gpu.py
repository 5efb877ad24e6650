"""What the three plan calls answer without a device (cpecan_hip_plan_dispatch, _plan_assembly_sweeps,
_plan_expectation_pass) is what batch creation does: one single-read batch per route of the kernel choice is created --
not run -- and its info() is held against the plan's answers for its machine, mode, flags and its own widest band."""
import os

import numpy as np
import pytest

import edge_reads
import pyoracle as o
from harness import BATCH_ENV, band_params, cp, make_items
from test_hdp_workgroup_gpu import exact_width_batch as hdp_width_batch
from test_hdp_workgroup_gpu import hbatch
from test_hdp_workgroup_gpu import upload as upload_hdp
from test_vanilla_workgroup_gpu import exact_width_batch as vanilla_width_batch
from test_vanilla_workgroup_gpu import upload as upload_vanilla
from test_vanilla_workgroup_gpu import vanilla_models, vbatch
from test_wide_workgroup_gpu import exact_width_batch as strawman_width_batch

pytestmark = pytest.mark.gpu

POST, EXPECT = cp.MODE_POSTERIOR, cp.MODE_EXPECTATIONS
WG, WIDE = cp.FLAG_WORKGROUP_KERNELS, cp.FLAG_WIDE_BANDS


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in BATCH_ENV:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def ctx():
    c = cp.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def nhdp(golden_dir):
    return o.load_nhdp(os.path.join(golden_dir, "testTemplate.nhdp"))


def first_read(batch):
    """the batch of the first read alone (its offsets are 0: the arrays stay as they are)"""
    out = dict(batch, items=batch["items"][:1])
    if "models" in batch:
        out["models"] = batch["models"][:1]
    return out


def bands_of(reads, e):
    """(widest band, whether every band edge moves by at most one k-mer per diagonal) of (anchors, lX, lY) reads, as batch
    creation works them out: on the host"""
    width, by_one = 0, True
    for an, lX, lY in reads:
        L, R = cp.band_construct(an, lX, lY, e)
        k = np.arange(len(L))
        width = max(width, int((((R - L) >> 1) + 1).max()))
        for edge in ((k + L) // 2, (k + R) // 2):
            by_one = by_one and bool(((np.diff(edge) >= 0) & (np.diff(edge) <= 1)).all())
    return width, by_one


def signal_bands(batch, e):
    return bands_of([(batch["anchors"][it["anchor_offset"]: it["anchor_offset"] + it["n_anchors"]], it["lX"], it["lY"])
                     for it in batch["items"]], e)


def check(b, machine, mode, kernel, flags, bands, lands):
    """info() of the created batch against the three plan calls; lands: what the route was chosen to be"""
    width, by_one = bands
    q = (machine, mode, kernel, flags, width, by_one)
    d = cp.plan_dispatch(*q)
    want = dict(kernel="systolic" if d["kernel"] == cp.KERNEL_SYSTOLIC else "general", max_band_width=width,
                fused_expectations=cp.plan_expectation_pass(*q))
    if d["kernel"] == cp.KERNEL_SYSTOLIC:
        want.update(family="wave" if d["wave"] else "workgroup", waves_per_workgroup=d["rows"])
        if d["wave"]:
            want["cells_per_lane"] = d["rows"]
    elif machine == cp.MACHINE_DNA5 and d["wave"]:
        want["family"] = "wave (5-state)"
    info = b.info()
    b.close()
    assert info.pop("workgroups") == 1
    sweeps = info.pop("assembly_sweeps", 0)
    assert info == want, (info, want)
    assert (sweeps != 0) == (cp.plan_assembly_sweeps(*q) != 0), (sweeps, info)   # (one stream group, the module loads)
    got = dict(info, assembly_sweeps=sweeps)
    assert {k: got.get(k) for k in lands} == lands, (got, lands)


def strawman(ctx, batch, bp, mode, flags, lands):
    batch = first_read(batch)
    ctx.models_clear()
    ctx.models_create([(cp.NANOPORE_TRANSITIONS, m, gx, gy) for (m, gx, gy) in batch["models"]])
    b = cp.Batch(ctx, make_items(batch, (1, 1)), batch["x_chars"], batch["events"], batch["anchors"], bp, mode,
                 cp.KERNEL_AUTO, flags)
    check(b, cp.MACHINE_STRAWMAN, mode, cp.KERNEL_AUTO, flags, signal_bands(batch, bp.diagonalExpansion), lands)


_FAMILY = {}


def family(name):
    """one read of an edge_reads family (its widest band is the family's) and its band parameters, made once"""
    if name not in _FAMILY:
        f = edge_reads.FAMILIES[name]
        batch = edge_reads.family_batch(name, n=1)
        _FAMILY[name] = (batch, band_params(0.01, f["md"], f["tb"], batch["e"]))
    return _FAMILY[name]


@pytest.mark.parametrize("narrow", [0, cp.FLAG_ASM_NARROW_BANDS], ids=["compiled", "asm-narrow"])
def test_strawman_posterior_up_to_120(ctx, narrow):
    batch, bp = family("w120")
    strawman(ctx, batch, bp, POST, narrow, dict(kernel="systolic", family="wave", cells_per_lane=2, max_band_width=120,
                                                assembly_sweeps=2 if narrow else 0))


def test_strawman_posterior_121_to_158(ctx):
    batch, bp = family("w158")
    strawman(ctx, batch, bp, POST, 0, dict(kernel="systolic", family="wave", cells_per_lane=3, max_band_width=158,
                                           assembly_sweeps=2))


def test_strawman_expectations_on_the_wave_family(ctx):
    batch, bp = family("w120")
    strawman(ctx, batch, bp, EXPECT, 0, dict(kernel="systolic", family="wave", fused_expectations=1, assembly_sweeps=0))


@pytest.mark.parametrize("fused", [0, cp.FLAG_WORKGROUP_FUSED_ESTEP], ids=["ring", "fused"])
def test_strawman_expectations_on_two_waves(ctx, fused):
    batch, bp = family("w120")
    strawman(ctx, batch, bp, EXPECT, WG | fused, dict(kernel="systolic", family="workgroup", waves_per_workgroup=2,
                                                      fused_expectations=1 if fused else 0))


@pytest.mark.parametrize("fused", [0, cp.FLAG_WIDE_BANDS_FUSED_ESTEP], ids=["ring", "fused"])
def test_strawman_expectations_on_six_waves(ctx, fused):
    batch, bp = strawman_width_batch(300)
    strawman(ctx, batch, bp, EXPECT, WIDE | fused, dict(kernel="systolic", family="workgroup", waves_per_workgroup=6,
                                                        max_band_width=300, fused_expectations=1 if fused else 0))


def test_strawman_past_504_runs_on_the_general_kernel(ctx):
    batch, bp = strawman_width_batch(505)
    strawman(ctx, batch, bp, POST, WIDE, dict(kernel="general", max_band_width=505, fused_expectations=0))


def test_vanilla_estep_on_four_waves(ctx):
    batch, bp = vanilla_width_batch(200)
    batch = first_read(batch)
    upload_vanilla(ctx, vanilla_models(batch))
    flags = cp.FLAG_WIDE_BANDS_VANILLA_ESTEP
    b = vbatch(ctx, batch, bp, (1, 1), flags | cp.FLAG_EXPECTATIONS)
    check(b, cp.MACHINE_VANILLA, EXPECT, cp.KERNEL_AUTO, flags, signal_bands(batch, bp.diagonalExpansion),
          dict(kernel="systolic", family="workgroup", waves_per_workgroup=4, max_band_width=200, fused_expectations=0))


def test_hdp_posterior_on_six_waves(ctx, nhdp):
    batch, bp = hdp_width_batch(300, "upper", (nhdp, o.HdpModel(nhdp)))
    batch = first_read(batch)
    upload_hdp(ctx, nhdp)
    flags = cp.FLAG_WIDE_BANDS_HDP
    b = hbatch(ctx, batch, bp, (1, 1), flags)
    check(b, cp.MACHINE_HDP, POST, cp.KERNEL_AUTO, flags, signal_bands(batch, bp.diagonalExpansion),
          dict(kernel="systolic", family="workgroup", waves_per_workgroup=6, max_band_width=300))


def test_dna_up_to_192(ctx):
    f = edge_reads.DNA_FAMILIES["w192"]
    case = edge_reads.dna_batch("w192", n=1)
    x, y, an = case["seqs"][0]
    bp = band_params(0.01, f["md"], f["tb"], case["e"])
    model = o.Sm5Model()
    ctx.models_clear()
    ids = ctx.models5_create([(list(model.c.t), model.match, model.gx, model.gy)])
    items = np.zeros(1, cp.ITEM_DTYPE)
    items[0] = (0, len(x), 0, len(y), 0, len(an), ids[0], 1, 1, 0)
    b = cp.Batch(ctx, items, x, None, an, bp, flags=0, y_chars=y)
    check(b, cp.MACHINE_DNA5, POST, cp.KERNEL_AUTO, 0, bands_of([(an, len(x), len(y))], case["e"]),
          dict(kernel="general", family="wave (5-state)", max_band_width=192))

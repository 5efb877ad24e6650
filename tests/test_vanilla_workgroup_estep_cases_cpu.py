"""The inputs of test_vanilla_workgroup_estep_gpu.py on the oracle alone (CPU): the nine SHAPES of
test_vanilla_workgroup_gpu and exact_width_batch at the edges of the builds, as batches of expectations.  What the GPU
test relies on and cannot see from its own side is asserted here, so that the inputs cannot drift: the widest band of
every case lies in the class its build is chosen for; every model's 61 sums are finite, the likelihood is negative and
all 60 skip bins are in use (a build that drops a bin, or a term of one, cannot pass).  At the band-edge widths some
bins are small (down to 5e-16): there the absolute part of the bar carries part of the comparison; the SHAPES and the
larger bins are where the relative part bites.

The cases and their oracle vectors are shared with the GPU test through test_band_edges_machines_gpu.cached."""
import numpy as np
import pytest

from harness import band_params
from test_band_edges_machines_gpu import cached
from test_fuzz_expectations_machines_gpu import signal_width, vanilla_oracle, vanilla_posteriors
from test_vanilla_workgroup_gpu import SHAPES, build_of, exact_width_batch, shape_batch, shape_id, vanilla_models

EDGE_WIDTHS = [184, 185, 248, 249, 376, 377, 504, 505]
# the widest band of the shapes of each build, as cpecan_band_construct gives them
SHAPE_WIDTHS = {4: (212, 232), 6: (341, 352), 8: (462, 483)}


def shape_case(shape):
    """(key, batch, models, band parameters, ragged) of one of SHAPES"""
    batch = shape_batch(shape)
    return (("ve-shape", shape["seed"]), batch, vanilla_models(batch),
            band_params(0.01, shape["md"], shape["tb"], shape["e"]), shape["ragged"])


def edge_case(width):
    """... of exact_width_batch(width): two reads, the path on the band's upper edge"""
    batch, bp = exact_width_batch(width)
    return ("ve-edge", width), batch, vanilla_models(batch), bp, (width % 2, 1)


def oracle_sums(key, batch, models, bp, ragged):
    """per-model vectors [30 beta | 30 alpha | likelihood] of the oracle's E-step, computed once per session"""
    return cached(key + ("e",), lambda: vanilla_oracle(batch, models, bp, ragged))


def oracle_posteriors(key, batch, models, bp, ragged):
    """the oracle's posterior run of every item (totals, cell counts), computed once per session"""
    return cached(key + ("post",), lambda: vanilla_posteriors(batch, models, bp, ragged))


def assert_usable(ref, what):
    for k, v in enumerate(ref):
        assert v.shape == (61,), (what, k)
        assert np.all(np.isfinite(v)) and v[60] < 0, (what, k)
        assert np.count_nonzero(v[:60]) == 60, (what, k, np.flatnonzero(v[:60] == 0))
        assert np.all(v[:60] > 0), (what, k)


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_shapes_on_the_oracle(shape):
    key, batch, models, bp, ragged = shape_case(shape)
    width = signal_width(batch, bp.diagonalExpansion)
    lo, hi = SHAPE_WIDTHS[shape["rows"]]
    assert lo <= width <= hi and build_of(width) == shape["rows"], width
    assert 1 <= len(models) <= 4 and len(models) == shape["n"]
    assert (shape["lX"] + shape["lY"]) // shape["md"] >= 3  # several traceback windows
    assert_usable(oracle_sums(key, batch, models, bp, ragged), shape_id(shape))


@pytest.mark.parametrize("width", EDGE_WIDTHS)
def test_band_edge_widths_on_the_oracle(width):
    key, batch, models, bp, ragged = edge_case(width)
    assert signal_width(batch, bp.diagonalExpansion) == width
    assert build_of(width) == {184: None, 185: 4, 248: 4, 249: 6, 376: 6, 377: 8, 504: 8, 505: None}[width]
    assert_usable(oracle_sums(key, batch, models, bp, ragged), width)

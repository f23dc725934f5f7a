"""GPU: the weight warming (csrc/warm.h) against knob 173 (MDM_VAR_NO_WARM: every Warm empty, the code before it).

A touch is a load whose value is discarded, so nothing may change: one decoder layer and a whole one-layer-per-scale denoiser
forward must be EQUAL, not close, with and without the knob, in both 16-bit modes.  Shapes of the layer (D = 512, H = 4; the hosts
are the attention cores and the query core of the cross-attention, one workgroup per (sample, head)):
    (1, 16)    4 workgroups: XCDs 4..7 have none and touch nothing, the other four each walk the prefix they reach
    (3, 50)    12 workgroups, ragged row tiles, the pair + tail launch takes riders (their weight plane is one of the ranges)
    (2, 196)   the full-scale forms (13 row tiles), 8 workgroups
The fp32-grade mode and a D = 256 model are handed no Warm at all (model.hip builds one only inside the 16-bit D = 512 cores'
branches; the library has no hook that says so, on purpose): what can be seen from outside is that the knob changes nothing."""
import ctypes as C

import pytest
import torch

from conftest import pkg
from test_blocks_gpu import _run_block, _setup
from test_route_fold_gpu import forward, inputs, model

pytestmark = pytest.mark.gpu
KNOB_NO_WARM = 173


def _with_knob(knob, fn):
    L = pkg("_lib")
    assert L.lib().mdm_set_gemm_variant(C.c_int32(knob)) == 0
    try:
        return fn()
    finally:
        L.lib().mdm_set_gemm_variant(C.c_int32(0))


def _layer_both(B, S, precision):
    m, sd, eph, proj, h, emb, xf, length, sc, pre, _ = _setup(B, S, 6, precision)
    L = pkg("_lib")
    run = lambda: _run_block(m, L.BLOCK_LAYER, h, sc, length, xf)
    return run(), _with_knob(KNOB_NO_WARM, run)


@pytest.mark.parametrize("precision", [1, 2])
@pytest.mark.parametrize("B,S", [(1, 16), (3, 50), (2, 196)])
def test_layer_is_equal_under_the_knob(B, S, precision):
    warm, plain = _layer_both(B, S, precision)
    print(f"B={B} S={S} precision {precision}: max |d| {float((warm - plain).abs().max()):.2e}")
    assert torch.isfinite(warm).all()
    assert torch.equal(warm, plain)


@pytest.mark.parametrize("precision", [1, 2])
def test_denoiser_forward_is_equal_under_the_knob(precision):
    """One decoder layer per time scale at D = 512: both scales' hosts and consumers in one forward."""
    m, _ = model(512, 8)
    inp = inputs(3, 50)
    warm, plain = forward(m, precision, inp, 0)[0], forward(m, precision, inp, KNOB_NO_WARM)[0]
    assert torch.isfinite(warm).all()
    assert torch.equal(warm, plain)


def test_fp32_grade_mode_ignores_the_knob():
    warm, plain = _layer_both(3, 50, 3)
    assert torch.isfinite(warm).all()
    assert torch.equal(warm, plain)


@pytest.mark.parametrize("precision", [1, 2])
def test_d256_ignores_the_knob(precision):
    m, _ = model(256, 8)
    inp = inputs(3, 40)
    warm, plain = forward(m, precision, inp, 0)[0], forward(m, precision, inp, KNOB_NO_WARM)[0]
    assert torch.isfinite(warm).all()
    assert torch.equal(warm, plain)

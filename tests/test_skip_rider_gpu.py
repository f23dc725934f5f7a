"""GPU: the dual block's skip projection on the idle CUs of its first Performer's pair + tail launch (riders, csrc/mlp_stream.hip
skip_rider) against the same projection as its own GEMM launch (knob 172, MDM_VAR_SKIP_LAUNCH, which is the code before the riders).

A rider puts every output element through the arithmetic of the launch it replaces (same MFMA and operand order, K ascending from
zero, gelu_erf2(acc + bias)) and the tiles are untouched, so the block output must be EQUAL, not close -- whether a shape gets
riders depends on its row count and the CU count, and a sample's result must not depend on the batch it travels in.

Which path a shape takes on 256 CUs (fused_pair_style: tile height h = mlp_stream_tile_h(M, 4), tile workgroups M / h + 1, items
ceil(M / 112), riders = min(idle CUs, items), taken if every rider has at most two items):
    (1, 5)     5 rows   h 16    1 tile wg      1 item    1 rider                 fewer rows than one row tile
    (3, 37)    111      h 16    7              1         1                       one ragged item, S no multiple of 16
    (2, 98)    196      h 16    13             2         2                       one full and one ragged item
    (5, 196)   980      h 16    62             9         9
    (48, 196)  9 408    h 48    197            84        59: two items each      (the headline shape, 64 x 196, is the other kind
                                                                                  that walks two: 197 tile wgs, 112 items, 59 riders)
    (54, 196)  10 584   h 48    221            95        35: three items -> REFUSED by the two-item rule
    (21, 195)  4 095    h 16    256            37        no idle CU -> REFUSED
The library has no hook that says which path ran (on purpose); on a device with another CU count the same assertions hold for
whatever the rule picks there."""
import ctypes as C
import functools

import pytest
import torch

from conftest import pkg
from test_blocks_gpu import R, TOL, _run_block, _setup

pytestmark = pytest.mark.gpu
KNOB_SKIP_LAUNCH = 172


def _with_knob(knob, fn):
    L = pkg("_lib")
    assert L.lib().mdm_set_gemm_variant(C.c_int32(knob)) == 0
    try:
        return fn()
    finally:
        L.lib().mdm_set_gemm_variant(C.c_int32(0))


@functools.lru_cache(maxsize=None)
def _oracle(B, S):
    """The oracle's dual block on the inputs of _setup(B, S, 6, .): they and the fp32 state dict are the same at every precision."""
    m, sd, eph, proj, h, emb, xf, length, sc, pre, (D, H, E) = _setup(B, S, 6, 1)
    with torch.no_grad():
        return R.dual_self_attention(h, emb, R.src_mask(S, length), sd, pre + ".dual_self_attn", H, eph, proj, "low.0")


def _both(B, S, precision):
    m, sd, eph, proj, h, emb, xf, length, sc, pre, _ = _setup(B, S, 6, precision)
    L = pkg("_lib")
    run = lambda: _run_block(m, L.BLOCK_DUAL, h, sc, length, xf)
    return run(), _with_knob(KNOB_SKIP_LAUNCH, run)


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("precision", [1, 2])
@pytest.mark.parametrize("B,S", [(1, 5), (3, 37), (2, 98), (5, 196), (48, 196), (54, 196)])
def test_riders_equal_the_skip_launch(B, S, precision):
    """Default path against knob 172: equal outputs, both within the block tolerance of the oracle.  (54, 196) turns out to be a
    refusal on 256 CUs (10 584 rows get 48-row tiles, not 64-row ones: 221 tile workgroups, 35 idle CUs, three items each);
    (48, 196) is the shape of its kind at which a rider does walk two items."""
    rode, launch = _both(B, S, precision)
    ref = _oracle(B, S)
    e_r, e_l = _rel(rode, ref), _rel(launch, ref)
    print(f"B={B} S={S} precision {precision}: default vs knob 172 max |d| {float((rode - launch).abs().max()):.2e}; vs oracle {e_r:.2e} / {e_l:.2e}")
    assert torch.isfinite(rode).all()
    assert torch.equal(rode, launch)
    assert e_r < TOL[precision] and e_l < TOL[precision]


@pytest.mark.parametrize("precision", [1, 2])
def test_refused_where_no_cu_is_idle(precision):
    """4 095 rows: 16-row tiles, 256 tile workgroups, no idle CU -- the riders are refused and the skip projection is launched
    behind the first Performer; the same output as knob 172 (the launch in front of it), and it runs."""
    B, S = 21, 195
    rode, launch = _both(B, S, precision)
    ref = _oracle(B, S)
    assert torch.isfinite(rode).all()
    assert torch.equal(rode, launch)
    assert _rel(rode, ref) < TOL[precision]


def test_fp32_grade_mode_ignores_the_knob():
    """Precision 3 takes DualTail::T3: the skip projection stays a launch whatever the knob says."""
    rode, launch = _both(2, 98, 3)
    assert torch.isfinite(rode).all()
    assert torch.equal(rode, launch)
    assert _rel(rode, _oracle(2, 98)) < TOL[3]


@pytest.mark.parametrize("precision", [1, 2])
def test_d256_ignores_the_knob(precision):
    """D = 256 has no pair + tail launch (DualTail::NONE): the whole denoiser forward is the same with and without the knob."""
    T_, synth = pkg("transformer"), pkg("synth")
    feats, ntext, dt, D, H, B, T = 8, 6, 64, 256, 4, 3, 40
    m = T_.MotionTransformer(feats, num_frames=64, latent_dim=D, ff_size=2 * D, num_layers=1, num_heads=H, text_latent_dim=dt,
                             moe_num_experts=8, precision=precision)
    m.load_state_dict(synth.synth_state_dict(m._layout, 5), strict=True)
    m.set_ephemerals(synth.synth_ephemerals(D, dt, 1, 7)), m.set_projections(synth.synth_projections(D // H, 1, 7))
    m = m.cuda().eval()
    x, t, length, xf_proj, xf_out = (v.cuda() for v in synth.synth_inputs(B, T, feats, ntext, dt, 11, min_len=4))

    def run():
        with torch.no_grad():
            out = m(x, t, length, xf_proj=xf_proj, xf_out=xf_out)
        torch.cuda.synchronize()
        return out.cpu()
    a, b = run(), _with_knob(KNOB_SKIP_LAUNCH, run)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b)

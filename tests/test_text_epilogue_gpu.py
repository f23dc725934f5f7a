"""GPU: the folded text cross-attention in the epilogue of the MoE block's stylization launch (TextPath::EPILOGUE, the TX form of
csrc/style_gemm.hip) against the same work as a launch of its own (knob 174, MDM_VAR_TEXT_LAUNCH, which is the code before it).

The epilogue puts every element through sd_fold_kernel's arithmetic -- the same MFMAs with the text fragment first, K ascending
in steps of 32, the same softmax grouping and LayerNorm reduction order -- on the 16-bit rows the launch would have written for
it, and the stylization rows themselves do not depend on the tile they sit in.  So the layer / denoiser output must be EQUAL, not
close, and both must sit within the block tolerance of the oracle (TOL of tests/test_blocks_gpu.py; routing injected from the
oracle, as there).

Tiles follow the sample: ceil(S / 32) tiles of ceil(S / tiles) rows.
    (B, S)     tiles per sample
    (1, 5)     5                        fewer rows than a row tile
    (2, 33)    17 / 16                  a second row tile (rows 16 ..) with one valid row
    (3, 37)    19 / 18                  S no multiple of 16
    (2, 98)    25 / 25 / 24 / 24        the coarse split of the benchmark shape
    (3, 196)   7 x 28                   the full scale: the FFN pair in one launch behind it
Text tokens N (H = 4 heads, passes of whole heads in <= 128 columns): 6 and 28 one pass (112 of 128 columns at 28), 32 all 128
columns, 40 two passes of 3 + 1 heads, 64 two passes of 2 + 2; 85 takes four passes, which stay on the GEMM chain."""
import ctypes as C
import functools

import pytest
import torch

from conftest import build_module, load_golden, pkg
from test_blocks_gpu import R, TOL, _run_block, _setup

pytestmark = pytest.mark.gpu
KNOB_TEXT_LAUNCH = 174
SHAPES = [(1, 5), (2, 33), (3, 37), (2, 98), (3, 196)]
TOKENS = [6, 28, 32, 40, 64]
# each S with the benchmark's N, each N with the benchmark's coarse shape
CASES = [(B, S, 28) for B, S in SHAPES] + [(2, 98, N) for N in TOKENS if N != 28]


def _with_knob(knob, fn):
    L = pkg("_lib")
    assert L.lib().mdm_set_gemm_variant(C.c_int32(knob)) == 0
    try:
        return fn()
    finally:
        L.lib().mdm_set_gemm_variant(C.c_int32(0))


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@functools.lru_cache(maxsize=None)
def _oracle(B, S, N, counts=None):
    """The oracle's decoder layer on the inputs of _setup(B, S, N, .) (the same at every precision) and its routing, (2, M, 2).
    counts: every sample alone on its own first counts[b] text tokens (the reference has no text mask)."""
    m, sd, eph, proj, h, emb, xf, length, sc, pre, (D, H, E) = _setup(B, S, N, 1)
    refs, idx = [], []
    with torch.no_grad():
        for sl, n in ([(slice(0, B), N)] if counts is None else [(slice(b, b + 1), n) for b, n in enumerate(counts)]):
            trace = {}
            refs.append(R.decoder_layer(h[sl], xf[sl, :n], emb[sl], R.src_mask(S, length[sl]), sd, pre, H, E, eph, proj, "low.0", None, trace))
            idx.append(torch.stack([trace[f"{pre}.ffn.branches.{b}.top2_idx"] for b in range(2)]))
    return torch.cat(refs), torch.cat(idx, 1)


def _layer_both(B, S, N, precision, counts=None):
    m, sd, eph, proj, h, emb, xf, length, sc, pre, _ = _setup(B, S, N, precision)
    ref, forced = _oracle(B, S, N, counts)
    L = pkg("_lib")
    run = lambda: _run_block(m, L.BLOCK_LAYER, h, sc, length, xf, forced if precision in (1, 2) else None,
                             ntok=None if counts is None else list(counts))
    return run(), _with_knob(KNOB_TEXT_LAUNCH, run), ref


@pytest.mark.parametrize("precision", [1, 2])
@pytest.mark.parametrize("B,S,N", CASES)
def test_layer_equals_the_text_launch(B, S, N, precision):
    fold, launch, ref = _layer_both(B, S, N, precision)
    e_f, e_l = _rel(fold, ref), _rel(launch, ref)
    print(f"B={B} S={S} N={N} precision {precision}: default vs knob 174 max |d| {float((fold - launch).abs().max()):.2e}; "
          f"vs oracle {e_f:.2e} / {e_l:.2e}")
    assert torch.isfinite(fold).all()
    assert torch.equal(fold, launch)
    assert e_f < TOL[precision] and e_l < TOL[precision]


@pytest.mark.parametrize("precision", [1, 2])
def test_per_sample_token_counts(precision):
    """A batch whose second sample carries a shorter caption (the conditional | empty-caption rows of guided sampling): the counts
    live in the folded bias (sd_fold_mask_cb), which the epilogue reads as the launch does.  The oracle runs every sample alone
    on its own tokens."""
    B, S, N, counts = 2, 98, 28, (28, 9)
    fold, launch, ref = _layer_both(B, S, N, precision, counts)
    e_f, e_l = _rel(fold, ref), _rel(launch, ref)
    print(f"counts {counts} precision {precision}: vs oracle {e_f:.2e} / {e_l:.2e}")
    assert torch.isfinite(fold).all()
    assert torch.equal(fold, launch)
    assert e_f < TOL[precision] and e_l < TOL[precision]
    full = _layer_both(B, S, N, precision)[0]
    assert not torch.equal(full[1], fold[1])  # the counts are applied


@pytest.mark.parametrize("precision", [1, 2])
@pytest.mark.parametrize("B,T,N", [(2, 196, 28), (3, 66, 28), (2, 74, 40)])
def test_denoiser_forward_equals_the_text_launch(B, T, N, precision):
    """One decoder layer per time scale at D = 512: the coarse layer at T / 2 frames (98: 25 / 25 / 24 / 24; 33: 17 / 16; 37: 19 /
    18 in two passes) and the full-scale layer at T (7 x 28; 3 x 22; 25 / 25 / 24) in one forward, free routing."""
    synth = pkg("synth")
    g, meta = load_golden("fwd_small_dims")
    m, _ = build_module(meta, precision=precision)
    seed = 300 + B + T + N
    x = (synth.uniform_pm1((B, T, 263), "text.x", seed) * (3.0 ** 0.5)).cuda()
    xf_out = (synth.uniform_pm1((B, N, 256), "text.xf", seed) * (3.0 ** 0.5)).cuda()
    ts = torch.tensor([999, 500, 17][:B]).cuda()
    length = torch.tensor([T, max(1, T - 27), T][:B]).cuda()

    def run():
        with torch.no_grad():
            out = m(x, ts, length, xf_proj=xf_out.mean(1), xf_out=xf_out)
        torch.cuda.synchronize()
        return out.cpu()
    fold, launch = run(), _with_knob(KNOB_TEXT_LAUNCH, run)
    assert torch.isfinite(fold).all()
    assert torch.equal(fold, launch)


def test_fp32_grade_mode_ignores_the_knob():
    """Precision 3 has no 16-bit stylization launch in the MoE block: sd_path() is not the fold, nothing to move."""
    fold, launch, ref = _layer_both(2, 98, 28, 3)
    assert torch.isfinite(fold).all()
    assert torch.equal(fold, launch)
    assert _rel(fold, ref) < TOL[3]


@pytest.mark.parametrize("precision", [1, 2])
def test_four_passes_stay_on_the_chain(precision):
    """N = 85 (the reference's padded caption): four passes, where the GEMM chain is taken instead of the fold -- unaffected."""
    fold, launch, ref = _layer_both(2, 98, 85, precision)
    assert torch.isfinite(fold).all()
    assert torch.equal(fold, launch)
    assert _rel(fold, ref) < TOL[precision]

"""CPU: tests/moe_block_ref.py (the fp64 reference of the MoE block tests) against oracle/denoiser_ref.py, which the
reference-generated goldens pin, and the routing margin it derives on the shapes the GPU tests use."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, golden_state, load_golden, pkg, rel_inf

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import denoiser_ref as R  # noqa: E402
import moe_block_ref as MB  # noqa: E402


def test_fp32_restatement_equals_the_oracle_block_with_the_same_decisions():
    g, meta = load_golden("fwd_small_dims")
    sd, eph, proj, mcfg = golden_state(meta)
    D, E, B, S = mcfg["latent_dim"], mcfg["moe_num_experts"], 2, 37
    synth = pkg("synth")
    h = synth.uniform_pm1((B, S, D), "blk.h", S) * 1.5
    emb = synth.uniform_pm1((B, D), "blk.emb", S)
    sp = MB.PRE + ".proj_out"
    w, b = eph["low.0.ffn_style"]
    sc = F.linear(F.silu(F.linear(emb, w, b)), sd[sp + ".emb_layers.1.weight"], sd[sp + ".emb_layers.1.bias"])
    trace = {}
    with torch.no_grad():
        want = R.moe_ffn(h, emb, sd, MB.PRE, E, eph["low.0.ffn_style"], None, trace)
        got, info = MB.moe_block(h, sc, sd, E)
    assert rel_inf(got, want) < 2e-6
    for br in range(2):
        assert torch.equal(info[br]["idx"], trace[f"{MB.PRE}.branches.{br}.top2_idx"])
        assert torch.equal(info[br]["vals"], trace[f"{MB.PRE}.branches.{br}.top2_val"])
        assert torch.equal(info[br]["usage"], trace[f"{MB.PRE}.branches.{br}.usage"])
        assert rel_inf(info[br]["importance"], trace[f"{MB.PRE}.branches.{br}.importance"]) < 1e-6
    # forced indices (a token sent twice to one expert included) go the same way through both
    forced = torch.stack([info[1]["idx"], info[0]["idx"]])
    forced[0, 5] = forced[0, 5, 0]
    with torch.no_grad():
        want = R.moe_ffn(h, emb, sd, MB.PRE, E, eph["low.0.ffn_style"], forced, None)
        got, _ = MB.moe_block(h, sc, sd, E, forced)
        got64, _ = MB.moe_block(h.double(), sc.double(), MB.cast_state(sd, torch.float64), E, forced)
    assert rel_inf(got, want) < 2e-6 and rel_inf(got64, want) < 1e-5


def test_top2_names_the_lowest_indices_on_ties():
    p = torch.tensor([[.2, .3, .3, .2], [.25, .25, .25, .25], [.1, .4, .1, .4], [.4, .2, .2, .2]], dtype=torch.float64)
    _, idx = MB.top2_lowest_index_first(p)
    assert idx.tolist() == [[1, 2], [0, 1], [1, 3], [0, 1]]
    _, want = R.top2_lowest_index_first(p)
    assert torch.equal(idx, want)


@pytest.mark.parametrize("D,H,E", [(64, 4, 4), (128, 4, 5), (256, 4, 2), (320, 5, 6), (192, 3, 3), (768, 6, 11), (512, 4, 8), (512, 4, 7),
                                   (1024, 4, 16), (1024, 4, 9)])
def test_the_derived_margin_leaves_out_at_most_half_a_percent(D, H, E):
    """The condition of the GPU routing test, on the reference alone: with the seed and the rows that test uses, the tokens whose
    fp64 top-3 logits lie closer than 8 x the fp32 restatement's logit error are at most 0.5 % per branch."""
    sd = MB.block_state(D, H, 4 * D, E, MB_SEED, experts=False)
    sd64 = MB.cast_state(sd, torch.float64)
    h, _, _ = MB.block_inputs(16, 256, D, MB_SEED)
    for br in range(2):
        margin, l64 = MB.routing_margin(h, sd, sd64, br)
        out = int((MB.top3_gap(l64) < margin).sum())
        print(f"D={D} E={E} branch {br}: margin {margin:.2e}, {out}/4096 under it")
        assert 0 < margin < 1e-4 and out <= 0.005 * 4096


MB_SEED = 3

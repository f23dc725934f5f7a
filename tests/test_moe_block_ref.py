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


# ---------------------------------------------------------------------------------------------------------------------
# the fp8 mode's staged reference: e4m3 helpers, and a torch emulation of the chain that must pass it and, with a seeded
# fault, fail exactly the stage the fault is in
# ---------------------------------------------------------------------------------------------------------------------
def test_e4m3_decode_table_is_torchs():
    b = torch.arange(256, dtype=torch.uint8)
    got, want = MB.e4m3_decode(b), b.view(torch.float8_e4m3fn).double()
    nan = torch.isnan(want)
    assert b[nan].tolist() == [0x7F, 0xFF] and torch.equal(torch.isnan(got), nan)
    assert torch.equal(got[~nan], want[~nan]) and float(got[~nan].max()) == 448.0 and float(got[~nan].min()) == -448.0
    assert MB.e4m3_nan_bytes(b) == 2


def test_e4m3_half_step_property_of_torchs_quantiser():
    """|q - v| <= e4m3_step(v) / 2 for torch's nearest-even conversion over +-448, subnormals and zero included, and the bound
    is nearly attained (so it is no wider than the format's)."""
    g = torch.Generator().manual_seed(0)
    v = torch.cat([(torch.rand(100000, generator=g, dtype=torch.float64) * 2 - 1) * 448,
                   (torch.rand(50000, generator=g, dtype=torch.float64) * 2 - 1) * 2.0 ** -5,  # the subnormal range, |v| < 2^-6, and the binade above
                   (torch.rand(50000, generator=g, dtype=torch.float64) * 2 - 1),
                   torch.tensor([0.0, 448.0, -448.0, 2.0 ** -9, 2.0 ** -10, 2.0 ** -6, 1.0, 256.0])]).float().double()
    q = MB.e4m3_decode(v.float().to(torch.float8_e4m3fn).view(torch.uint8))
    ratio = (q - v).abs() / MB.e4m3_step(v)
    print(f"worst |q - v| / step over {v.numel()} values: {float(ratio.max()):.6f}")
    assert float(ratio.max()) <= 0.5 and float(ratio.max()) > 0.49
    assert MB.e4m3_step(torch.tensor([0.0, 2.0 ** -9, 0.01, 1.0, 1.9, 300.0, 448.0])).tolist() == [2.0 ** -9, 2.0 ** -9, 2.0 ** -9, 0.125, 0.125, 32.0, 32.0]


def _rne8(v):
    return v.float().to(torch.float8_e4m3fn).view(torch.uint8)


def _trunc8(v):
    """e4m3 by truncation toward zero: nearest-even, one code down wherever that rounded away from zero."""
    q = _rne8(v)
    return torch.where(MB.e4m3_decode(q).abs() > v.abs().double(), q - 1, q)


def _assign(idx, vals, E):
    """A slab assignment of decisions idx (2, M, 2) with probabilities vals: perm, goff, pos4, rowscale as the router leaves them
    (tests/test_route_fold_gpu.py check_assignment), entries in (branch, token, k) order inside a slab."""
    M = idx.shape[1]
    group = (idx + E * torch.arange(2)[:, None, None]).reshape(-1)
    order = torch.sort(group, stable=True).indices  # slab row -> entry
    goff = torch.cat([torch.zeros(1, dtype=torch.int64), torch.bincount(group, minlength=2 * E).cumsum(0)])
    row_of = (torch.arange(2)[:, None] * M + torch.arange(M)[None, :])[:, :, None].expand(2, M, 2).reshape(-1)
    pos = torch.empty(4 * M, dtype=torch.int64)
    pos[order] = torch.arange(4 * M)
    return row_of[order], goff, pos.reshape(2, M, 2).permute(1, 0, 2).reshape(M, 4), vals.reshape(-1)[order]


FP8_SHAPE, FP8_TOKENS = (128, 4, 256, 5), (2, 37)
FAULTS = {"rows converted by truncation": 1, "hidden layer converted by truncation": 2, "activation scale by slab position": 2,
          "first GEMM's channel scales of the group before": 2, "second GEMM's channel scales of the group before": 3,
          "hidden scale 4 with inverse 1/8": 2}
_FP8_CASE = {}


def _fp8_case():
    if not _FP8_CASE:
        D, H, Fd, E = FP8_SHAPE
        sd = MB.block_state(D, H, Fd, E, MB_SEED)
        sd64 = MB.cast_state(sd, torch.float64)
        h, sc, _ = MB.block_inputs(*FP8_TOKENS, D, MB_SEED)
        with torch.no_grad():
            _, info = MB.moe_block(h.double(), sc.double(), sd64, E)
        _FP8_CASE.update(sd=sd, sd64=sd64, h=h, sc=sc, idx=torch.stack([i["idx"] for i in info]), e_ln=MB.ln_margin(h, sd, sd64))
    return _FP8_CASE


def _emulate(fault=None):
    """The fp8 mode's chain in torch: fp32 LayerNorm, amax / 448 scales, torch e4m3 casts, fp32 matmuls, the x 8 hidden scale, an
    fp16 y2, an fp32 tail; the fp64 reference's decisions.  Returns (dev, wq) as MB.fp8_block_stages takes them."""
    c = _fp8_case()
    D, H, Fd, E = FP8_SHAPE
    sd, h, sc, idx = c["sd"], c["h"], c["sc"], c["idx"]
    B, S = FP8_TOKENS
    M = B * S
    vals = torch.stack([F.softmax(MB.gate_logits(h, sd, br), dim=1).gather(1, idx[br]) for br in range(2)])
    perm, goff, pos4, rowscale = _assign(idx, vals, E)
    h32 = torch.stack([MB._ln(h, sd, f"{MB.PRE}.branches.{br}.layernorm").reshape(M, D) for br in range(2)])
    x8, s = MB.quantize_rows_e4m3(h32)
    if fault == "rows converted by truncation":
        x8 = _trunc8(h32 * (1.0 / s)[..., None])
    stack = lambda leaf: torch.stack([sd[f"{MB.PRE}.branches.{g // E}.moe.experts.{g % E}.{leaf}"] for g in range(2 * E)])
    (w1q, w1s), (w2q, w2s) = MB.quantize_rows_e4m3(stack("0.weight")), MB.quantize_rows_e4m3(stack("2.weight"))
    b1, b2 = stack("0.bias"), stack("2.bias")
    srow = s.reshape(-1)[torch.arange(4 * M) % (2 * M) if fault == "activation scale by slab position" else perm]
    a8 = MB.e4m3_decode(x8).float().reshape(2 * M, D)[perm]
    hs = 4.0 if fault == "hidden scale 4 with inverse 1/8" else 8.0
    hid, y2 = torch.zeros((4 * M, Fd), dtype=torch.uint8), torch.zeros((4 * M, D), dtype=torch.float16)
    for g in range(2 * E):
        lo, hi = int(goff[g]), int(goff[g + 1])
        g1 = (g - 1) % (2 * E) if fault == "first GEMM's channel scales of the group before" else g
        g2 = (g - 1) % (2 * E) if fault == "second GEMM's channel scales of the group before" else g
        v = hs * F.gelu((a8[lo:hi] @ MB.e4m3_decode(w1q[g]).float().T) * srow[lo:hi, None] * w1s[g1][None, :] + b1[g])
        hid[lo:hi] = (_trunc8 if fault == "hidden layer converted by truncation" else _rne8)(v.clamp(-448, 448))
        y = ((MB.e4m3_decode(hid[lo:hi]).float() @ MB.e4m3_decode(w2q[g]).float().T) * 0.125 * w2s[g2][None, :] + b2[g]) * rowscale[lo:hi, None]
        y2[lo:hi] = y.half()
    out = MB.block_tail(h, (0.5 * y2.float()[pos4].sum(1)).view(B, S, D), sc, sd)
    return dict(x8=x8, s=s, perm=perm, goff=goff, pos4=pos4, rowscale=rowscale, hid=hid, y2=y2, out=out), dict(w1q=w1q, w1s=w1s, w2q=w2q, w2s=w2s)


def _stages(fault=None):
    c = _fp8_case()
    with torch.no_grad():
        dev, wq = _emulate(fault)
        checks, _ = MB.fp8_block_stages(c["h"].double(), c["sc"].double(), c["sd64"], FP8_SHAPE[3], c["e_ln"], dev, wq)
    for k in checks:
        print(f"{fault or 'no fault'}: stage {k.stage} {k.what}: {'ok' if k.ok else 'FAILS'} (worst {k.worst:.3g})")
    return checks


def test_fp8_stage_bounds_are_satisfiable_by_a_torch_emulation():
    checks = _stages()
    assert sorted({k.stage for k in checks}) == [1, 2, 3, 4] and MB.failed_stages(checks) == []
    assert 0 < _fp8_case()["e_ln"] < 1e-4


@pytest.mark.parametrize("fault", list(FAULTS))
def test_fp8_stage_checks_fail_the_stage_of_a_seeded_fault(fault):
    """Every stage is checked on what the stage before it left, so a fault shows in its own stage and in no other."""
    assert MB.failed_stages(_stages(fault)) == [FAULTS[fault]]

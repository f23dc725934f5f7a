"""GPU: the MoE block in the fp8 mode (precision 5: the fp16 flow with e4m3 expert GEMMs) through mdm_block_forward(MDM_BLOCK_MOE)
with forced routing, judged STAGE BY STAGE: after the run the test reads what every stage left in the workspace
(mdm_route_workspace, mdm_expert_workspace) and compares it with fp64 arithmetic applied to the device's own output of the stage
before it (tests/moe_block_ref.py fp8_block_stages).  No end-to-end tolerance: every bound is a rounding property or a gate the
project already uses.

  1. router rows: the e4m3 rows X8 and their scales s against the fp64 LayerNorm h64 of each branch.  e_LN = 8 x the largest
     |fp32 restatement - fp64| of the branch LayerNorms over the case (moe_block_ref.ln_margin, the construction of routing_margin).
       |s - amax64 / 448| <= 2^-21 s + e_LN / 448;   |decode(X8) s - h64| <= s step(|h64| / s + e_LN / s) / 2 + e_LN;
       no NaN byte; every row's largest decoded magnitude is exactly 448.
  2. GEMM1 on the device's X8 and s: v64 = 8 GELU((decode(X8) s)[perm] W1q_g^T + b1_g) per slab of goff, e = 2e-5 max |v64| (the
     kernel's gate on quantised operands in tests/test_fp8_gpu.py):
       |decode(hid) - clamp(v64, +-448)| <= step(min(|v64| + e, 448)) / 2 + e;   no NaN byte.
  3. GEMM2 on the device's hid: y64 = rowscale ((decode(hid) / 8) W2q_g^T + b2_g):
       |y2 - y64| <= 2^-11 |y64| + 2^-25 + 2e-5 max |y64|   (fp16 nearest rounding, normal and subnormal, and the kernel's gate).
  4. tail on the device's y2: mean over pos4, stylization, residual in fp64; rel_inf < 6e-3, the fp16 mode's gate (TOL[2] of
     tests/test_moe_block_gpu.py), because this part is the fp16 mode's code.
step(v) = 2 ** (max(floor(log2 |v|), -6) - 3) is the e4m3 spacing (tests/test_moe_block_ref.py holds it to torch's quantiser, and
holds the four checks to a torch emulation of the chain with and without seeded faults).  The slab assignment (perm / goff / pos4 /
rowscale) is verified by check_assignment of tests/test_route_fold_gpu.py before it is used, and the expert weights' e4m3 images
and channel scales are asserted byte-equal to torch's conversion under amax / 448.  Rows of hid and y2 at or past goff[2E] enter
no check.

Reported, not gated: the block output against the UNQUANTISED fp64 block with the same decisions.  Measured on MI355X
(rel_inf, tokens 74 / 2404):
  (128, 4, 256, 5)     3.77e-02 / 4.25e-02      (768, 6, 1024, 11)   3.86e-02 / 3.67e-02      (1024, 4, 2048, 16)  3.61e-02 / 4.15e-02
  (256, 4, 512, 2)     3.82e-02 / 3.90e-02      (512, 4, 1024, 8)    4.22e-02 / 3.96e-02      (1024, 4, 2048, 9)   4.20e-02 / 3.83e-02
  (512, 4, 1024, 8) skewed table 4.28e-02; (1024, 4, 2048, 16) slabs of 1 / 127 / 128 / 129 rows 3.96e-02; (256, 4, 512, 2) with
  expert 0's first Linear x 64 (max |v64| 2355, clamped at 448) 2.58e-01.  Worst err / bound per stage over all cases: row scales
  0.14, rows 1.00 (e4m3 near-ties sit at the half step), hidden layer 0.999 (the same), expert outputs 0.95, tail 0.047.
Before the row kernel wrote e4m3 rows (D = 768 took moe_gate_kernel, which stored bf16 rows and no scales), the (768, 6, 1024, 11)
case at 74 tokens failed all four checks of stage 1 (288 NaN bytes, scales 7e7 bounds off) and stage 2, with a finite block output
at rel err 1.06 against the unquantised fp64 block -- nothing the suite looked at before.
"""
import ctypes as C
import os
import sys

import pytest
import torch

from conftest import ROOT, pkg, rel_inf

sys.path.insert(0, os.path.join(ROOT, "tests"))
import moe_block_ref as MB  # noqa: E402
from test_moe_block_gpu import SEED, SHAPES, _grouped, accepted, block, free_case, tag  # noqa: E402
from test_route_fold_gpu import check_assignment, read_route  # noqa: E402

pytestmark = pytest.mark.gpu
PREC = 5
FP8_SHAPES = [s for s in SHAPES if accepted(s, PREC)]
TOKENS = [(2, 37), (4, 601)]  # every slab inside one 128-row tile / slabs of several tiles with a ragged last one
_ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def test_the_shapes_are_the_ones_the_fp8_mode_admits():
    """The run-time-E LDS-staged router (D = 128, 256; E = 9 at D = 1024), the constant-E one (E = 8 / 16 at D = 512 / 1024), the row
    kernel's width (D = 768), E = 2."""
    assert FP8_SHAPES == [(128, 4, 256, 5), (256, 4, 512, 2), (768, 6, 1024, 11), (512, 4, 1024, 8), (1024, 4, 2048, 16), (1024, 4, 2048, 9)]


def read_stages(bk, ws, B, S):
    """What the block left in workspace ws: the verified slab assignment, the router's e4m3 rows and scales, hid, y2 (GPU tensors)."""
    L = pkg("_lib")
    M, D, Fd, E = B * S, bk.D, bk.F, bk.E
    r = read_route(bk.m, ws, B, S, 1, M, True)
    check_assignment(r, M, E, f"D={D} E={E} tokens {M}")
    off = (C.c_int64 * 3)()
    L.check(L.lib().mdm_expert_workspace(C.byref(bk.m.pack().model), C.c_int32(B), C.c_int32(S), C.c_int32(1), off))
    take = lambda o, nbytes, dt: ws[o:o + nbytes].clone().view(dt)
    x8 = r["hn"].reshape(-1).view(torch.uint8)[:2 * M * D].reshape(2, M, D)  # slot 0 of the route aid, as bytes
    dev = dict(x8=x8, s=take(off[0], 2 * M * 4, torch.float32).reshape(2, M), hid=take(off[1], 4 * M * Fd, torch.uint8).reshape(4 * M, Fd),
               y2=take(off[2], 4 * M * D * 2, torch.float16).reshape(4 * M, D), perm=r["perm"], goff=r["goff"], pos4=r["pos4"],
               rowscale=r["rowscale"])
    return dev, r


def packed_experts(bk):
    """The e4m3 images and channel scales of the expert matrices in the model's pack, byte-equal to torch's conversion of the same
    fp32 matrices under amax / 448."""
    pm = bk.m.pack()
    D, Fd, E = bk.D, bk.F, bk.E
    wq = {}
    for leaf, key, shape in (("w1", "0.weight", (2 * E, Fd, D)), ("w2", "2.weight", (2 * E, D, Fd))):
        w = pm.W["L0." + leaf]
        assert w.fmt == "f8" and w.Kp == shape[2] and tuple(w.hi.shape) == (shape[0] * shape[1], shape[2])
        src = torch.stack([bk.sd64[f"{MB.PRE}.branches.{g // E}.moe.experts.{g % E}.{key}"] for g in range(2 * E)]).float()
        q, s = MB.quantize_rows_e4m3(src)
        assert torch.equal(w.lo.reshape(shape[:2]), s), (leaf, "channel scales")
        assert torch.equal(w.hi.reshape(shape), q), (leaf, "e4m3 image", int((w.hi.reshape(shape) != q).sum()))
        wq[leaf + "q"], wq[leaf + "s"] = w.hi.reshape(shape), w.lo.reshape(shape[:2])
    return wq


def staged_case(shape, B, S, forced=None, what="reference routing"):
    """One run of the block at precision 5 with the given decisions (None: the fp64 reference's own), all four stages asserted."""
    bk = block(shape)
    h, sc, length = MB.block_inputs(B, S, shape[0], SEED)
    if forced is None:
        _, info = bk.reference(h, sc)
        forced = torch.stack([info[br]["idx"].cpu() for br in range(2)])
    ref, _ = bk.reference(h, sc, forced)
    out, idx, ws = bk.run(PREC, h, sc, length, forced, dump=True, workspace=True)
    assert torch.equal(idx, forced.long())
    dev, r = read_stages(bk, ws, B, S)
    assert torch.equal(r["top_idx"], forced.long())
    dev["out"] = out
    e_ln = MB.ln_margin(h, bk.r32, bk.r64)
    with torch.no_grad():
        checks, vals = MB.fp8_block_stages(h.double().cuda(), sc.double().cuda(), bk.sd64, bk.E, e_ln, dev, packed_experts(bk))
    sizes = (r["goff"][1:] - r["goff"][:-1]).tolist()
    print(f"{tag(shape, PREC, B, S)} [{what}]: e_LN {e_ln:.2e}, slabs {min(sizes)} .. {max(sizes)} rows ({sizes.count(0)} empty), "
          f"max |v64| {float(vals['v64'].abs().max()):.1f}; vs the unquantised fp64 block: rel err {rel_inf(out, ref):.2e}")
    for k in checks:
        print(f"    stage {k.stage} {k.what}: {'ok' if k.ok else 'FAILS'}, worst err / bound {k.worst:.3g}")
    assert torch.isfinite(out).all()
    assert sorted({k.stage for k in checks}) == [1, 2, 3, 4]
    assert all(k.ok for k in checks), (shape, B, S, what, [k for k in checks if not k.ok])
    return sizes, vals


@pytest.mark.parametrize("B,S", TOKENS)
@pytest.mark.parametrize("shape", FP8_SHAPES, ids=_ids)
def test_every_stage_matches_fp64_on_the_device_operands(shape, B, S):
    sizes, _ = staged_case(shape, B, S)
    if (B, S) == (2, 37):  # (with this seed no slab is empty here, E = 16 included: the two hand-built tables below hold the empty ones)
        assert max(sizes) <= 128
    else:
        assert max(sizes) > 128 and any(n % 128 for n in sizes)


def test_skewed_routing_with_empty_slabs_at_both_ends():
    """Branch 0 all to experts (0, 1), branch 1 all to (E - 1, E - 2): four slabs of M rows; empty slabs in a run of E - 2 behind the
    first two (the trailing ones of branch 0), and in a run of E - 2 in front of the last two (the leading ones of branch 1)."""
    shape = (512, 4, 1024, 8)
    E, (B, S) = shape[3], TOKENS[1]
    M = B * S
    forced = torch.stack([torch.tensor([0, 1]).expand(M, 2), torch.tensor([E - 1, E - 2]).expand(M, 2)]).clone()
    sizes, _ = staged_case(shape, B, S, forced, "branch 0 to (0, 1), branch 1 to (E-1, E-2)")
    assert sizes == [M, M] + [0] * (2 * E - 4) + [M, M]


def test_slabs_of_1_127_128_and_129_rows():
    """The 128-row tile of the fp8 GEMM: slabs one row long, one under, at and one over the tile, in both branches."""
    shape = (1024, 4, 2048, 16)
    B, S = TOKENS[1]
    sizes, _ = staged_case(shape, B, S, _grouped(B * S, shape[3], [[1, 127, 128, 129], [129, 128, 127, 1]]), "slabs of 1, 127, 128, 129 rows")
    assert sizes[:8] == [1, 1, 127, 127, 128, 128, 129, 129] and sizes[16:24] == [129, 129, 128, 128, 127, 127, 1, 1]


def test_hidden_layer_saturates_at_448_inside_the_block():
    """Expert 0's first Linear (weight and bias, both branches) scaled by 64: its hidden units leave e4m3's range at the static
    scale 8, the kernel clamps them to +-448 (no NaN byte), and stages 2 - 4 hold with the clamp."""
    shape = (256, 4, 512, 2)
    B, S = TOKENS[0]
    bk = block(shape)
    keys = [f"{MB.PRE}.branches.{br}.moe.experts.0.0.{leaf}" for br in range(2) for leaf in ("weight", "bias")]
    pristine = {k: bk.sd64[k].float().cpu() for k in keys}
    big = {k: v * 64.0 for k, v in pristine.items()}
    try:
        bk.m.load_state_dict(big, strict=False)
        bk.sd64.update(MB.cast_state(big, torch.float64, "cuda"))
        h, sc, _ = MB.block_inputs(B, S, shape[0], SEED)
        with torch.no_grad():  # from the reference alone: the unquantised fp64 hidden layer of expert 0 leaves the range
            v_ref = max(float((8 * torch.nn.functional.gelu(MB._lin(MB._ln(h.double().cuda(), bk.sd64, f"{MB.PRE}.branches.{br}.layernorm"), bk.sd64,
                                                                    f"{MB.PRE}.branches.{br}.moe.experts.0.0"))).abs().max()) for br in range(2))
        assert v_ref > 464, ("choose another factor", v_ref)
        forced = torch.tensor([0, 1]).expand(2, B * S, 2).clone()  # every token meets the scaled expert
        _, vals = staged_case(shape, B, S, forced, "expert 0's first Linear x 64")
        assert float(vals["v64"].abs().max()) > 464
    finally:
        bk.m.load_state_dict(pristine, strict=False)
        bk.sd64.update(MB.cast_state(pristine, torch.float64, "cuda"))


@pytest.mark.parametrize("shape", [s for s in FP8_SHAPES if not (s[0] in (512, 1024) and s[3] in (8, 16))], ids=_ids)
def test_router_decisions_equal_fp64_outside_the_margin_in_the_fp8_mode(shape):
    """The free-routing check of tests/test_moe_block_gpu.py at precision 5 for the shapes its own test does not run in this mode
    (it runs the constant-E ones): the router writes e4m3 rows there, its decisions stay the fp32 ones."""
    free_case(shape, PREC, 8, 512)

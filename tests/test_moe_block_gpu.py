"""GPU: the MoE inference block (router, offsets, assign, expert MLPs, stylization tail) through mdm_block_forward(MDM_BLOCK_MOE)
against the fp64 restatement of tests/moe_block_ref.py, across the widths, expert counts, routing skews and token counts that
include/mdm_hip.h admits.  Weights are the block's own sub-state (seeded), the module is a one-layer MotionTransformer of that
width called at the block entry point.

Tolerances: the project's per-mode gates (TOL, as tests/test_blocks_gpu.py) for arithmetic; for the router's decisions a margin
computed per case and branch from the reference alone (8 x the fp32 restatement's logit error, moe_block_ref.routing_margin) --
outside it every ordered decision must equal the fp64 one, and at most 0.5 % of a case's tokens may lie inside it.  Nothing the
kernels compute enters a bound.  Cases run smallest first."""
import ctypes as C
import os
import sys

import pytest
import torch

from conftest import ROOT, pkg, rel_inf

sys.path.insert(0, os.path.join(ROOT, "tests"))
import moe_block_ref as MB  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = {3: 1e-3, 1: 3e-2, 2: 6e-3, 4: 1e-3}
SEED = 3
NUM_FRAMES = 8200
LEFT_OUT_CAP = 0.005
# (D, H, F, E): router kernel / expert path, see the table in DESIGN.md
SHAPES = [(64, 4, 128, 4), (128, 4, 256, 5), (256, 4, 512, 2), (320, 5, 256, 6), (192, 3, 320, 3), (768, 6, 1024, 11),
          (512, 4, 1024, 8), (512, 4, 320, 7), (1024, 4, 2048, 16), (1024, 4, 2048, 9)]
ROW_KERNEL, GATE16_RT, GATE16_CONST = (320, 5, 256, 6), (128, 4, 256, 5), (512, 4, 1024, 8)
KNOB_CONST_E, KNOB_RUNTIME_E, KNOB_MLP_LDS = 26, 27, 34
_MODS = {}


class Block:
    """One width's module on the GPU, its sub-state in fp64 on the GPU (reference) and the router's part of it on the CPU."""

    def __init__(self, D, H, Fd, E):
        T = pkg("transformer")
        self.D, self.H, self.F, self.E = D, H, Fd, E
        m = T.MotionTransformer(8, num_frames=NUM_FRAMES, latent_dim=D, ff_size=Fd, num_layers=1, num_heads=H,
                                text_latent_dim=64, moe_num_experts=E, precision=3)
        sd = MB.block_state(D, H, Fd, E, SEED, num_frames=NUM_FRAMES)
        res = m.load_state_dict(sd, strict=False)
        assert not res.unexpected_keys
        self.m = m.cuda().eval()
        self.sd64 = MB.cast_state(sd, torch.float64, "cuda")
        self.r32 = {k: v for k, v in sd.items() if ".experts." not in k}
        self.r64 = MB.cast_state(self.r32, torch.float64)
        self.gates0 = {k: v.clone() for k, v in sd.items() if ".moe.gate." in k}

    def load_gates(self, edit=None):
        """Replace the gate matrices and biases by edit(pristine copies) in the module (repacked on next use) and in the reference's
        state; None restores the seeded ones."""
        g = {k: v.clone() for k, v in self.gates0.items()}
        if edit is not None:
            edit(g)
        self.m.load_state_dict(g, strict=False)
        self.r32.update(g)
        self.r64.update(MB.cast_state(g, torch.float64))
        self.sd64.update(MB.cast_state(g, torch.float64, "cuda"))

    def counters(self):
        b = self.m.moe_buffers()
        return (torch.stack([b[f"{MB.PRE}.branches.{br}.moe.expert_usage"] for br in range(2)]).cpu().double(),
                torch.stack([b[f"{MB.PRE}.branches.{br}.moe.expert_importance"] for br in range(2)]).cpu().double())

    def reference(self, h, sc, forced=None):
        with torch.no_grad():
            out, info = MB.moe_block(h.double().cuda(), sc.double().cuda(), self.sd64, self.E, forced)
        return out.cpu(), info

    def run(self, prec, h, sc, length, forced=None, knob=0, dump=False, status=False, pack_prec=None, workspace=False):
        """One launch chain of the block.  Returns out (CPU) [, dumped decisions (2, M, 2)] [, the workspace tensor (GPU) as the block
        left it: workspace=True]; status=True: (status, out) unchecked."""
        L = pkg("_lib")
        lib = L.lib()
        self.m.precision = pack_prec or prec
        pm = self.m.pack()
        B, S, D = h.shape
        M = B * S
        ws = self.m._workspace(B, S, 1)
        sc4 = torch.zeros((4, B, 2 * D))
        sc4[3] = sc
        hd, scd, ld = h.cuda().contiguous(), sc4.cuda(), length.to(torch.int32).cuda()
        out = torch.full_like(hd, 777.0)
        fr = forced.to(torch.int32).cuda().contiguous() if forced is not None else None
        buf = torch.full((4 * M,), -1, dtype=torch.int32, device="cuda") if dump else None
        assert lib.mdm_set_gemm_variant(C.c_int32(knob)) == 0
        if dump:
            lib.mdm_route_dump(C.c_void_p(buf.data_ptr()), C.c_int64(buf.numel()))
        try:
            st = lib.mdm_block_forward(C.byref(pm.model), C.c_int32(0), C.c_int32(L.BLOCK_MOE), None, C.c_void_p(hd.data_ptr()),
                                       C.c_void_p(scd.data_ptr()), C.c_void_p(ld.data_ptr()), C.c_int32(B), C.c_int32(S),
                                       C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), C.c_int64(ws.numel()),
                                       C.c_void_p(L.ptr(fr)), C.c_int32(prec), C.c_void_p(L.stream_ptr()))
            torch.cuda.synchronize()
        finally:
            lib.mdm_route_dump(C.c_void_p(0), C.c_int64(0))
            lib.mdm_set_gemm_variant(C.c_int32(0))
        if status:
            return st, out.cpu()
        L.check(st, "mdm_block_forward(MDM_BLOCK_MOE)")
        res = (out.cpu(),) + ((buf.reshape(2, M, 2).cpu().long(),) if dump else ()) + ((ws,) if workspace else ())
        return res if len(res) > 1 else res[0]


def block(shape):
    if shape not in _MODS:
        _MODS[shape] = Block(*shape)
    return _MODS[shape]


def accepted(shape, prec):
    """csrc/model.hip set_precision, as include/mdm_hip.h documents it: the 16-bit and mixed modes need D and F in multiples of the
    64-wide k-tile (precision 1 falls back to fp32 rows instead of refusing), the fp8 mode multiples of 128."""
    D, _, Fd, _ = shape
    if prec in (2, 4):
        return D % 64 == 0 and Fd % 64 == 0
    if prec == 5:
        return D % 128 == 0 and Fd % 128 == 0
    return True


def tag(shape, prec, B, S, knob=0):
    return f"D={shape[0]} H={shape[1]} F={shape[2]} E={shape[3]} precision {prec} knob {knob} tokens {B * S}"


# ---------------------------------------------------------------------------------------------------------------------
# the two checks every case below is made of
# ---------------------------------------------------------------------------------------------------------------------
def forced_case(shape, prec, B, S, forced=None, knob=0, what="reference routing"):
    """Arithmetic: the block with given decisions (None: the fp64 reference's own) against the reference with the same ones."""
    bk = block(shape)
    h, sc, length = MB.block_inputs(B, S, shape[0], SEED)
    if forced is None:
        _, info = bk.reference(h, sc)
        forced = torch.stack([info[br]["idx"].cpu() for br in range(2)])
    ref, _ = bk.reference(h, sc, forced)
    out = bk.run(prec, h, sc, length, forced, knob)
    err = rel_inf(out, ref)
    print(f"{tag(shape, prec, B, S, knob)} [{what}]: rel err {err:.2e}")
    assert torch.isfinite(out).all()
    assert err < TOL[prec], (shape, prec, what, err)
    return out


def free_case(shape, prec, B, S, knob=0, calls=1):
    """Free routing: ordered decisions against fp64 outside the derived margin, counters against the dumped decisions and the
    fp64 probabilities, the output against fp64 on every token outside the margin.  calls = 2: the counters accumulate."""
    bk = block(shape)
    D, _, _, E = shape
    M = B * S
    h, sc, length = MB.block_inputs(B, S, D, SEED)
    ref, info = bk.reference(h, sc)
    bk.m.reset_all_moe_counters()
    u0, i0 = bk.counters()
    for _ in range(calls):
        out, idx = bk.run(prec, h, sc, length, None, knob, dump=True)
    u1, i1 = bk.counters()
    assert int(idx.min()) >= 0 and int(idx.max()) < E
    near_any = torch.zeros(M, dtype=torch.bool)
    line = []
    for br in range(2):
        margin, l64 = MB.routing_margin(h, bk.r32, bk.r64, br)
        near = MB.top3_gap(l64) < margin
        want = info[br]["idx"].cpu()
        wrong = (idx[br] != want).any(-1)
        near_any |= near
        line.append(f"branch {br}: margin {margin:.2e}, left out {int(near.sum())}/{M} ({100.0 * int(near.sum()) / M:.3f} %), "
                    f"differing inside it {int((wrong & near).sum())}")
        assert int(near.sum()) <= LEFT_OUT_CAP * M, (shape, prec, br, "reference cap: choose another seed", int(near.sum()))
        bad = (wrong & ~near).nonzero().flatten()
        assert bad.numel() == 0, (shape, prec, knob, br, bad[:8].tolist(), idx[br][bad[:8]].tolist(), want[bad[:8]].tolist())
        # counters: usage = top-1 histogram of the dumped decisions (exact), importance = fp64 probabilities at those decisions
        hist = torch.bincount(idx[br][:, 0], minlength=E).double()
        assert torch.equal(u1[br] - u0[br], calls * hist) and float(hist.sum()) == M, (shape, prec, br, (u1[br] - u0[br]).tolist())
        p64 = torch.softmax(info[br]["logits"], dim=1).cpu()
        imp = torch.zeros(E, dtype=torch.float64).index_add_(0, idx[br].flatten(), p64.gather(1, idx[br]).flatten())
        e_imp = float((i1[br] - i0[br] - calls * imp).abs().max() / (calls * imp.max()))
        line.append(f"importance rel err {e_imp:.1e}")
        assert e_imp < 1e-5, (shape, prec, br, e_imp)
    ok = ~near_any
    err = float((out.reshape(M, D)[ok].double() - ref.reshape(M, D)[ok]).abs().max() / ref.abs().max()) if bool(ok.any()) else 0.0
    print(f"{tag(shape, prec, B, S, knob)} [free routing]: rel err {err:.2e}; " + "; ".join(line))
    assert torch.isfinite(out).all()
    if prec in TOL:  # the fp8 mode's arithmetic is gated stage by stage in tests/test_fp8_block_gpu.py
        assert err < TOL[prec], (shape, prec, err)
    return out, idx


# ---------------------------------------------------------------------------------------------------------------------
# a refused precision writes nothing
# ---------------------------------------------------------------------------------------------------------------------
def test_refused_precision_returns_unsupported_and_writes_nothing():
    """The fp8 mode needs D and F in multiples of 128: at (64, 4, 128, 4) the block returns MDM_ERR_UNSUPPORTED before any launch."""
    shape = SHAPES[0]
    assert not accepted(shape, 5)
    h, sc, length = MB.block_inputs(2, 37, shape[0], SEED)
    bk = block(shape)
    st, out = bk.run(5, h, sc, length, status=True, pack_prec=3)  # (refused before any weight is read)
    assert st == 3 and bool((out == 777.0).all())
    with pytest.raises(pkg("_lib").MdmError):
        bk.run(5, h, sc, length, pack_prec=3)


# ---------------------------------------------------------------------------------------------------------------------
# 2. shape matrix, routing forced to the reference's
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S", [(2, 37), (4, 601)])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_shape_matrix_matches_fp64_with_reference_routing(shape, B, S):
    bk = block(shape)
    for prec in (3, 4, 1, 2):
        bk.m.precision = prec
        assert bk.m.workspace_bytes(B, S, 1) > 0  # pack() and workspace_bytes() take every admitted width
        if not accepted(shape, prec):
            h, sc, length = MB.block_inputs(B, S, shape[0], SEED)
            st, out = bk.run(prec, h, sc, length, status=True)
            assert st == 3 and bool((out == 777.0).all()), (shape, prec, st)
            continue
        forced_case(shape, prec, B, S)
        if shape == GATE16_CONST and prec in (1, 2, 4):
            forced_case(shape, prec, B, S, knob=KNOB_MLP_LDS)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the router's own decisions
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_router_decisions_equal_fp64_outside_the_margin(shape):
    """One precision per format of the hn rows the router writes (3: fp32 or pre-split rows, 1: bf16, 2: fp16, 5: e4m3 where the
    mode exists and the constant-E router does), both the constant-E and the run-time-E kernel where the former exists."""
    B, S = 8, 512
    const_e = shape[0] in (512, 1024) and shape[3] in (8, 16)
    for prec in (3, 1, 2) + ((5,) if const_e else ()):
        for knob in ((KNOB_CONST_E, KNOB_RUNTIME_E) if const_e else (0,)):
            free_case(shape, prec, B, S, knob)


# ---------------------------------------------------------------------------------------------------------------------
# 4. ties
# ---------------------------------------------------------------------------------------------------------------------
def _tie(groups):
    def edit(sd):
        for br in range(2):
            w, b = sd[f"{MB.PRE}.branches.{br}.moe.gate.weight"], sd[f"{MB.PRE}.branches.{br}.moe.gate.bias"]
            for g in groups:
                for e in g[1:]:
                    w[e], b[e] = w[g[0]].clone(), b[g[0]].clone()
            assert all(torch.equal(w[e], w[g[0]]) and torch.equal(b[e], b[g[0]]) for g in groups for e in g)
    return edit


@pytest.mark.parametrize("shape", [GATE16_RT, ROW_KERNEL, GATE16_CONST], ids=lambda s: "x".join(map(str, s)))
def test_tied_experts_are_named_lowest_index_first(shape):
    """Bit-identical gate rows and biases give bit-equal logits in every router kernel.  Wherever a tied group reaches the top 2,
    the decision names its lowest indices in ascending order: a tied first place is (g0, g1); a tied second place is g0.  Pairs at
    (0, 1), in the middle and at (E - 2, E - 1), and a triple; the row kernel, the LDS-staged router with run-time E, and with
    constant E (knob 26) next to its run-time twin (knob 27) at D = 512, E = 8."""
    D, _, _, E = shape
    B, S = 3, 171
    h, sc, length = MB.block_inputs(B, S, D, SEED)
    mid = E // 2 - 1
    bk = block(shape)
    try:
        _tied_groups(bk, shape, h, sc, length, B, S, mid)
    finally:
        bk.load_gates(None)


def _tied_groups(bk, shape, h, sc, length, B, S, mid):
    E = shape[3]
    for groups in ([(0, 1)], [(mid, mid + 1)], [(E - 2, E - 1)], [(0, 1, 2)], [(E - 3, E - 2, E - 1)]):
        bk.load_gates(_tie(groups))
        for prec in (3, 2):
            for knob in ((KNOB_CONST_E, KNOB_RUNTIME_E) if shape == GATE16_CONST else (0,)):
                _, idx = bk.run(prec, h, sc, length, None, knob, dump=True)
                g = torch.tensor(groups[0])
                first_in, second_in = torch.isin(idx[..., 0], g), torch.isin(idx[..., 1], g)
                top = first_in
                assert bool((idx[top] == g[:2]).all()), (shape, groups, prec, knob, idx[top][(idx[top] != g[:2]).any(-1)][:4].tolist())
                snd = second_in & ~first_in
                assert bool((idx[snd][:, 1] == g[0]).all()), (shape, groups, prec, knob)
                print(f"{tag(shape, prec, B, S, knob)} tie {groups}: tied first place {int(top.sum())}, tied second place {int(snd.sum())} of {2 * B * S}")
                assert int(top.sum()) > 0 and int(snd.sum()) > 0, "the case must contain both kinds of tie"
                assert bool((idx[..., 0] != idx[..., 1]).all())


@pytest.mark.parametrize("shape", [GATE16_RT, ROW_KERNEL, GATE16_CONST], ids=lambda s: "x".join(map(str, s)))
def test_zero_gates_route_every_token_to_experts_0_and_1(shape):
    """The state of a fresh model (reset_parameters zeroes the gates): every logit is 0, every probability fp32 1 / E, every decision
    (0, 1); seen through the dump, the counters and the output against the reference."""
    D, _, _, E = shape

    def edit(sd):
        for br in range(2):
            sd[f"{MB.PRE}.branches.{br}.moe.gate.weight"].zero_()
            sd[f"{MB.PRE}.branches.{br}.moe.gate.bias"].zero_()

    bk = block(shape)
    bk.load_gates(edit)
    try:
        _zero_gates(bk, shape)
    finally:
        bk.load_gates(None)


def _zero_gates(bk, shape):
    D, _, _, E = shape
    B, S = 3, 171
    M = B * S
    h, sc, length = MB.block_inputs(B, S, D, SEED)
    ref, info = bk.reference(h, sc)
    assert all(bool((info[br]["idx"].cpu() == torch.tensor([0, 1])).all()) for br in range(2))
    for prec in (3, 4, 1, 2):
        bk.m.reset_all_moe_counters()
        out, idx = bk.run(prec, h, sc, length, dump=True)
        assert bool((idx == torch.tensor([0, 1])).all())
        usage, imp = bk.counters()
        want_u = torch.zeros(2, E, dtype=torch.float64)
        want_u[:, 0] = M
        want_i = torch.zeros(2, E, dtype=torch.float64)
        want_i[:, :2] = M * float(torch.tensor(1.0) / torch.tensor(float(E)))
        assert torch.equal(usage, want_u)
        assert float((imp - want_i).abs().max()) <= 1e-5 * float(want_i.max()), imp.tolist()
        err = rel_inf(out, ref)
        print(f"{tag(shape, prec, B, S)} [zero gates]: rel err {err:.2e}")
        assert err < TOL[prec]


# ---------------------------------------------------------------------------------------------------------------------
# 5. skew
# ---------------------------------------------------------------------------------------------------------------------
EDGES = [31, 32, 33, 63, 64, 65, 111, 112, 113, 127, 128, 129]  # csrc/mlp_stream.hip row tiles 32 / 64 / 112, tile GEMMs 128


def _grouped(M, E, sizes_by_branch):
    """Tokens in groups: group j goes to experts (2j, 2j + 1), sizes[j] tokens each, the rest to the group after the last sized
    one; spread over the token order by a fixed permutation.  Slab sizes of experts 2j and 2j + 1 are exactly sizes[j]."""
    f = torch.empty((2, M, 2), dtype=torch.int64)
    for br, sizes in enumerate(sizes_by_branch):
        assert len(sizes) < E // 2 and sum(sizes) < M
        g = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
        g = torch.cat([g, torch.full((M - g.numel(),), len(sizes))])
        g = g[torch.randperm(M, generator=torch.Generator().manual_seed(br))]
        f[br, :, 0], f[br, :, 1] = 2 * g, 2 * g + 1
        counts = torch.bincount(f[br].flatten(), minlength=E)
        assert counts[:2 * len(sizes)].tolist() == [s for s in sizes for _ in range(2)]
    return f


def skews(M, E):
    t = torch.arange(M)
    G = E // 2
    one = torch.tensor([0, 1]).expand(2, M, 2).clone()
    yield "all tokens to (0, 1)", one
    yield "all tokens to (E-1, E-2)", torch.tensor([E - 1, E - 2]).expand(2, M, 2).clone()
    alone = one.clone()
    alone[:, M - 1] = torch.tensor([2, 3])
    yield "all but the last token to (0, 1)", alone
    per = G - 1
    chunks = [EDGES[i:i + per] for i in range(0, len(EDGES), per)]
    if len(chunks) % 2:
        chunks.append(chunks[0])
    for i in range(0, len(chunks), 2):
        yield f"slab sizes {chunks[i]} | {chunks[i + 1]}", _grouped(M, E, [chunks[i], chunks[i + 1]])
    alt = torch.stack([2 * (t % G), 2 * ((t + 1) % G)], 1)
    yield "odd experts empty", torch.stack([alt, alt.flip(1)])
    twice = torch.stack([t % E, t % E], 1)
    yield "both choices the same expert", torch.stack([twice, (twice + 1) % E])


SKEW_RUNS = [(GATE16_CONST, 1, 0), (GATE16_CONST, 2, 0), (GATE16_CONST, 2, KNOB_MLP_LDS), (GATE16_CONST, 3, 0), (GATE16_CONST, 4, 0),
             (ROW_KERNEL, 2, 0), (ROW_KERNEL, 3, 0), ((1024, 4, 2048, 16), 2, 0)]


@pytest.mark.parametrize("shape,prec,knob", SKEW_RUNS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_skewed_routing_matches_fp64(shape, prec, knob):
    """Routing built by hand: one huge slab and 2E - 2 empty ones, a token alone in its experts, slab sizes at, one under and one
    over the expert kernels' row tiles, alternating empty experts, a token sent twice to one expert (the reference sums both
    probabilities on that expert's output; the kernel's two slab rows must add up to the same)."""
    B, S = 4, 250
    for what, forced in skews(B * S, shape[3]):
        forced_case(shape, prec, B, S, forced, knob, what)


@pytest.mark.parametrize("shape,prec", [(GATE16_CONST, 2), (GATE16_CONST, 3), (ROW_KERNEL, 2), (GATE16_RT, 3)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_out_of_range_forced_indices_are_clamped_at_the_c_abi(shape, prec):
    """The Python wrapper refuses forced indices outside [0, E); the kernels clamp them: bit-identical to the clamped run."""
    D, _, _, E = shape
    B, S = 2, 37
    bk = block(shape)
    h, sc, length = MB.block_inputs(B, S, D, SEED)
    t = torch.arange(B * S)
    forced = torch.stack([torch.stack([t % E, (t + 1) % E], 1), torch.stack([(t + 2) % E, t % E], 1)])
    wild = forced.clone()
    wild[0, ::3, 0], wild[1, 1::4, 1], wild[0, 5, 1] = wild[0, ::3, 0] - 2 * E, wild[1, 1::4, 1] + 3 * E, 2 ** 31 - 1
    clamped = wild.clamp(0, E - 1)
    assert not torch.equal(clamped, forced)
    a, ia = bk.run(prec, h, sc, length, wild, dump=True)
    b, ib = bk.run(prec, h, sc, length, clamped, dump=True)
    assert torch.isfinite(a).all() and torch.equal(a, b) and torch.equal(ia, ib) and torch.equal(ib, clamped)
    ref, _ = bk.reference(h, sc, clamped)
    assert rel_inf(a, ref) < TOL[prec]


# ---------------------------------------------------------------------------------------------------------------------
# 6. counters
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [2, 3])
@pytest.mark.parametrize("shape", [GATE16_RT, ROW_KERNEL, GATE16_CONST], ids=lambda s: "x".join(map(str, s)))
def test_counters_accumulate_over_two_calls(shape, prec):
    """free_case checks one call's increments in every free-routing case of this module; here a second call must add the same
    again, for the three router kernels, in a 16-bit and an fp32-grade mode, below and across the router's grid-stride loop."""
    free_case(shape, prec, 3, 171, calls=2)
    free_case(shape, prec, 1, 8193 if shape != ROW_KERNEL else 2049, calls=2)


# ---------------------------------------------------------------------------------------------------------------------
# 8. row independence
# ---------------------------------------------------------------------------------------------------------------------
PATHS = [("FUSED streamed", GATE16_CONST, 2, 0), ("FUSED LDS-staged", GATE16_CONST, 2, KNOB_MLP_LDS), ("FUSED streamed, mixed", GATE16_CONST, 4, 0),
         ("GROUPED 16-bit", (512, 4, 320, 7), 2, 0), ("GROUPED 16-bit, bf16", GATE16_RT, 1, 0),
         ("GROUPED fp32-grade, pre-split rows + pair stream", GATE16_CONST, 3, 0), ("GROUPED fp32-grade, pre-split rows", (256, 4, 512, 2), 3, 0),
         ("GROUPED fp32-grade, fp32 rows", ROW_KERNEL, 3, 0)]


@pytest.mark.parametrize("name,shape,prec,knob", PATHS, ids=[p[0].replace(" ", "_") for p in PATHS])
def test_rows_are_independent_of_their_order_and_of_the_run(name, shape, prec, knob):
    """Two runs of one input are bit-identical (slab order comes from atomics and must not show), and permuting the frames inside
    each sample permutes the output rows bit for bit: slab sizes and the kernel choice are unchanged, so a tile that leaks across
    rows at a ragged slab edge shows."""
    B, S = 3, 211
    D = shape[0]
    bk = block(shape)
    h, sc, _ = MB.block_inputs(B, S, D, SEED)
    length = torch.full((B,), S)
    out, idx = bk.run(prec, h, sc, length, None, knob, dump=True)
    again, idx2 = bk.run(prec, h, sc, length, None, knob, dump=True)
    assert torch.isfinite(out).all() and torch.equal(idx, idx2)
    assert torch.equal(out, again), (name, float((out - again).abs().max()))
    perms = torch.stack([torch.randperm(S, generator=torch.Generator().manual_seed(b)) for b in range(B)])
    hp = torch.stack([h[b, perms[b]] for b in range(B)])
    outp, idxp = bk.run(prec, hp, sc, length, None, knob, dump=True)
    want = torch.stack([out[b, perms[b]] for b in range(B)])
    flat = (perms + S * torch.arange(B)[:, None]).flatten()
    assert torch.equal(idxp, idx[:, flat])
    assert torch.equal(outp, want), (name, float((outp - want).abs().max()))
    print(f"{name}: {tag(shape, prec, B, S, knob)}: bit-identical across runs and under a frame permutation")


# ---------------------------------------------------------------------------------------------------------------------
# 7. token-count boundaries (last: the largest cases of the module)
# ---------------------------------------------------------------------------------------------------------------------
def _bs(M):
    for B in (1, 2, 3, 5, 7, 9, 11, 13):
        if M % B == 0 and M // B <= NUM_FRAMES:
            return B, M // B
    raise AssertionError(M)


@pytest.mark.parametrize("M", [1, 15, 16, 17, 8191, 8192, 8193, 20001, 65547])
@pytest.mark.parametrize("shape", [GATE16_RT, GATE16_CONST], ids=lambda s: "x".join(map(str, s)))
def test_token_count_boundaries_of_the_lds_staged_router(shape, M):
    """1 .. 17: the 16-token workgroup iteration; 8191 .. 20001: the router's grid-stride loop (512 workgroups x 16 tokens) with its
    row prefetch and per-block partial counters over several iterations; 65547: moe_assign_kernel's loop (1024 x 256 entries)."""
    B, S = _bs(M)
    for prec in (2, 3):
        free_case(shape, prec, B, S)


@pytest.mark.parametrize("M", [2047, 2048, 2049, 9002])
def test_token_count_boundaries_of_the_row_router(M):
    """512 workgroups x 4 rows."""
    B, S = _bs(M)
    for prec in (2, 3):
        free_case(ROW_KERNEL, prec, B, S)

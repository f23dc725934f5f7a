"""GPU: the MoE router folded into the cross-attention stylization launch (RoutePath::FOLDED: gate in that launch's epilogue, slab
offsets inside the assign launch) against the three-launch router (knob 171, MDM_VAR_ROUTE_LAUNCH, which is the code before the
fold).  Everything the router leaves -- top_idx, top_val, the hn rows, goff -- and the denoiser output must be bit-identical; the
order inside an expert's slab is unspecified in both, so perm / pos4 / rowscale are checked as a consistent assignment, not
against each other.

Models are synthetic one-layer MotionTransformers (one decoder layer per time scale), run through the whole mdm_denoiser_forward
with mdm_route_dump set; the full-scale layer's routing is then read out of the workspace (mdm_route_workspace).  The coarse
layer's workspace state is overwritten by the full-scale layer, so it is read after a one-layer call (MDM_BLOCK_LAYER) at the
coarse row counts.

Importance sums: both paths against the float64 sum of top_val per (branch, expert) with the bound n * 2^-24 * sum, n = the number
of addends: the worst case of ANY fp32 summation order of n non-negative terms, so it holds for the per-workgroup grouping of
either path (16-row groups of the gate launch, 32-row tiles of the stylization launch)."""
import ctypes as C

import pytest
import torch

from conftest import pkg

pytestmark = pytest.mark.gpu
KNOB_LAUNCH = 171
FEATS, NTEXT, DT = 8, 6, 64
_MODELS = {}


def model(D, E):
    if (D, E) not in _MODELS:
        T_, synth = pkg("transformer"), pkg("synth")
        H, Fd = 4, 2 * D
        m = T_.MotionTransformer(FEATS, num_frames=64, latent_dim=D, ff_size=Fd, num_layers=1, num_heads=H, text_latent_dim=DT,
                                 moe_num_experts=E, precision=1)
        sd = synth.synth_state_dict(m._layout, 5)
        m.load_state_dict(sd, strict=True)
        m.set_ephemerals(synth.synth_ephemerals(D, DT, 1, 7)), m.set_projections(synth.synth_projections(D // H, 1, 7))
        gates = {k: v.clone() for k, v in sd.items() if ".moe.gate." in k}
        _MODELS[(D, E)] = (m.cuda().eval(), gates)
    return _MODELS[(D, E)]


def inputs(B, T):
    x, t, length, xf_proj, xf_out = pkg("synth").synth_inputs(B, T, FEATS, NTEXT, DT, 11, min_len=4)
    return x.cuda(), t.cuda(), length.cuda(), xf_proj.cuda(), xf_out.cuda()


def counters(m, scale):
    """(usage, importance) float64 (2, E) of the one decoder layer at `scale` ('low' / 'high')."""
    b = m.moe_buffers()
    pick = lambda leaf: torch.stack([next(v for k, v in b.items() if f"decoder_blocks_{scale}.0." in k and f"branches.{br}." in k and k.endswith(leaf))
                                     for br in range(2)]).cpu().double()
    return pick("expert_usage"), pick("expert_importance")


def read_route(m, ws, B, T, N, M, h16):
    """The router's buffers as the last MoE block (M rows) left them in workspace ws carved for (B, T, N)."""
    L = pkg("_lib")
    off = (C.c_int64 * 8)()
    L.check(L.lib().mdm_route_workspace(C.byref(m.pack().model), C.c_int32(B), C.c_int32(T), C.c_int32(N), off))
    D, E = m.latent_dim, m.moe_num_experts
    torch.cuda.synchronize()

    def view(i, n, dt):
        nbytes = n * torch.empty((), dtype=dt).element_size()
        return ws[off[i]:off[i] + nbytes].clone().view(dt).cpu()
    r = dict(hn=view(0, 2 * M * D, torch.int16 if h16 else torch.int32).reshape(2, M, D), top_idx=view(1, 4 * M, torch.int32).reshape(2, M, 2).long(),
             top_val=view(2, 4 * M, torch.float32).reshape(2, M, 2), perm=view(3, 4 * M, torch.int32).long(),
             rowscale=view(4, 4 * M, torch.float32), pos4=view(5, 4 * M, torch.int32).reshape(M, 4).long(),
             goff=view(6, 2 * E + 1, torch.int32).long(), cursor=view(7, 2 * E, torch.int32).long())
    return r


def forward(m, prec, inp, knob, forced=None, calls=1):
    """Whole denoiser forwards under `knob`: output, dumped decisions [layer] -> (2, M_layer, 2), the full-scale layer's routing."""
    L = pkg("_lib")
    x, t, length, xf_proj, xf_out = inp
    B, T, _ = x.shape
    m.precision = prec
    dump = torch.full((2, 4 * B * T), -1, dtype=torch.int32, device="cuda")
    assert L.lib().mdm_set_gemm_variant(C.c_int32(knob)) == 0
    L.lib().mdm_route_dump(C.c_void_p(dump.data_ptr()), C.c_int64(dump.numel()))
    try:
        for _ in range(calls):
            out = m(x, t, length, xf_proj=xf_proj, xf_out=xf_out, forced_routing=forced)
        torch.cuda.synchronize()
    finally:
        L.lib().mdm_route_dump(C.c_void_p(0), C.c_int64(0))
        L.lib().mdm_set_gemm_variant(C.c_int32(0))
    idx = [dump[li, :4 * Ml].reshape(2, Ml, 2).cpu().long() for li, Ml in ((0, B * T // 2), (1, B * T))]
    route = read_route(m, m._workspace(B, T, NTEXT), B, T, NTEXT, B * T, prec in (1, 2))
    return out.cpu(), idx, route


def layer(m, prec, B, S, knob):
    """One decoder layer (the coarse one, layer 0) alone at B x S rows: output and its routing."""
    L, synth = pkg("_lib"), pkg("synth")
    D = m.latent_dim
    m.precision = prec
    pm = m.pack()
    h = (synth.uniform_pm1((B, S, D), "fold.h", S) * 1.5).cuda()
    sc = (synth.uniform_pm1((4, B, 2 * D), "fold.sc", S) * 0.5).cuda()
    xf = (synth.uniform_pm1((B, NTEXT, DT), "fold.xf", S) * 1.7).cuda()
    ln = torch.full((B,), S, dtype=torch.int32, device="cuda")
    tcache = m.prepare_text(xf)
    ws = m._workspace(B, S, NTEXT)
    out = torch.empty_like(h)
    assert L.lib().mdm_set_gemm_variant(C.c_int32(knob)) == 0
    try:
        L.check(L.lib().mdm_block_forward(C.byref(pm.model), C.c_int32(0), C.c_int32(L.BLOCK_LAYER), C.byref(tcache["tc"]),
                                          C.c_void_p(h.data_ptr()), C.c_void_p(sc.data_ptr()), C.c_void_p(ln.data_ptr()), C.c_int32(B),
                                          C.c_int32(S), C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), C.c_int64(ws.numel()),
                                          None, C.c_int32(prec), C.c_void_p(L.stream_ptr())))
        torch.cuda.synchronize()
    finally:
        L.lib().mdm_set_gemm_variant(C.c_int32(0))
    return out.cpu(), read_route(m, ws, B, S, NTEXT, B * S, prec in (1, 2))


def check_assignment(r, M, E, what):
    """goff / perm / pos4 / rowscale / cursor form one consistent slab assignment of the decisions in top_idx."""
    idx, goff, perm, pos4 = r["top_idx"], r["goff"], r["perm"], r["pos4"]
    assert int(idx.min()) >= 0 and int(idx.max()) < E, what
    group = (idx + E * torch.arange(2)[:, None, None]).reshape(-1)  # entry (br, tok, k) -> slab
    counts = torch.bincount(group, minlength=2 * E)
    assert int(goff[0]) == 0 and int(goff[2 * E]) == 4 * M, (what, goff.tolist())
    assert torch.equal(goff[1:] - goff[:-1], counts), (what, goff.tolist(), counts.tolist())
    assert torch.equal(r["cursor"], counts), (what, "cursors were zero before the first reservation", r["cursor"].tolist())
    row_of = (torch.arange(2)[:, None] * M + torch.arange(M)[None, :])[:, :, None].expand(2, M, 2)  # entry -> hn row
    pos = pos4.reshape(M, 2, 2).permute(1, 0, 2)  # (br, tok, k)
    assert torch.equal(perm[pos], row_of), (what, "perm[pos4[tok, j]] maps back to (branch, tok)")
    assert torch.equal(pos.reshape(-1).sort().values, torch.arange(4 * M)), (what, "pos4 is a permutation of the slab rows")
    assert torch.equal(r["rowscale"][pos].view(torch.int32), r["top_val"].view(torch.int32)), what
    for g in range(2 * E):
        have = perm[goff[g]:goff[g + 1]].sort().values
        want = row_of.reshape(-1)[group == g].sort().values
        assert torch.equal(have, want), (what, g)
    return counts


def check_importance(m, scale, r, E, calls, what):
    usage, imp = counters(m, scale)
    for br in range(2):
        first = torch.bincount(r["top_idx"][br][:, 0], minlength=E).double()
        assert torch.equal(usage[br], calls * first), (what, br, usage[br].tolist())
        s64 = torch.zeros(E, dtype=torch.float64).index_add_(0, r["top_idx"][br].reshape(-1), r["top_val"][br].reshape(-1).double())
        n = torch.bincount(r["top_idx"][br].reshape(-1), minlength=E).double()
        bound = (calls * n) * 2.0 ** -24 * (calls * s64)
        err = (imp[br] - calls * s64).abs()
        print(f"{what} branch {br}: importance err / bound max {float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= bound).all()), (what, br, err.tolist(), bound.tolist())


def same_route(a, b, what):
    for k in ("top_idx", "goff"):
        assert torch.equal(a[k], b[k]), (what, k)
    assert torch.equal(a["top_val"].view(torch.int32), b["top_val"].view(torch.int32)), (what, "top_val")
    assert torch.equal(a["hn"], b["hn"]), (what, "hn rows")


def fold_vs_launch(D, E, prec, B, T, forced=None, expect_empty=False):
    """The denoiser forward and the coarse layer alone, default path against knob 171; returns the full-scale slab sizes."""
    m, _ = model(D, E)
    inp = inputs(B, T)
    res = {}
    for knob in (0, KNOB_LAUNCH):
        m.reset_all_moe_counters()
        out, idx, r = forward(m, prec, inp, knob, forced)
        what = f"D={D} E={E} precision {prec} B={B} T={T} knob {knob}"
        assert torch.isfinite(out).all(), what
        counts = check_assignment(r, B * T, E, what)
        assert torch.equal(idx[1], r["top_idx"]), (what, "the dump is the full-scale layer's top_idx")
        check_importance(m, "high", r, E, 1, what)
        res[knob] = (out, idx, r, counts)
    (out_f, idx_f, r_f, counts), (out_l, idx_l, r_l, _) = res[0], res[KNOB_LAUNCH]
    what = f"D={D} E={E} precision {prec} B={B} T={T}"
    assert all(torch.equal(a, b) for a, b in zip(idx_f, idx_l)), (what, "routing of both layers")
    same_route(r_f, r_l, what)
    assert torch.equal(out_f, out_l), (what, float((out_f - out_l).abs().max()))
    if forced is not None:
        for li, Ml in ((0, B * T // 2), (1, B * T)):
            assert torch.equal(idx_f[li], forced[li, :4 * Ml].reshape(2, Ml, 2).long()), (what, li)
    if expect_empty:
        assert int((counts == 0).sum()) > 0, (what, counts.tolist())
    if forced is None:  # the coarse layer's workspace state: one layer alone at the coarse row count
        lay = {}
        for knob in (0, KNOB_LAUNCH):
            m.reset_all_moe_counters()
            o, r = layer(m, prec, B, T // 2, knob)
            check_assignment(r, B * T // 2, E, f"{what} coarse layer knob {knob}")
            check_importance(m, "low", r, E, 1, f"{what} coarse layer knob {knob}")
            lay[knob] = (o, r)
        same_route(lay[0][1], lay[KNOB_LAUNCH][1], what + " coarse layer")
        assert torch.equal(lay[0][0], lay[KNOB_LAUNCH][0]), what + " coarse layer"
    return counts


@pytest.mark.parametrize("prec", [1, 2])
@pytest.mark.parametrize("E", [8, 16])
@pytest.mark.parametrize("B,T", [(3, 40), (2, 16)])
def test_folded_route_is_bit_identical_on_partial_tiles(B, T, E, prec):
    """B = 3, T = 40: 60 coarse rows and 120 full-scale ones, last 32-row tiles of 28 and 24 rows.  B = 2, T = 16: 16 coarse rows,
    one partial tile (and one whole tile at the full scale).  The 16-lane groups past the end of the last tile are active."""
    fold_vs_launch(512, E, prec, B, T)


def _skew(m, gates, E):
    g = {k: v.clone() for k, v in gates.items()}
    for k in g:
        if k.endswith("gate.bias"):
            br1 = ".branches.1." in k
            g[k][5 if not br1 else E - 2] += 30.0  # every token's first choice
            g[k][0 if not br1 else 3] -= 30.0      # never chosen: an empty slab
            g[k][1 if not br1 else 4] -= 30.0
    m.load_state_dict(g, strict=False)


@pytest.mark.parametrize("prec", [1, 2])
@pytest.mark.parametrize("E", [8, 16])
def test_folded_route_with_skewed_gates_and_empty_slabs(E, prec):
    """Gate biases send every token's first choice to one expert per branch and shut two experts per branch out: one slab of M
    rows, empty slabs (goff[e] == goff[e + 1]) before, between and after the occupied ones."""
    m, gates = model(512, E)
    _skew(m, gates, E)
    try:
        counts = fold_vs_launch(512, E, prec, 3, 40, expect_empty=True)
    finally:
        m.load_state_dict(gates, strict=False)
    M = 120
    assert int(counts[5]) >= M and int(counts[E + E - 2]) >= M
    assert counts[[0, 1, E + 3, E + 4]].tolist() == [0, 0, 0, 0], counts.tolist()


@pytest.mark.parametrize("prec", [1, 2])
def test_forced_routing_through_the_folded_path(prec):
    E, B, T = 8, 3, 40
    gen = torch.Generator().manual_seed(3)
    first = torch.randint(0, E, (2, 2, B * T), generator=gen)
    second = (first + torch.randint(1, E, (2, 2, B * T), generator=gen)) % E
    forced = torch.full((2, 4 * B * T), 0, dtype=torch.int32)
    for li, Ml in ((0, B * T // 2), (1, B * T)):
        forced[li, :4 * Ml] = torch.stack([first[li, :, :Ml], second[li, :, :Ml]], -1).reshape(-1).to(torch.int32)
    fold_vs_launch(512, E, prec, B, T, forced=forced)


@pytest.mark.parametrize("knob", [0, KNOB_LAUNCH])
def test_two_forwards_on_one_stream_accumulate_the_counters(knob):
    """The cursors are zeroed by the producing launch of every forward (check_assignment: they end at the slab sizes, not at twice
    them), and the module buffers hold twice one forward's increments."""
    E, B, T, prec = 8, 3, 40, 1
    m, _ = model(512, E)
    inp = inputs(B, T)
    m.reset_all_moe_counters()
    out1, idx1, r1 = forward(m, prec, inp, knob)
    m.reset_all_moe_counters()
    out2, idx2, r2 = forward(m, prec, inp, knob, calls=2)
    what = f"two forwards, knob {knob}"
    assert torch.equal(out1, out2) and all(torch.equal(a, b) for a, b in zip(idx1, idx2))
    same_route(r1, r2, what)
    check_assignment(r2, B * T, E, what)
    check_importance(m, "high", r2, E, 2, what)


@pytest.mark.parametrize("D,prec", [(256, 1), (256, 2), (512, 3)])
def test_ineligible_shapes_and_modes_keep_the_router_launches(D, prec):
    """D = 256 (no one-launch stylization) and the fp32-grade mode take the three-launch router whatever the knob says: knob 171
    changes nothing, and the routing is a consistent assignment."""
    E, B, T = 8, 3, 40
    m, _ = model(D, E)
    inp = inputs(B, T)
    out0, idx0, r0 = forward(m, prec, inp, 0)
    out1, idx1, r1 = forward(m, prec, inp, KNOB_LAUNCH)
    check_assignment(r0, B * T, E, f"D={D} precision {prec}")
    assert torch.equal(out0, out1) and all(torch.equal(a, b) for a, b in zip(idx0, idx1))
    assert torch.equal(r0["top_val"], r1["top_val"]) and torch.equal(r0["goff"], r1["goff"])

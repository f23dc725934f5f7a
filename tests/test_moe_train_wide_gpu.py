"""GPU: the MoE block's training step (csrc/moe_train.hip) at the widths a big model runs and at the shapes that open its other
code paths, against fp64 autograd through the oracle's forward (oracle/moe_train_ref.py) on the HIP router's decisions.

The paths each shape opens are listed beside SHAPES.  Gate: 2e-4 of each tensor's largest entry.  Every GEMM of the step is
bf16x3: each product a*b loses at most the lo*lo term and the bf16 rounding of the lo halves, ~2^-17 |a||b|, with random
signs, so a K-term dot product is off by ~1e-5 of its own size at any K (the error and the sum both grow like sqrt(K)); the
row kernels, column sums and split-K partials are fp32, ~1e-6 of the result.  The fp32 oracle itself is within 6.5e-6 of
the fp64 one at D = 1024.  A row dropped or counted twice in a column sum or split-K chunk moves a gradient by ~1/M of its
largest entry: > 1e-3 for M <= 1000, and the single-row probes below turn it into a 100 % error at every M."""
import pytest
import torch

from conftest import pkg, rel_inf
from oracle import denoiser_ref as R
from oracle import moe_train_ref as T
from test_moe_train_gpu import PREFIX, _hip_forward_backward, _inputs, _make_sd, _trainer

pytestmark = pytest.mark.gpu
GATE = 2e-4
NSK = 32  # K chunks of the split-K weight gradients (moe_train.hip)
EXPERT = ("w1", "b1", "w2", "b2")

_SD = {}


def _sd(D, F, E, Te, seed):
    """_make_sd memoised per shape: the big blocks take seconds to draw on the host (treated as read-only)."""
    key = (D, F, E, Te, seed)
    if key not in _SD:
        _SD[key] = _make_sd(D, F, E, Te, seed)
    return _SD[key]


def _free_routing(sd, E, x, emb, eph):
    """The oracle's own top-2 decisions in fp32, per branch (M, 2)."""
    trace = {}
    with torch.no_grad():
        R.moe_ffn(x, emb, sd, PREFIX, E, eph, trace=trace)
    return [trace[f"{PREFIX}.branches.{b}.top2_idx"] for b in range(2)]


def _grad_errs(tr, E, o_g, sd):
    errs = {}
    for name, ks in pkg("moe_train").reference_keys(PREFIX, E).items():
        g = tr.grads.views[name].cpu()
        ref = torch.stack([o_g[k] if o_g.get(k) is not None else torch.zeros_like(sd[k]) for k in ks]).reshape(g.shape)
        errs["d" + name] = rel_inf(g, ref)
    return errs


SHAPES = [
    (1024, 2048, 8, 4096, 4096, 4, 196),   # big block: <16,true> row kernels, 80 KB gate/LN LDS
    (1024, 2048, 8, 4096, 1024, 2, 24),    # same, with the captured eph projection (De != Te)
    (1024, 2048, 16, 4096, 4096, 2, 196),  # configs[4] block: 144 KB LDS, E = 16 router on fp32 rows
    (512, 1024, 16, 2048, 2048, 3, 37),    # 72 KB LDS opt-in at <8,true>
    (768, 1536, 16, 3072, 1024, 2, 33),    # <16,false> row kernels, 108 KB LDS, eph, row-kernel router
    (1000, 2000, 4, 1000, 1000, 2, 29),    # no bf16 planes (fp32 and k-strided expert weights), wide <16,false>
    (100, 200, 3, 64, 64, 5, 7),           # no planes, narrow <4,false>, M = 35: short and empty trailing split-K chunks
    (1024, 2048, 16, 4096, 4096, 1, 5),    # M = 5 < NSK at full width (27 empty split-K chunks), most expert groups empty
    (1024, 2048, 8, 4096, 4096, 32, 196),  # bench size, M = 6272
]


@pytest.mark.parametrize("D,F,E,Te,De,B,S", SHAPES)
def test_wide_block_gradients_match_fp64_autograd(D, F, E, Te, De, B, S):
    sd = _sd(D, F, E, Te, seed=D + E)
    x, emb, eph, dout = _inputs(B, S, D, De, Te, seed=S)
    tr = _trainer(D, F, E, Te, sd)
    for v in tr.grads.views.values():
        v.fill_(float("nan"))  # the backward overwrites every gradient
    out, dx, demb, route, lb = _hip_forward_backward(tr, x, emb, eph, dout)
    free = _free_routing(sd, E, x, emb, eph)
    for b in range(2):
        assert torch.equal(free[b], route[b]), f"branch {b}: routing differs from the oracle's fp32 routing"
    o_out, o_dx, o_demb, o_g, o_lb, _ = T.moe_ffn_grads(sd, PREFIX, E, x, emb, eph, dout, dtype=torch.float64, forced=route)
    errs = {"out": rel_inf(out, o_out), "dx": rel_inf(dx, o_dx), "demb": rel_inf(demb, o_demb), "lb_loss": rel_inf(lb, o_lb)}
    errs.update(_grad_errs(tr, E, o_g, sd))
    used = [len(set(route[b].flatten().tolist())) for b in range(2)]
    print(f"MoE block training vs fp64 D={D} F={F} E={E} De={De} B*S={B * S} (experts used {used[0]}+{used[1]} of {2 * E}): "
          + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) < GATE, errs


def _oracle_graph(sd, E, x, emb, eph, forced):
    """fp64 forward of the oracle on fixed routing, kept for several backward passes: (out, [x, emb, params...], keys)."""
    keys = [k for k in sd if k.startswith(PREFIX + ".")]
    p = {k: sd[k].detach().double().clone().requires_grad_(True) for k in keys}
    xd = x.detach().double().clone().requires_grad_(True)
    ed = emb.detach().double().clone().requires_grad_(True)
    ephd = None if eph is None else (eph[0].double(), eph[1].double())
    out = T.moe_ffn_train(xd, ed, p, PREFIX, E, ephd, forced=forced)
    return out, [xd, ed] + [p[k] for k in keys], keys


@pytest.mark.parametrize("D,F,E,Te,De,B,S,rows", [
    (1024, 2048, 8, 4096, 4096, 4, 196, (0, 24, 25, 774, 775, 783)),  # M = 784, chunk 25: first / last rows of chunks 0, 30, 31
    (100, 200, 3, 64, 64, 5, 7, (0, 1, 2, 33, 34)),                   # M = 35, chunk 2: chunk 17 is one row, 18..31 are empty
])
def test_single_row_gradients_probe_every_reduction_boundary(D, F, E, Te, De, B, S, rows):
    """dout is zero except on one row r: every gradient is then that row's contribution alone, so a column sum or split-K
    chunk (NSK = 32 chunks of ceil(M / 32) rows) that drops r, or adds it twice, is a 100 % error rather than a 1 / M one.
    The probes sit on both sides of the first and last chunk boundaries.  Expert groups r was not routed to must get
    exactly zero gradients: their rows carry exact zeros through every GEMM and column sum.

    A single row also exposes the conditioning of the gate's softmax backward, dl_e = p_e (dp_e - p1 dp1 - p2 dp2).  Row 24
    of the D = 1024 case routes with p1 = 0.99972 and 0.999996: the routed entries are ~p2 (dp1 - dp2), and a plain fp32
    dp1 - c cancels to the rounding of c (fp32 autograd itself is off by 2.5e-2 there).  The kernel sums 1 - p1 from the other
    probabilities instead; what remains is dp's own bf16x3 error (~1e-5) times |dp| / |dp1 - dp2| ~ 8 on branch 0: 1.8e-4."""
    M = B * S
    chunk = (M + NSK - 1) // NSK
    assert all(r < M for r in rows) and {0, M - 1} <= set(rows)
    sd = _sd(D, F, E, Te, seed=D + E)
    x, emb, eph, _ = _inputs(B, S, D, De, Te, seed=S)
    tr = _trainer(D, F, E, Te, sd)
    route = None
    worst = {}
    for r in rows:
        dout = torch.zeros(B, S, D)
        dout.view(M, D)[r] = torch.rand(D, generator=torch.Generator().manual_seed(r)) * 2 - 1
        out, dx, demb, rt, lb = _hip_forward_backward(tr, x, emb, eph, dout)
        if route is None:
            route = rt
            free = _free_routing(sd, E, x, emb, eph)
            for b in range(2):
                assert torch.equal(free[b], route[b]), f"branch {b}: routing differs from the oracle's fp32 routing"
            o_out, leaves, keys = _oracle_graph(sd, E, x, emb, eph, route)
        assert torch.equal(rt, route)
        gs = torch.autograd.grad(o_out, leaves, dout.double(), retain_graph=True, allow_unused=True)
        errs = {"dx": rel_inf(dx, gs[0]), "demb": rel_inf(demb, gs[1])}
        errs.update(_grad_errs(tr, E, dict(zip(keys, gs[2:])), sd))
        print(f"single-row probe D={D} M={M} row {r} (chunk {r // chunk}): " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
        worst[r] = max(errs.items(), key=lambda kv: kv[1])
        for name in EXPERT:
            g = tr.grads.views[name].cpu()
            for b in range(2):
                hit = set(route[b][r].tolist())
                for e in range(E):
                    assert (g[b, e].abs().max() > 0) == (e in hit), (r, name, b, e, sorted(hit))
    assert all(v < GATE for _, v in worst.values()), worst


def test_clip_and_adam_at_the_full_parameter_count():
    """clip_grad_norm_ + Adam over the ~1.35e8 parameters of the D = 1024, E = 16 block: sumsq's block cap (1024 blocks,
    float atomics) and adam's grid-stride loop (8192 blocks) at full size, one clipped and one unclipped step against the
    oracle's arithmetic in fp64.  Gates as in test_moe_train_gpu.test_clip_and_adam_match_torch: the updates are ~1e-3 of
    fp32 parameters of order 1, and v ~ (clip g)^2 carries twice the relative error of the norm."""
    D, F, E, Te = 1024, 2048, 16, 4096
    tr = _trainer(D, F, E, Te, _sd(D, F, E, Te, seed=D + E), lr=1e-3, max_norm=1.0)
    n = tr.params.flat.numel()
    assert n > 1.3e8
    g = torch.Generator().manual_seed(5)
    p0 = tr.params.flat.cpu()
    p = p0.double()
    m = torch.zeros(n, dtype=torch.float64)
    v = torch.zeros(n, dtype=torch.float64)
    for step, scale in ((1, 0.5), (2, 1e-5)):  # norms ~3.4e3 (clipped) and ~0.07 (unclipped)
        grads = (torch.rand(n, generator=g) * 2 - 1) * scale
        tr.grads.flat.copy_(grads)
        tr.optimizer_step()
        p, m, v, norm = T.adam_clip_step(p, grads.double(), m, v, step, lr=1e-3, max_norm=1.0)
        del grads
        e_norm = abs(tr.grad_norm() - float(norm)) / float(norm)
        e_upd = rel_inf(tr.params.flat.cpu() - p0, p - p0.double())
        e_v = rel_inf(tr.adam_v.cpu(), v)
        print(f"clip + Adam, {n} parameters, step {step}: norm {float(norm):.3e} (rel err {e_norm:.1e}), update {e_upd:.1e}, "
              f"adam_v {e_v:.1e}")
        assert (float(norm) > 1.0) == (step == 1)
        assert e_norm <= 1e-5
        assert e_upd < 2e-4
        assert e_v < 1e-4


@pytest.mark.parametrize("D,E", [(1056, 8), (1024, 17), (1024, 1)])
def test_shapes_outside_the_documented_limits_are_refused(D, E):
    """D <= 1024 and 2 <= E <= 16: the workspace query answers -1, the trainer raises before any launch, and the C entries
    return MDM_ERR_ARG without touching their outputs."""
    import ctypes as C

    L = pkg("_lib")
    lib = L.lib()
    F, Te, B, S = 64, 64, 2, 4
    assert lib.mdm_moe_train_workspace_bytes(B, S, D, F, E, Te) == -1
    tr = pkg("moe_train").MoEFFNTrainer(D, F, E, Te, device="cuda")
    x, emb = torch.zeros(B, S, D, device="cuda"), torch.zeros(B, Te, device="cuda")
    with pytest.raises(L.MdmError, match="unsupported MoE training shape"):
        tr.forward(x, emb)
    ws = torch.zeros(lib.mdm_moe_train_workspace_bytes(B, S, 1024, F, 16, Te), dtype=torch.uint8, device="cuda")
    out = torch.full_like(x, 7.0)
    lb = torch.full((2,), 7.0, device="cuda")
    vp = lambda t: C.c_void_p(t.data_ptr())
    rc = lib.mdm_moe_ffn_train_forward(C.byref(tr.params.struct), D, F, E, Te, Te, None, None, vp(x), vp(emb), B, S, C.c_float(0.0),
                                       C.c_uint64(0), vp(out), vp(lb), None, vp(ws), C.c_int64(ws.numel()), C.c_void_p(L.stream_ptr()))
    assert rc == 1, rc  # MDM_ERR_ARG
    dx = torch.full_like(x, 7.0)
    rc = lib.mdm_moe_ffn_train_backward(C.byref(tr.params.struct), D, F, E, Te, Te, None, vp(x), vp(emb), B, S, C.c_float(0.0),
                                        C.c_uint64(0), vp(x), vp(dx), None, C.byref(tr.grads.struct), vp(ws), C.c_int64(ws.numel()),
                                        C.c_void_p(L.stream_ptr()))
    assert rc == 1, rc
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((lb == 7.0).all()) and bool((dx == 7.0).all())


@pytest.mark.parametrize("D", [768, 1000, 100])
def test_dropout_outside_the_vector_widths_is_refused(D):
    """Dropout masks are generated per float4 chunk of the vectorised rows: D in {256, 512, 1024} only; any other width is
    MDM_ERR_UNSUPPORTED from forward and backward alike, not a silently unmasked step."""
    L = pkg("_lib")
    tr = pkg("moe_train").MoEFFNTrainer(D, 64, 4, 64, device="cuda", dropout=0.1)
    with pytest.raises(L.MdmError, match="mdm_moe_ffn_train_forward failed: MDM_ERR_UNSUPPORTED"):
        tr.forward(torch.zeros(1, 4, D, device="cuda"), torch.zeros(1, 64, device="cuda"))

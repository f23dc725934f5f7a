"""GPU: the scratch-taking C entries beside the denoiser.  Each gets a guarded window (tests/scratch_hygiene.py) of exactly the size its
query returns; its results must be bit-equal under two histories of that window -- zeros and 0xFF bytes (NaN as fp32) where the
scratch is float-only, zeros and a donor run's bytes where it also holds indices (the MoE training workspace) -- with the guards
untouched, and one byte less must be MDM_ERR_ARG with every output's sentinel intact.

mdm_text_head_forward, mdm_gru_bidir and the two MoE training calls take the scratch's size; mdm_canvas_joint_loss_grad,
mdm_partner_tracks, mdm_motion_render and mdm_world_render take a bare pointer (the query is the contract), so they have no call
to refuse: those four are run through their Python layer, whose one scratch allocation is replaced by the window."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import pkg, rel_inf
import scratch_hygiene as SH

pytestmark = pytest.mark.gpu

FILLS = ("Z", "P")


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ---- mdm_text_head_forward ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [3, 1])
@pytest.mark.parametrize("B,N0,Hs,Dt", [(3, 5, 64, 32), (1, 5, 1024, 256)], ids=["3x5x64x32", "1x5x1024x256"])
def test_text_head(B, N0, Hs, Dt, precision):
    L = pkg("_lib")
    lib = L.lib()
    TH = pkg("text_head")
    torch.manual_seed(Hs + B)
    enc = TH.EnhancedTextEncoder(Dt, hidden_size=Hs, precision=precision).cuda()
    P = enc.num_prompt_tokens
    pw = enc._weights()
    packed = L.Packed(pw.hi.data_ptr(), pw.lo.data_ptr(), pw.Kp)
    hidden = torch.randn(B, N0, Hs, device="cuda")
    prompts = enc.prompt_tokens.detach().float().reshape(P, Hs).contiguous()
    ln, lin = enc.proj[0], enc.proj[1]
    need = lib.mdm_text_head_workspace_bytes(B, N0, P, Hs, Dt)
    assert need > 0

    def call(ws, nbytes, xf_out, xf_proj):
        return lib.mdm_text_head_forward(hidden.data_ptr(), prompts.data_ptr(), ln.weight.data_ptr(), ln.bias.data_ptr(), C.byref(packed),
                                         lin.bias.data_ptr(), B, N0, P, Hs, Dt, xf_out.data_ptr(), xf_proj.data_ptr(), ws.data_ptr(),
                                         nbytes, precision, L.stream_ptr())

    res = {}
    for fill in FILLS:
        g = SH.guarded(need)
        SH.fill_float_scratch(g.win, fill)
        go, xo = SH.guarded_like((B, P + N0, Dt), fill=7.0)
        gp, xp = SH.guarded_like((B, Dt), fill=7.0)
        assert call(g.win, need - 1, xo, xp) == SH.ERR_ARG
        torch.cuda.synchronize()
        assert bool((xo == 7.0).all()) and bool((xp == 7.0).all()) and bool((g.win == (0 if fill == "Z" else SH.POISON_BYTE)).all())
        assert call(g.win, need, xo, xp) == 0
        torch.cuda.synchronize()
        assert g.guards_untouched() and go.guards_untouched() and gp.guards_untouched()
        res[fill] = (xo, xp)
    assert torch.isfinite(res["Z"][0]).all() and torch.isfinite(res["Z"][1]).all() and not bool((res["Z"][0] == 7.0).any())
    assert _same(res["Z"][0], res["P"][0]) and _same(res["Z"][1], res["P"][1])
    want = enc.project(hidden)  # the Python layer computes the same
    assert _same(want[1], res["Z"][0]) and _same(want[0], res["Z"][1])


# ---- mdm_gru_bidir -----------------------------------------------------------------------------------------------------------------
def test_gru_bidir():
    """B = 3, T = 7, H = 16, lengths [7, 1, 4]; against torch's GRU cell recurrence in fp64 as well (a poisoned scratch that is read
    shows as NaN, a zeroed one that is read as a wrong state)."""
    L = pkg("_lib")
    lib = L.lib()
    B, T, H = 3, 7, 16
    lens = np.array([7, 1, 4], dtype=np.int32)
    g = torch.Generator().manual_seed(7)
    r = lambda *s: (torch.rand(*s, generator=g) * 2 - 1)  # noqa: E731
    gx, w_hh, b_hh, h0 = r(B, T, 2, 3 * H), r(2, 3 * H, H) * H ** -0.5, r(2, 3 * H) * 0.1, r(2, H)
    dev = [v.cuda().contiguous() for v in (gx, w_hh, b_hh, h0)]
    ld = torch.from_numpy(lens).cuda()
    need = lib.mdm_gru_bidir_workspace_bytes(B, H)
    assert need > 0

    def call(ws, nbytes, out):
        return lib.mdm_gru_bidir(*[v.data_ptr() for v in dev], ld.data_ptr(), lens.ctypes.data, B, T, H, out.data_ptr(), ws.data_ptr(),
                                 nbytes, L.stream_ptr())

    res = {}
    for fill in FILLS:
        gw = SH.guarded(need)
        SH.fill_float_scratch(gw.win, fill)
        go, out = SH.guarded_like((B, 2 * H), fill=7.0)
        assert call(gw.win, need - 1, out) == SH.ERR_ARG
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()) and bool((gw.win == (0 if fill == "Z" else SH.POISON_BYTE)).all())
        assert call(gw.win, need, out) == 0
        torch.cuda.synchronize()
        assert gw.guards_untouched() and go.guards_untouched()
        res[fill] = out
    assert _same(res["Z"], res["P"])
    # fp64 recurrence (torch.nn.GRU's gate order r, z, n): direction 0 runs t = 0 .. len - 1, direction 1 t = len - 1 .. 0
    ref = torch.zeros(B, 2 * H, dtype=torch.float64)
    for b in range(B):
        for d in range(2):
            h = h0[d].double()
            order = range(int(lens[b])) if d == 0 else range(int(lens[b]) - 1, -1, -1)
            for t in order:
                gi, gh = gx[b, t, d].double(), w_hh[d].double() @ h + b_hh[d].double()
                rg = torch.sigmoid(gi[:H] + gh[:H])
                zg = torch.sigmoid(gi[H:2 * H] + gh[H:2 * H])
                ng = torch.tanh(gi[2 * H:] + rg * gh[2 * H:])
                h = (1 - zg) * ng + zg * h
            ref[b, d * H:(d + 1) * H] = h
    err = rel_inf(res["Z"].cpu(), ref)
    print(f"gru_bidir vs fp64 recurrence: {err:.2e}")
    assert err < 1e-5  # fp32 arithmetic over at most 7 steps of a contraction


# ---- mdm_moe_ffn_train_forward / _backward -------------------------------------------------------------------------------------------
def test_moe_training_workspace():
    """The smallest case of tests/test_moe_train_gpu.py (D = 64, F = 128, E = 3, B = 2, S = 7) in a guarded window of exactly
    mdm_moe_train_workspace_bytes.  The workspace holds the router's indices and carries the forward's state to the backward, so the
    fills are zeros and the bytes a donor step (other x, emb and dout) left.  A same-fill repeat is compared first: what it
    reproduces bit for bit must be bit-equal between the fills; anything it does not is held to the oracle at that file's gate
    (2e-3 of the largest entry) under each fill.  Not repeatable are the four LayerNorm-parameter gradients (dln_w, dln_b,
    dst_norm_w, dst_norm_b): csrc/moe_train.hip sums the rows' contributions into LDS and then into the gradient with
    floating-point atomicAdd, in an order that changes from run to run."""
    from oracle import moe_train_ref as T
    import test_moe_train_gpu as MT
    L = pkg("_lib")
    lib = L.lib()
    D, F, E, Te, De, B, S = 64, 128, 3, 64, 64, 2, 7
    sd = MT._make_sd(D, F, E, Te, seed=D + E)
    x, emb, eph, dout = MT._inputs(B, S, D, De, Te, seed=S)
    xd, embd, _, doutd = MT._inputs(B, S, D, De, Te, seed=S + 50)
    tr = MT._trainer(D, F, E, Te, sd)
    need = lib.mdm_moe_train_workspace_bytes(B, S, D, F, E, Te)
    gw = SH.guarded(need)
    tr._ws, tr._shape = gw.win, (B, S)

    def step(x_, emb_, dout_):
        for v in tr.grads.views.values():
            v.fill_(float("nan"))
        route = torch.zeros(2, B * S, 2, dtype=torch.int32, device="cuda")
        out = tr.forward(x_.cuda(), emb_.cuda(), None, route_out=route)
        dx, demb = tr.backward(dout_.cuda())
        torch.cuda.synchronize()
        assert tr._ws is gw.win and gw.guards_untouched()
        r = {"out": out, "dx": dx, "demb": demb, "route": route, "lb_loss": tr.lb_loss.clone()}
        r.update({"d" + k: v.clone() for k, v in tr.grads.views.items()})
        return r

    gw.win.zero_()
    step(xd, embd, doutd)
    donor = gw.win.clone()
    runs = {}
    for name, fill in (("Z", None), ("Z2", None), ("D", donor)):
        gw.win.zero_() if fill is None else gw.win.copy_(fill)
        runs[name] = step(x, emb, dout)
    # by construction, not by luck: at 4 B S = 56 slab rows every column sum (colsum_kernel: one atomic per block of 256 rows) has
    # one addend, and the split-K partials are summed in a fixed order; only the LayerNorm-parameter gradients go through atomics
    unordered = {"dln_w", "dln_b", "dst_norm_w", "dst_norm_b"}
    print("differ between two runs from zeros:", sorted(k for k in runs["Z"] if not _same(runs["Z"][k], runs["Z2"][k])))
    for k in sorted(set(runs["Z"]) - unordered):
        assert _same(runs["Z"][k], runs["Z2"][k]), f"{k} is not repeatable from the same workspace contents"
        assert _same(runs["Z"][k], runs["D"][k]), f"{k} depends on what the workspace held before the step"
    o_out, o_dx, o_demb, o_g, o_lb, trace = T.moe_ffn_grads(sd, MT.PREFIX, E, x, emb, eph, dout)
    ref = {"out": o_out, "dx": o_dx, "demb": o_demb, "lb_loss": o_lb}
    for name, ks in pkg("moe_train").reference_keys(MT.PREFIX, E).items():
        ref["d" + name] = torch.stack([o_g.get(k, torch.zeros_like(sd[k])) for k in ks]).reshape(tr.grads.views[name].shape)
    for fill in ("Z", "D"):
        for b in range(2):
            assert torch.equal(trace[f"{MT.PREFIX}.branches.{b}.top2_idx"], runs[fill]["route"][b].cpu().long())
        errs = {k: rel_inf(runs[fill][k].cpu(), v) for k, v in ref.items()}
        print(f"fill {fill} vs the oracle: " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
        assert max(errs.values()) < 2e-3, (fill, errs)

    # one byte less: refused before any launch, by both calls
    s = tr.params.struct
    out, lb = torch.full((B, S, D), 7.0, device="cuda"), torch.full((2,), 7.0, device="cuda")
    xg, eg, dg = x.cuda().contiguous(), emb.cuda().contiguous(), dout.cuda().contiguous()
    gw.win.copy_(donor)
    assert lib.mdm_moe_ffn_train_forward(C.byref(s), D, F, E, Te, De, None, None, xg.data_ptr(), eg.data_ptr(), B, S, 0.0, 0, out.data_ptr(),
                                         lb.data_ptr(), None, gw.win.data_ptr(), need - 1, L.stream_ptr()) == SH.ERR_ARG
    dx, demb = torch.full((B, S, D), 7.0, device="cuda"), torch.full((B, De), 7.0, device="cuda")
    tr.grads.flat.fill_(7.0)
    assert lib.mdm_moe_ffn_train_backward(C.byref(s), D, F, E, Te, De, None, xg.data_ptr(), eg.data_ptr(), B, S, 0.0, 0, dg.data_ptr(),
                                          dx.data_ptr(), demb.data_ptr(), C.byref(tr.grads.struct), gw.win.data_ptr(), need - 1,
                                          L.stream_ptr()) == SH.ERR_ARG
    torch.cuda.synchronize()
    assert all(bool((v == 7.0).all()) for v in (out, lb, dx, demb, tr.grads.flat))
    assert torch.equal(gw.win, donor) and gw.guards_untouched()


# ---- entries that take a bare scratch pointer: through their Python layer ---------------------------------------------------------------
class _TorchWithScratch:
    """`torch` for one module of the package: its first 1-D float32 torch.empty of `floats` elements returns the guarded window."""

    def __init__(self, window, floats):
        self._window, self._floats, self.taken = window, floats, 0

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *a, **kw):
        t = torch.empty(*a, **kw)
        if t.dim() == 1 and t.dtype == torch.float32 and t.numel() == self._floats and t.is_cuda and not self.taken:
            self.taken += 1
            return self._window
        return t


@contextlib.contextmanager
def _scratch_of(module, floats, fill):
    """Inside: `module` allocates its scratch of `floats` floats as a guarded window holding `fill`; after: the window was used and
    its guards are untouched."""
    assert floats > 0
    g = SH.guarded(4 * floats)
    SH.fill_float_scratch(g.win, fill)
    proxy = _TorchWithScratch(g.win.view(torch.float32), floats)
    real, module.torch = module.torch, proxy
    try:
        yield g
        torch.cuda.synchronize()
    finally:
        module.torch = real
    assert proxy.taken == 1, "the call did not allocate a scratch of the queried size"
    assert g.guards_untouched(), "a write outside the scratch"


def _two_fills(module, floats, run):
    res = {}
    for fill in FILLS:
        with _scratch_of(module, floats, fill):
            res[fill] = run()
    z, p = res["Z"], res["P"]
    for a, b in zip(z, p):
        assert _same(a, b), "the result depends on what the scratch held before the call"
    return z


def test_canvas_joint_loss_grad():
    """Two motions of 10 and 7 canvas frames on two window rows of 12 frames, F = 263."""
    MC = pkg("motion_control")
    F, J, Tw, lens = 263, 22, 12, (10, 7)
    g = torch.Generator().manual_seed(17)
    x = torch.randn(2, Tw, F, generator=g) * 0.7
    off = torch.tensor([0, 10, 17])
    fr = torch.cat([1 * Tw + torch.arange(10), 0 * Tw + torch.arange(7)])
    mean, std = torch.randn(2, F, generator=g) * 0.2, torch.rand(2, F, generator=g) + 0.5
    std[:, 0], mean[:, 0] = 0.05, mean[:, 0] * 0.1
    tg = torch.randn(17, J, 3, generator=g) * 2.0
    w = torch.rand(17, J, 3, generator=g)
    w[w < 0.3] = 0.0
    floats = int(pkg("_lib").lib().mdm_canvas_control_workspace_floats(sum(lens), F))
    loss, grad = _two_fills(MC, floats, lambda: MC.canvas_loss_grad(x.cuda(), off, fr, mean, std, tg, w))
    assert torch.isfinite(loss).all() and torch.isfinite(grad).all() and bool((loss > 0).all()) and bool(grad.abs().sum() > 0)


def test_partner_tracks():
    """One pair, 6 frames (lengths 6 and 4), every bone a capsule, one contact."""
    MS = pkg("motion_scene")
    B, T, F, J = 2, 6, 263, 22
    g = torch.Generator().manual_seed(6)
    x0 = torch.randn(B, T, F, generator=g) * 0.7
    mean, std = torch.randn(B, F, generator=g) * 0.2, torch.rand(B, F, generator=g) + 0.5
    std[:, 0], mean[:, 0] = std[:, 0] * 0.1, mean[:, 0] * 0.1
    lens = torch.tensor([6, 4])
    pose = torch.tensor([[0.0, 0.0, 0.0], [0.25, -0.15, 0.7]], dtype=torch.float64)
    contacts = [MS.contact(0, J - 1, 1, J - 2, range(0, T), weight=2.0, meet=0.3)]
    tables = MS.partner_tables([[0, 1]], pose, lens, MS.skeleton_bones(J), T=T, J=J, contacts=contacts, radius=0.3, margin=0.05, weight=5.0)
    floats = MS.partner_scratch_floats(B, T, F)
    tracks, bounds, targets, world = _two_fills(MS, floats, lambda: MS.partner_tracks(x0.cuda(), lens, mean, std, tables, return_world=True))
    assert all(bool(torch.isfinite(v).all()) for v in (tracks, targets, world)) and bool(tracks.abs().sum() > 0)
    assert not bool(torch.isnan(bounds).any())


def test_motion_render():
    """One 32 x 32 frame (frame 1 of a two-frame walk: the trajectory behind the figure goes through the scratch)."""
    import render_ref as RR
    import world_render_ref as WR
    MR = pkg("motion_render")
    sk = WR.skel("t2m")
    j = torch.from_numpy(RR.walk(sk, 2, 2)[None]).cuda()
    floats = int(pkg("_lib").lib().mdm_motion_render_scratch_floats(1, 2))
    (out,) = _two_fills(MR, floats, lambda: (MR.render_motion(j, [2], size=(32, 32), frames=[1]),))
    assert out.shape == (1, 1, 32, 32, 3) and int((out != 255).any(-1).sum()) > 30  # a figure and a floor


def test_world_render():
    """One 32 x 32 frame of the first world of tests/test_world_render_gpu.py's parity batch: two characters, five primitives."""
    import world_render_ref as WR
    MR = pkg("motion_render")
    sk, j, lens, prims = WR.static_world("t2m")
    j, lens, prims = torch.from_numpy(j[:1]).cuda(), lens[:1], torch.from_numpy(prims[:1])
    cam = dict(elev=60.0, azim=135.0, dist=4.0, fov=60.0)
    floats = int(pkg("_lib").lib().mdm_world_render_scratch_floats(1, 2, 5, 1, prims.shape[1], 0))
    (out,) = _two_fills(MR, floats, lambda: (MR.render_world(j, lens, scene=prims, size=(32, 32), camera=cam, frames=[1]),))
    assert out.shape == (1, 1, 32, 32, 3) and int((out != 255).any(-1).sum()) > 100

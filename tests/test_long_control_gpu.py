"""GPU: joint-position control over the canvas of a long motion.

* mdm_canvas_joint_loss_grad against the fp64 autograd restatement of tests/test_motion_control_host.py over canvases of
  1, 2, 255, 256, 257, 513 and 600 frames (and an empty one), three motions of unequal length per call, F = 263 and 251,
  the canvas frames spread over window rows in shuffled order with padded rows between them, dense / keyframe / fractional
  weights, exact zeros in the columns that cannot be steered; a target at the end of a three-window canvas reaches the root
  velocities of frame 0;
* mdm_canvas_joint_guidance: single-window canvases agree with mdm_joint_guidance, all-zero weights, rows the table does
  not name and masked entries keep their bits, the argument errors;
* every sampler on a plain and a respaced schedule, graph and eager, three windows of 16 / 12 / 16 frames at h = 4 (a
  36-frame canvas on loops_tiny): the overlaps are bit-equal in x and x0 after every step, every step agrees with the loop
  restated in tests/sampler_ref.py (handshake blend, update, fp64 guidance over the canvas, owner copy), graph == eager and
  two streams == one bitwise, a canvas prefix edit keeps its frames;
* the trainer: batch split, joints front end, a pelvis path over the canvas is followed, the configs[1] widths in bf16.
"""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

from conftest import pkg, rel_inf
from test_motion_control_host import ref_loss_grad

import sampler_ref as S
from sampler_ref import caption_trainer as _trainer, make_diffusion as _diffusion, vp as _vp

pytestmark = pytest.mark.gpu


def _stats(F, M, seed):
    """mean / std (M, F): std in [0.5, 1.5], 0.05 on the heading velocity (small per frame, as in HumanML3D)."""
    g = torch.Generator().manual_seed(seed)
    mean = torch.randn(M, F, generator=g) * 0.2
    std = torch.rand(M, F, generator=g) + 0.5
    std[:, 0] = 0.05
    mean[:, 0] *= 0.1
    return mean, std


def _weights(kind, n, J, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.zeros(n, J, 3)
    if kind == "keys":  # root XZ and one hand on a few keyframes
        for f in sorted({0, n // 3, n // 2, n - 1}):
            w[f, 0, 0] = w[f, 0, 2] = 1.0
            w[f, J - 1] = 1.0
    elif kind == "all":
        w[:] = 1.0
    else:  # fractional weights, some zero
        w = torch.rand(n, J, 3, generator=g)
        w[w < 0.3] = 0.0
    return w


def _layout(canvases, Tw, seed):
    """Canvases cut into windows of at most Tw - 3 frames, the windows dealt to batch rows in shuffled order, every row
    padded to Tw: (number of batch rows, motion_offsets, frame_rows = window_row * Tw + frame)."""
    rng = np.random.RandomState(seed)
    wins = [(m, s, min(Tw - 3, n - s)) for m, n in enumerate(canvases) for s in range(0, n, Tw - 3)]
    slot = rng.permutation(len(wins) + 1)  # one batch row stays unused
    rows = [np.zeros(n, np.int64) for n in canvases]
    for k, (m, s, ln) in enumerate(wins):
        rows[m][s:s + ln] = slot[k] * Tw + np.arange(ln)
    off = np.concatenate([[0], np.cumsum(canvases)]).astype(np.int64)
    return len(wins) + 1, torch.from_numpy(off), torch.from_numpy(np.concatenate(rows) if rows else np.zeros(0, np.int64))


def _canvas_ref(x, off, fr, mean, std, tg, w):
    """fp64 loss (M,) and gradient (total, F) in canvas order: the restatement run on each motion's rows gathered into
    canvas order."""
    F = x.shape[-1]
    flat = x.reshape(-1, F).cpu()
    loss, grad = [], torch.zeros(fr.numel(), F, dtype=torch.float64)
    for m in range(off.numel() - 1):
        a, b = int(off[m]), int(off[m + 1])
        if b == a:
            loss.append(torch.zeros((), dtype=torch.float64))
            continue
        l, g = ref_loss_grad(flat[fr[a:b]][None], [b - a], mean[m], std[m], tg[a:b][None], w[a:b][None])
        loss.append(l[0])
        grad[a:b] = g[0]
    return torch.stack(loss), grad


@functools.lru_cache(maxsize=None)
def _grad_case(canvases, F, kind):
    J, Tw = (F + 1) // 12, 200
    gen = torch.Generator().manual_seed(sum(canvases) * 7 + F)
    B, off, fr = _layout(canvases, Tw, sum(canvases) + F)
    x = torch.randn(B, Tw, F, generator=gen) * 0.7
    mean, std = _stats(F, len(canvases), F + len(canvases))
    total = int(off[-1])
    tg = torch.randn(total, J, 3, generator=gen) * 2.0
    w = torch.cat([_weights(kind, n, J, n + F) for n in canvases if n]) if total else torch.zeros(0, J, 3)
    return x, off, fr, mean, std, tg, w, _canvas_ref(x, off, fr, mean, std, tg, w)


# ---- mdm_canvas_joint_loss_grad -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [263, 251])
@pytest.mark.parametrize("canvases", [(1, 2, 255), (256, 257, 513), (600, 0, 37)])
def test_canvas_loss_grad_matches_fp64_autograd(canvases, F):
    M = pkg("motion_control")
    D = 3 * ((F + 1) // 12) + 1
    worst_l = worst_g = 0.0
    for kind in ("keys", "all", "frac"):
        x, off, fr, mean, std, tg, w, (rl, rg) = _grad_case(canvases, F, kind)
        assert len(set((fr // 200).tolist())) > 1 and bool((fr[1:] < fr[:-1]).any())  # several rows, not in order
        loss, grad = M.canvas_loss_grad(x.cuda(), off, fr, mean, std, tg, w)
        loss, grad = loss.cpu(), grad.cpu()
        assert tuple(grad.shape) == (sum(canvases), F)
        assert torch.equal(grad[:, D:], torch.zeros(sum(canvases), F - D)), kind
        for m, n in enumerate(canvases):
            a = int(off[m])
            if n == 0:
                assert float(loss[m]) == 0.0
                continue
            el = abs(float(loss[m]) - float(rl[m])) / max(float(rl[m]), 1e-30)
            eg = rel_inf(grad[a:a + n], rg[a:a + n])
            print(f"[canvas loss_grad {kind} n={n} F={F}] loss rel {el:.2e} gradient rel_inf {eg:.2e}")
            worst_l, worst_g = max(worst_l, el), max(worst_g, eg)
            assert el <= 1e-5, (kind, m, el)
            assert eg <= 1e-4, (kind, m, eg)
    print(f"[canvas loss_grad {canvases} F={F}] worst loss rel {worst_l:.2e}, worst gradient rel_inf {worst_g:.2e}")


def test_a_target_in_the_last_window_reaches_frame_0():
    """Weights on the last 10 frames of a 513-frame canvas spread over three windows' rows only: the gradient on the root
    velocities (columns 0 - 2) of canvas frame 0, two windows earlier, is non-zero and matches the restatement."""
    M = pkg("motion_control")
    F, J, n, Tw = 263, 22, 513, 180
    gen = torch.Generator().manual_seed(77)
    x = torch.randn(3, Tw, F, generator=gen) * 0.7
    fr = torch.cat([w * Tw + torch.arange(171) for w in (2, 0, 1)])  # 3 x 171 frames, rows not in canvas order
    off = torch.tensor([0, n])
    mean, std = _stats(F, 1, 5)
    tg = torch.randn(n, J, 3, generator=gen) * 2.0
    w = torch.zeros(n, J, 3)
    w[-10:] = 1.0
    loss, grad = M.canvas_loss_grad(x.cuda(), off, fr, mean, std, tg, w)
    rl, rg = _canvas_ref(x, off, fr, mean, std, tg, w)
    grad = grad.cpu()
    assert bool((rg[0, :3] != 0).all()) and bool((grad[0, :3] != 0).all())
    e0 = float((grad[0, :3].double() - rg[0, :3]).abs().max() / rg[0, :3].abs().max())
    e = rel_inf(grad, rg)
    print(f"[cross-window] frame 0 root columns: kernel {grad[0, :3].tolist()} reference {rg[0, :3].tolist()} rel {e0:.2e}; "
          f"whole gradient rel_inf {e:.2e}")
    assert e0 <= 1e-4 and e <= 1e-4
    assert abs(float(loss[0]) - float(rl[0])) <= 1e-5 * float(rl[0])
    assert torch.equal(grad[171 * 3 - 10:, 67:], torch.zeros(10, F - 67))


# ---- mdm_canvas_joint_guidance ------------------------------------------------------------------------------------------
def _guide(x, x0, mask, off, fr, mean, std, tg, w, M, F, scale, iters, coef, steps, t, ws):
    L = pkg("_lib")
    return L.lib().mdm_canvas_joint_guidance(_vp(x), _vp(x0), _vp(mask), _vp(off), _vp(fr), _vp(mean), _vp(std), _vp(tg), _vp(w),
                                             C.c_int32(M), C.c_int32(F), C.c_float(scale), C.c_int32(iters), _vp(coef),
                                             C.c_int32(steps), C.c_void_p(0), C.c_int32(t), _vp(ws),
                                             C.c_void_p(L.stream_ptr()))


def _window_guide(x, x0, mask, lens, mean, std, tg, w, scale, iters, coef, steps, t):
    L = pkg("_lib")
    B, T, F = x0.shape
    return L.lib().mdm_joint_guidance(_vp(x), _vp(x0), _vp(mask), _vp(lens), _vp(mean), _vp(std), _vp(tg), _vp(w),
                                      C.c_int32(B), C.c_int32(T), C.c_int32(F), C.c_float(scale), C.c_int32(iters),
                                      _vp(coef), C.c_int32(steps), C.c_void_p(0), C.c_int32(t), C.c_void_p(L.stream_ptr()))


def _kernel_case(B=3, T=40, F=263, seed=3):
    """Single-window canvases: motion b is the first lens[b] frames of batch row b (identity frame rows)."""
    L = pkg("_lib")
    gen = torch.Generator().manual_seed(seed)
    J = (F + 1) // 12
    x0 = (torch.randn(B, T, F, generator=gen) * 0.7).cuda()
    x = torch.randn(B, T, F, generator=gen).cuda()
    mean, std = (v.cuda().contiguous() for v in _stats(F, B, seed))
    tg = (torch.randn(B, T, J, 3, generator=gen) * 2.0).cuda()
    w = torch.stack([_weights("frac", T, J, seed + b) for b in range(B)]).cuda()
    lens = [T, T // 2, 1][:B]
    off = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32).cuda()
    fr = torch.cat([b * T + torch.arange(n) for b, n in enumerate(lens)]).to(torch.int32).cuda()
    ctg = torch.cat([tg[b, :n] for b, n in enumerate(lens)]).contiguous()
    cw = torch.cat([w[b, :n] for b, n in enumerate(lens)]).contiguous()
    ws = torch.empty(int(L.lib().mdm_canvas_control_workspace_floats(sum(lens), F)), device="cuda")
    return dict(x=x, x0=x0, mean=mean, std=std, tg=tg, w=w, lens=torch.tensor(lens, dtype=torch.int32).cuda(), off=off, fr=fr,
                ctg=ctg, cw=cw, ws=ws, B=B, T=T, F=F)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("iters,scale", [(1, 0.01), (5, 1e-4)])
def test_single_window_canvases_agree_with_the_window_kernel(iters, scale, masked):
    L = pkg("_lib")
    d = _diffusion("ddim10")
    N = d.num_timesteps
    coef = d._device_coef("ddim", 0.0, 2, "cuda")
    c = _kernel_case()
    mask = (torch.rand(c["x0"].shape, generator=torch.Generator().manual_seed(8)) < 0.4).float().cuda() if masked else None
    xa, x0a, xb, x0b = c["x"].clone(), c["x0"].clone(), c["x"].clone(), c["x0"].clone()
    L.check(_window_guide(xa, x0a, mask, c["lens"], c["mean"], c["std"], c["tg"], c["w"], scale, iters, coef, N, 3))
    L.check(_guide(xb, x0b, mask, c["off"], c["fr"], c["mean"], c["std"], c["ctg"], c["cw"], c["B"], c["F"], scale, iters, coef, N,
                   3, c["ws"]))
    assert not torch.equal(x0a, c["x0"])
    e0, e = rel_inf(x0b.cpu(), x0a.cpu()), rel_inf(xb.cpu(), xa.cpu())
    ed = rel_inf((x0b - c["x0"]).cpu(), (x0a - c["x0"]).cpu())  # of the step itself, not hidden behind x0's size
    print(f"[canvas vs window, {iters} iterations, mask {masked}] x0 {e0:.2e} x {e:.2e} delta {ed:.2e}")
    assert e0 <= 1e-5 and e <= 1e-5
    if masked:
        keep = mask == 1
        assert torch.equal(x0b[keep], c["x0"][keep]) and torch.equal(xb[keep], c["x"][keep])


def test_zero_weights_unnamed_rows_and_masked_entries_keep_their_bits():
    L = pkg("_lib")
    d = _diffusion("ddim10")
    N = d.num_timesteps
    coef = d._device_coef("dpmpp", 0.0, 2, "cuda")
    c = _kernel_case()
    x, x0 = c["x"], c["x0"]
    x0[0, :5, :10] = -0.0
    x[0, :5, :10] = -0.0
    bits = lambda v: v.view(torch.int32)  # noqa: E731
    args = lambda w, mask: (mask, c["off"], c["fr"], c["mean"], c["std"], c["ctg"], w, c["B"], c["F"], 0.05, 3, coef, N, 4,  # noqa: E731
                            c["ws"])
    xo, x0o = x.clone(), x0.clone()
    L.check(_guide(xo, x0o, *args(torch.zeros_like(c["cw"]), None)))
    assert torch.equal(bits(xo), bits(x)) and torch.equal(bits(x0o), bits(x0))
    xo, x0o = x.clone(), x0.clone()
    L.check(_guide(xo, x0o, *args(c["cw"], None)))
    named = torch.zeros(c["B"] * c["T"], dtype=torch.bool, device="cuda")
    named[c["fr"].long()] = True
    named = named.view(c["B"], c["T"])
    assert torch.equal(bits(x0o[~named]), bits(x0[~named])) and torch.equal(bits(xo[~named]), bits(x[~named]))
    assert torch.equal(bits(x0o[:, :, 67:]), bits(x0[:, :, 67:])) and torch.equal(bits(xo[:, :, 67:]), bits(x[:, :, 67:]))
    assert not torch.equal(x0o[named], x0[named])
    mask = (torch.rand(x0.shape, generator=torch.Generator().manual_seed(8)) < 0.5).float().cuda()
    xo, x0o = x.clone(), x0.clone()
    L.check(_guide(xo, x0o, *args(c["cw"], mask)))
    keep = mask == 1
    assert torch.equal(bits(x0o[keep]), bits(x0[keep])) and torch.equal(bits(xo[keep]), bits(x[keep]))
    assert not torch.equal(x0o[~keep], x0[~keep])


def test_argument_errors():
    L = pkg("_lib")
    lib = L.lib()
    d = _diffusion("ddim10")
    N = d.num_timesteps
    coef = d._device_coef("ddim", 0.0, 2, "cuda")
    c = _kernel_case()
    a = [c["x"], c["x0"], None, c["off"], c["fr"], c["mean"], c["std"], c["ctg"], c["cw"], c["B"], c["F"], 0.1, 1, coef, N, 0,
         c["ws"]]
    assert _guide(*a) == 0
    for i in (0, 1, 3, 4, 5, 6, 7, 8, 13, 16):
        bad = list(a)
        bad[i] = None
        assert _guide(*bad) == 1, i
    for i, v in ((9, -1), (10, 262), (11, float("nan")), (11, float("inf")), (12, 0), (12, L.CONTROL_MAX_ITERS + 1), (14, 0),
                 (15, N), (15, -1)):
        bad = list(a)
        bad[i] = v
        assert _guide(*bad) == 1, (i, v)
    keep = c["x0"].clone()
    bad = list(a)
    bad[9] = 0  # M == 0: a no-op
    assert _guide(*bad) == 0
    empty = list(a)
    empty[3] = torch.zeros(4, dtype=torch.int32, device="cuda")  # three empty motions
    x0 = c["x0"].clone()
    empty[1] = x0
    assert _guide(*empty) == 0
    torch.cuda.synchronize()
    assert torch.equal(x0, keep)
    s = C.c_void_p(L.stream_ptr())
    total = int(c["off"][-1])
    loss, grad = torch.empty(c["B"], device="cuda"), torch.empty(total, c["F"], device="cuda")
    ptrs = [c["x0"], c["off"], c["fr"], c["mean"], c["std"], c["ctg"], c["cw"]]

    def lg(p, M_=c["B"], F_=c["F"], lo=loss, gr=grad, ws=c["ws"]):
        return lib.mdm_canvas_joint_loss_grad(*[_vp(v) for v in p], C.c_int32(M_), C.c_int32(F_), _vp(lo), _vp(gr), _vp(ws), s)

    assert lg(ptrs) == 0
    for i in range(7):
        bad = list(ptrs)
        bad[i] = None
        assert lg(bad) == 1, i
    assert lg(ptrs, lo=None) == 1 and lg(ptrs, gr=None) == 1 and lg(ptrs, ws=None) == 1
    assert lg(ptrs, F_=262) == 1 and lg(ptrs, M_=-1) == 1 and lg(ptrs, M_=0) == 0
    assert lib.mdm_canvas_control_workspace_floats(724, 263) == 724 * 73 and lib.mdm_canvas_control_workspace_floats(10, 262) == 0
    torch.cuda.synchronize()


# ---- loops --------------------------------------------------------------------------------------------------------------
LENS, H, T = [16, 12, 16], 4, 16
CANVAS = 36
SOLVERS = [("cfg", 0.0), ("ddpm", 0.0), ("cfg_ddim", 0.0), ("cfg_ddim", 0.5), ("ddim", 0.0), ("ddim", 0.5), ("cfg_dpmpp", 0.0)]


def _long_setup():
    ML = pkg("motion_long")
    g, meta, m, noises, _ = S.loops_setup(B=len(LENS))
    sel = [0, 1, 0]
    text = {"xf_proj": g["xf_proj"][sel], "xf_out": g["xf_out"][sel], "length": torch.tensor(LENS)}
    kw = {"xf_proj": text["xf_proj"].cuda(), "xf_out": text["xf_out"].cuda(), "length": text["length"].cuda(), "text": ["a", "b", "a"]}
    x_T = pkg("synth").uniform_pm1((len(LENS), T, g["x_T"].shape[2]), "longctl.x_T", meta["iseed"]) * (3.0 ** 0.5)
    starts, Cn = ML.plan_windows(LENS, H)
    assert Cn == CANVAS
    tab = ML.handshake_tables(starts, LENS, T, H, "linear")
    kw.update({"handshake_" + k: torch.from_numpy(v) for k, v in tab.items()})
    return g, meta, m, noises, kw, text, x_T, starts, tab


def _canvas_control(starts, scale=2e-4, iters=2):
    """A pelvis path and a hand keyframe over the 36-frame canvas, as canvas_control_* kwargs (CPU tensors)."""
    M, ML = pkg("motion_control"), pkg("motion_long")
    tg, w = M.root_path_targets(CANVAS, [[0.0, 0.0], [1.0, 0.5], [1.5, 2.0]], [0, CANVAS // 2, CANVAS - 1])
    kj = torch.zeros(CANVAS, 22, 3)
    kj[CANVAS - 4, 21] = torch.tensor([0.3, 1.2, 1.8])
    ktg, kw_ = M.keyframe_targets(kj, [CANVAS - 4], [21])
    mean, std = _stats(263, 1, 21)
    return {"canvas_control_offsets": torch.tensor([0, CANVAS], dtype=torch.int32),
            "canvas_control_rows": torch.from_numpy(ML.canvas_frame_rows(starts, LENS, T)),
            "canvas_control_joints": tg + ktg, "canvas_control_weights": w + kw_, "canvas_control_mean": mean,
            "canvas_control_std": std, "control_scale": scale, "control_iters": iters}


def _overlaps_equal(x):
    return all(torch.equal(x[i, LENS[i] - H:LENS[i]], x[i + 1, :H]) for i in range(len(LENS) - 1))


def _owner(x, t):
    y = x.clone().reshape(-1, x.shape[-1])
    off, rows = t["offsets"], t["owner_rows"]
    for c in range(len(off) - 1):
        for e in range(off[c] + 1, off[c + 1]):
            y[rows[e]] = y[rows[off[c]]]
    return y.view_as(x)


def _blend_np(eps, t):
    y = eps.clone().reshape(-1, eps.shape[-1])
    off, rows, w = t["offsets"], t["rows"], t["weights"].astype(np.float64)
    for c in range(len(off) - 1):
        es = range(off[c], off[c + 1])
        v = sum(w[e] * y[rows[e]] for e in es)
        for e in es:
            y[rows[e]] = v
    return y.view_as(eps)


def _guide_ref(ctl, tab, mask=None):
    """x0 (B, T, F) f64 -> the canvas gathered from its owner rows, ``iters`` fp64 autograd steps down the canvas loss, the
    result scattered to the owner rows and copied into every overlap."""
    fr = ctl["canvas_control_rows"].long()

    def guide(x0):
        flat = x0.clone().reshape(-1, x0.shape[-1])
        one_minus_m = 1.0 if mask is None else 1.0 - mask.double().reshape(-1, x0.shape[-1])[fr]
        c = flat[fr]
        for _ in range(ctl["control_iters"]):
            _, gr = ref_loss_grad(c[None], [CANVAS], ctl["canvas_control_mean"][0], ctl["canvas_control_std"][0],
                                  ctl["canvas_control_joints"][None], ctl["canvas_control_weights"][None])
            c = c - ctl["control_scale"] * one_minus_m * gr[0]
        flat[fr] = c
        return _owner(flat.view_as(x0), tab)

    return guide


def _cuda(kw):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in kw.items()}


def _run(d, mode, m, kw, scale, eta, use_graph, x_T, ns, streams=0, seed=None):
    """The runner's loop, clipped; returns (final x, [x after step i], [x0 after step i])."""
    xs, x0s = [], []
    r = d._runner(m, tuple(x_T.shape), kw, "cuda", mode, scale if mode.startswith("cfg") else 0.0, eta, True, use_graph, streams)
    out = r.run(x_T.cuda(), ns, False, lambda i, t, x: (xs.append(x.clone().cpu()), x0s.append(r.x0.clone().cpu())), seed=seed)
    return out.cpu(), xs, x0s


@pytest.mark.parametrize("schedule", ["plain25", "ddim10"])
@pytest.mark.parametrize("mode,eta", SOLVERS)
def test_controlled_long_loops_match_the_restated_loop(mode, eta, schedule):
    g, meta, m, noises, kw, text, x_T, starts, tab = _long_setup()
    d = _diffusion(schedule)
    N, scale = d.num_timesteps, meta["cfg_scale"]
    ctl = _canvas_control(starts)
    ns = noises(f"longctl.{mode}.{eta}", N)
    ckw = dict(kw, **_cuda(ctl))
    finals = []
    for use_graph in (True, False):
        out, got, got0 = _run(d, mode, m, ckw, scale, eta, use_graph, x_T, ns)
        assert len(got) == N and torch.equal(out, got[-1]) and torch.isfinite(out).all()
        for i in range(N):
            assert _overlaps_equal(got[i]) and _overlaps_equal(got0[i]), (use_graph, i)
        finals.append(out)
        if use_graph:
            want = S.loop_ref(d, mode, scale, S.device_eps(m, text["length"]), prompts=[(text["xf_proj"], text["xf_out"])],
                              uncond=m.uncond_embedding(len(LENS), "cuda"), inputs=[_owner(x_T, tab)] + got[:-1], eta=eta,
                              step_noise=ns, clip=True, eps_hook=lambda e: _blend_np(e, tab), noise_hook=lambda z: _owner(z, tab),
                              x0_hook=_guide_ref(ctl, tab))
            worst = max(rel_inf(got[i], want[i]) for i in range(N))
            print(f"[long control] {mode} eta {eta} {schedule}: worst step rel_inf vs restated loop {worst:.2e}")
            assert worst <= 1e-4, worst
    assert torch.equal(finals[0], finals[1])
    plain, _, _ = _run(d, mode, m, kw, scale, eta, True, x_T, ns)
    assert not torch.equal(plain, finals[0])


@pytest.mark.parametrize("mode,eta", [("cfg", 0.0), ("cfg_ddim", 0.5), ("cfg_dpmpp", 0.0), ("ddim", 0.0)])
def test_graph_equals_eager_and_two_streams_equal_one_bitwise(mode, eta):
    g, meta, m, noises, kw, text, x_T, starts, tab = _long_setup()
    d = _diffusion([4, 3, 3])
    ckw = dict(kw, **_cuda(_canvas_control(starts, iters=3)))
    outs = {}
    for use_graph, streams in ((True, 1), (False, 1), (True, 2)):
        outs[(use_graph, streams)], _, _ = _run(d, mode, m, ckw, meta["cfg_scale"], eta, use_graph, x_T, None, streams, seed=11)
    assert torch.isfinite(outs[(True, 1)]).all() and _overlaps_equal(outs[(True, 1)])
    assert torch.equal(outs[(True, 1)], outs[(False, 1)])
    assert torch.equal(outs[(True, 1)], outs[(True, 2)])


@pytest.mark.parametrize("mode,eta", [("cfg_ddim", 0.0), ("cfg_dpmpp", 0.0)])
def test_control_with_a_canvas_prefix_edit(mode, eta):
    """A known canvas prefix (into the first overlap) with control on the rest: the prefix is kept bit for bit, the steps
    agree with the restated loop (edit blend, then guidance under 1 - mask)."""
    E, ML = pkg("motion_edit"), pkg("motion_long")
    g, meta, m, noises, kw, text, x_T, starts, tab = _long_setup()
    d = _diffusion("ddim10")
    N, scale = d.num_timesteps, meta["cfg_scale"]
    ctl = _canvas_control(starts)
    known_c = pkg("synth").uniform_pm1((CANVAS, 263), "longctl.known", meta["iseed"])
    known = ML.canvas_to_windows(known_c, starts, LENS, T)
    mask = ML.canvas_to_windows(torch.broadcast_to(E.prefix_mask(CANVAS, 14), (CANVAS, 263)), starts, LENS, T)
    ckw = dict(kw, inpaint_motion=known.cuda(), inpaint_mask=mask.cuda(), **_cuda(ctl))
    ns = noises("longctl.edit", N)
    out, got, got0 = _run(d, mode, m, ckw, scale, eta, True, x_T, ns)
    canvas = ML.windows_to_canvas(out, starts, LENS)
    assert torch.equal(canvas[:14], known_c[:14]) and not torch.equal(canvas[14:], known_c[14:])
    assert all(_overlaps_equal(v) for v in got) and all(_overlaps_equal(v) for v in got0)
    want = S.loop_ref(d, mode, scale, S.device_eps(m, text["length"]), prompts=[(text["xf_proj"], text["xf_out"])],
                      uncond=m.uncond_embedding(len(LENS), "cuda"), inputs=[_owner(x_T, tab)] + got[:-1], eta=eta, step_noise=ns,
                      clip=True, known=known, mask=mask, eps_hook=lambda e: _blend_np(e, tab),
                      noise_hook=lambda z: _owner(z, tab), x0_hook=_guide_ref(ctl, tab, mask))
    worst = max(rel_inf(got[i], want[i]) for i in range(N))
    print(f"[long control + edit] {mode}: worst step rel_inf vs restated loop {worst:.2e}")
    assert worst <= 1e-4, worst


def test_inversion_and_per_window_control_are_refused():
    g, meta, m, noises, kw, text, x_T, starts, tab = _long_setup()
    d = _diffusion("ddim10")
    ckw = dict(kw, **_cuda(_canvas_control(starts)))
    with pytest.raises(ValueError, match="DDIM inversion takes no editing, composed prompts or joint control"):
        d._runner(m, tuple(x_T.shape), ckw, "cuda", "ddim", 0.0, 0.0, False, False, start_step=3, direction=+1)
    per = dict(kw, control_joints=torch.zeros(3, T, 22, 3), control_weights=torch.zeros(3, T, 22, 3),
               control_mean=torch.zeros(3, 263), control_std=torch.ones(3, 263))
    with pytest.raises(NotImplementedError, match="canvas_control"):
        d._runner(m, tuple(x_T.shape), per, "cuda", "ddim", 0.0, 0.0, False, False)


# ---- trainer ------------------------------------------------------------------------------------------------------------
SCRIPTS = [[("walk", 16), ("turn", 12), ("sit", 16)], [("jump", 16)], [("run", 10), ("stop", 12)]]


def _height_control(canv):
    """Every joint's height pulled to 1 on every canvas frame: linear in x0, so stable unclipped (the trainer's loops)."""
    tg = [torch.zeros(c, 22, 3) for c in canv]
    w = [torch.zeros(c, 22, 3) for c in canv]
    for a, b in zip(tg, w):
        a[..., 1], b[..., 1] = 1.0, 1.0
    return tg, w


def test_trainer_generate_long_with_control():
    ML, post = pkg("motion_long"), pkg("postprocess")
    g, meta, m, noises, kw, text, x_T, starts, tab = _long_setup()
    tr = _trainer(m, meta)
    canv = [ML.plan_windows([n for _, n in sc], 4)[1] for sc in SCRIPTS]
    tg, w = _height_control(canv)
    mean, std = np.zeros(263, np.float32), np.ones(263, np.float32)
    std[0] = 0.05
    opts = dict(overlap=4, seed=3, sampler="ddim", sample_steps=10, eta=0.5, control_joints=tg, control_weights=w,
                control_scale=0.05, control_iters=2)
    outs = {bs: [o.cpu() for o in tr.generate_long(SCRIPTS, 263, batch_size=bs, mean=mean, std=std, **opts)] for bs in (3, 6)}
    assert [tuple(o.shape) for o in outs[3]] == [(c, 263) for c in canv]
    for a, b in zip(outs[3], outs[6]):
        assert torch.isfinite(a).all() and rel_inf(a, b) < 1e-5, rel_inf(a, b)
    plain = tr.generate_long(SCRIPTS, 263, batch_size=6, overlap=4, seed=3, sampler="ddim", sample_steps=10, eta=0.5)
    assert all(not torch.equal(p.cpu(), o) for p, o in zip(plain, outs[6]))
    for extra in (dict(sampler="dpmpp2m", eta=0.0), dict(sampler="ddpm", sample_steps=25, eta=0.0)):
        o = tr.generate_long(SCRIPTS, 263, batch_size=6, mean=mean, std=std, **dict(opts, **extra))
        assert all(bool(torch.isfinite(v).all()) for v in o)
    joints = tr.generate_long_joints(SCRIPTS, 263, mean, std, batch_size=6, sigma=1.0, **opts)
    for j, mo, c in zip(joints, outs[6], canv):
        want = post.motion_to_joints(mo.cuda()[None], mean, std, torch.tensor([c]), 22, 1.0)[0]
        assert tuple(j.shape) == (c, 22, 3) and torch.equal(j, want)
    # with a motion to start from as well: it runs, and the control still changes the result
    init = [torch.zeros(c, 263) for c in canv]
    a = tr.generate_long(SCRIPTS, 263, batch_size=6, mean=mean, std=std, init_motion=init, strength=0.5, **opts)
    b = tr.generate_long(SCRIPTS, 263, batch_size=6, overlap=4, seed=3, sampler="ddim", sample_steps=10, eta=0.5,
                         init_motion=init, strength=0.5)
    assert all(bool(torch.isfinite(u).all()) and not torch.equal(u, v) for u, v in zip(a, b))


# the loss ratio measured on an MI355X (9645.0 uncontrolled, 51.3 controlled) and its gate: 3 x the
# measurement, never above 0.5
PATH_RATIO_MEASURED = 0.0053
PATH_RATIO_GATE = min(3 * PATH_RATIO_MEASURED, 0.5)


def test_a_pelvis_path_over_the_canvas_is_followed():
    """loops_tiny, guided DDIM-20, x0 clipped, three windows over a 36-frame canvas, a pelvis path from the origin through
    (2, 0) at frame 18 to (2, 2) at frame 35; mean 0, std 1 except the heading velocity's 0.05.  control_scale by §14's rule
    scale x 0.8 L^2 std^2 < 2 at L = 36: 0.8 x 1296 = 1037, so 0.0015 (x 1037 = 1.56); control_iters 8.  The final canvas's
    loss under its targets against the uncontrolled run of the same seed."""
    M, ML = pkg("motion_control"), pkg("motion_long")
    g, meta, m, noises, kw, text, x_T, starts, tab = _long_setup()
    d = _diffusion("ddim20")
    tg, w = M.root_path_targets(CANVAS, [[0.0, 0.0], [2.0, 0.0], [2.0, 2.0]], [0, CANVAS // 2, CANVAS - 1])
    mean, std = torch.zeros(1, 263), torch.ones(1, 263)
    std[:, 0] = 0.05
    fr = torch.from_numpy(ML.canvas_frame_rows(starts, LENS, T))
    ctl = {"canvas_control_offsets": torch.tensor([0, CANVAS], dtype=torch.int32), "canvas_control_rows": fr,
           "canvas_control_joints": tg, "canvas_control_weights": w, "canvas_control_mean": mean, "canvas_control_std": std,
           "control_scale": 0.0015, "control_iters": 8}
    loss = {}
    for name, k in (("plain", kw), ("ctl", dict(kw, **_cuda(ctl)))):
        out = d.ddim_sample_loop_with_cfg(m, (len(LENS), T, 263), clip_denoised=True, model_kwargs=k, cfg_scale=2.5, seed=7)
        assert _overlaps_equal(out.cpu())
        loss[name] = float(M.canvas_loss_grad(out, [0, CANVAS], fr, mean, std, tg, w)[0][0])
    ratio = loss["ctl"] / loss["plain"]
    print(f"[behaviour] canvas loss uncontrolled {loss['plain']:.4f} controlled {loss['ctl']:.4f} ratio {ratio:.4f}")
    assert ratio <= PATH_RATIO_GATE, ratio


def test_configs1_widths_bf16_two_724_frame_canvases():
    """configs[1] widths in bf16: two motions of four 196-frame windows at h = 20 (724-frame canvases), every joint's height
    pulled to 1 on every frame, 3 guided DDIM steps: finite, the overlaps equal, the control changes the result."""
    ML, T_, synth = pkg("motion_long"), pkg("transformer"), pkg("synth")
    m = T_.MotionTransformer(263, num_frames=196, latent_dim=512, ff_size=1024, num_layers=4, num_heads=4,
                             text_latent_dim=256, moe_num_experts=8, model_size="small", precision=1)
    m.load_state_dict(synth.synth_state_dict(m._layout, 0), strict=True)
    m.set_ephemerals(synth.synth_ephemerals(512, 256, 4, 7)), m.set_projections(synth.synth_projections(128, 4, 7))
    xo_u = synth.uniform_pm1((1, 28, 256), "in.uncond", 0) * (3.0 ** 0.5)
    m = m.cuda().eval()
    m.set_uncond_embedding(xo_u.mean(1).cuda(), xo_u.cuda())
    xo = torch.stack([synth.uniform_pm1((28, 256), f"cap.{i}", 0) * (3.0 ** 0.5) for i in range(8)])
    Tr = pkg("trainer")
    tr = Tr.DDPMTrainer(types.SimpleNamespace(device=torch.device("cuda"), diffusion_steps=1000, is_train=False, cfg_scale=7.5), m)
    plans = ML.script_plans([[(f"c{i}", 196)] * 4 for i in range(2)], 20, 196)
    assert [p[3] for p in plans] == [724, 724]
    tg, w = _height_control([724, 724])
    mean, std = np.zeros(263, np.float32), np.ones(263, np.float32)
    std[0] = 0.05
    control = ML.canvas_control(plans, 263, tg, w, 0.05, 2, mean, std, "cuda")
    kw = {"xf_proj": xo.mean(1).cuda(), "xf_out": xo.cuda(), "length": torch.full((8,), 196).cuda(),
          **ML.batch_tables(plans, [0, 1], 196, 20)}
    d = tr.sampling_diffusion("ddim", 3)
    outs = {}
    for name, k in (("plain", kw), ("ctl", dict(kw, **control([0, 1], 196)))):
        outs[name] = d.ddim_sample_loop_with_cfg(m, (8, 196, 263), clip_denoised=False, model_kwargs=k, cfg_scale=7.5, seed=5).cpu()
    out = outs["ctl"]
    assert torch.isfinite(out).all() and not torch.equal(out, outs["plain"])
    for i in (0, 1, 2, 4, 5, 6):
        assert torch.equal(out[i, 176:], out[i + 1, :20]), i

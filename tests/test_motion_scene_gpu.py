"""GPU: scene constraints: joints kept out of obstacles and above the floor by the guidance of §14 / §23.

* mdm_joint_scene_loss_grad against the fp64 autograd restatement of tests/scene_ref.py: (B, T) = (1, 2) and (3, 40) at F = 263
  and 251 with one primitive of each kind plus a keep-in box per sample, (2, 196) at F = 263 with 16 primitives (the LDS
  limit), ragged lengths with 0 and 1, scene only / with fractional target weights / joint weights with zeros / non-zero
  radii; the primitives are placed from the reference's fp64 positions and shifted clear of their jump sets, and the test
  asserts that placement (every penalised joint >= 1e-3 m from a jump set, every primitive penalising >= 5 % of (t, j) in a
  sample) before it looks at the kernel; gates are §14's (loss rel <= 1e-5, gradient rel_inf <= 1e-4, exact zeros);
* bitwise: K = 0 is mdm_joint_loss_grad, a scene no joint touches leaves x and x0 (-0.0 included), masked entries keep their
  bits; the guidance kernel's single step, its update of x and k iterations = k chained steps; the argument errors;
* the canvas kernel: two motions of 300 and 700 frames through shuffled rows against the restatement at §23's gates, and a
  40-frame canvas against the window kernel;
* loops: cfg_dpmpp and ddim eta = 0.5 with a scene and a root path against the loop restated in tests/sampler_ref.py with
  the autograd guidance, teacher-forced, <= 1e-4 per step, one with an edit mask; graph == eager bitwise; the trainer's batch
  split; a long motion of two windows at overlap 20 with a scene against the restated canvas loop;
* behaviour: a pillar on a pelvis path and the floor: the scene cuts L_scene of the final sample.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import build_module, load_golden, pkg, rel_inf
from test_motion_control_host import ref_positions

import sampler_ref as S
import scene_ref as R
from sampler_ref import caption_trainer as _trainer, loops_setup as _setup, make_diffusion as _diffusion, vp as _vp
from test_motion_control_gpu import _stats, _weights

pytestmark = pytest.mark.gpu

VARIANTS = ("scene", "targets", "joint_weights", "radii")


def _joint_params(variant, B, J, seed):
    g = torch.Generator().manual_seed(seed)
    jp = torch.zeros(B, J, 2)
    jp[..., 1] = 1.0
    if variant == "joint_weights":
        jp[..., 1] = torch.rand(B, J, generator=g) * 2
        jp[..., 1][torch.rand(B, J, generator=g) < 0.15] = 0.0
    if variant == "radii":
        jp[..., 0] = torch.rand(B, J, generator=g) * 0.15
    return jp


@functools.lru_cache(maxsize=None)
def _case(B, T, F, K, variant):
    """x0, mean, std and lengths as test_loss_grad_matches_fp64_autograd draws them; a scene per sample placed from the
    reference's positions; the reference's loss and gradient.  Shared by the tests, left unchanged."""
    J = (F + 1) // 12
    gen = torch.Generator().manual_seed(B * 1000 + T + F)
    x0 = torch.randn(B, T, F, generator=gen) * 0.7
    mean, std = _stats(F, B, B + T)
    tg = torch.randn(B, T, J, 3, generator=gen) * 2.0
    lens = torch.randint(1, T + 1, (B,), generator=gen)
    lens[0] = T
    if B > 1:
        lens[1] = 0
    if B > 2:
        lens[2] = 1
    jp = _joint_params(variant, B, J, T + F)
    P = [ref_positions(x0[b, :int(n)], mean[b], std[b]).detach() if int(n) else torch.zeros(0, J, 3, dtype=torch.float64)
         for b, n in enumerate(lens)]
    scene = torch.stack([R.place_scene(P[b], jp[b], K, seed=b) for b in range(B)]).float()
    stats = [R.scene_stats(P[b], scene[b], jp[b]) for b in range(B)]
    w = _weights("frac", B, T, J, T + F) if variant == "targets" else None
    ref = R.ref_scene_loss_grad(x0, lens, mean, std, scene, jp, tg if w is not None else None, w)
    return dict(x0=x0, mean=mean, std=std, lens=lens, jp=jp, scene=scene, stats=stats, tg=tg if w is not None else None, w=w,
                ref=ref, P=P)


def _scene_lg(x0, lens, mean, std, scene, jp, tg=None, w=None):
    """mdm_joint_scene_loss_grad on packed records (B, K, 12) and joint parameters (B, J, 2)."""
    L = pkg("_lib")
    B, T, F = x0.shape
    dev = [None if v is None else v.cuda().float().contiguous() for v in (x0, mean, std, tg, w, scene, jp)]
    ln = lens.cuda().to(torch.int32)
    loss, grad = torch.empty(B, device="cuda"), torch.empty(B, T, F, device="cuda")
    K = scene.shape[1]
    L.check(L.lib().mdm_joint_scene_loss_grad(_vp(dev[0]), _vp(ln), _vp(dev[1]), _vp(dev[2]), _vp(dev[3]), _vp(dev[4]),
                                              _vp(dev[5] if K else None), C.c_int32(K), _vp(dev[6]), C.c_int32(B), C.c_int32(T),
                                              C.c_int32(F), _vp(loss), _vp(grad), C.c_void_p(L.stream_ptr())))
    return loss.cpu(), grad.cpu()


# ---- mdm_joint_scene_loss_grad ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("B,T,F,K", [(1, 2, 263, 5), (1, 2, 251, 5), (3, 40, 263, 5), (3, 40, 251, 5), (2, 196, 263, 16)])
def test_scene_loss_grad_matches_fp64_autograd(B, T, F, K, variant):
    c = _case(B, T, F, K, variant)
    D = 3 * ((F + 1) // 12) + 1
    # the placement, on the reference alone
    jump = torch.stack([s[0] for s in c["stats"]])
    share = torch.stack([s[1] for s in c["stats"]])
    print(f"[scene B={B} T={T} F={F} K={K} {variant}] least jump distance {float(jump.min()):.2e} m, share of (t, j) penalised "
          f"per primitive (best sample) {[round(v, 3) for v in share.max(0).values.tolist()]}")
    assert float(jump.min()) >= R.JUMP_CLEAR, jump
    assert bool((share.max(0).values >= 0.05).all()), share
    loss, grad = _scene_lg(c["x0"], c["lens"], c["mean"], c["std"], c["scene"], c["jp"], c["tg"], c["w"])
    rl, rg = c["ref"]
    worst_l = worst_g = 0.0
    for b in range(B):
        n = int(c["lens"][b])
        assert torch.equal(grad[b, :, D:], torch.zeros(T, F - D)), b
        assert torch.equal(grad[b, n:], torch.zeros(T - n, F)), b
        if n == 0:
            assert float(loss[b]) == 0.0
            continue
        assert float(rl[b]) > 0
        el = abs(float(loss[b]) - float(rl[b])) / float(rl[b])
        eg = rel_inf(grad[b], rg[b])
        worst_l, worst_g = max(worst_l, el), max(worst_g, eg)
        assert el <= 1e-5, (b, el)
        assert eg <= 1e-4, (b, n, eg)
    print(f"[scene B={B} T={T} F={F} K={K} {variant}] worst loss rel {worst_l:.2e}, worst gradient rel_inf {worst_g:.2e}")


def test_python_entry_equals_the_packed_call():
    """motion_scene.scene_loss_grad on lists of primitives: one shared list and one list per sample."""
    MS = pkg("motion_scene")
    c = _case(3, 40, 263, 5, "scene")
    prims = [MS.sphere((0.3, 0.8, 0.2), 0.7, margin=0.05), MS.capsule((1, -1, 0), (1, 2, 0), 0.3, weight=2.0),
             MS.box((0, 0.5, 1), (0.5, 0.4, 0.6), 0.7), MS.floor(0.1), MS.box((0, 1, 0), (2, 2, 2), -0.3, inside=True)]
    rec = MS.pack_scene(prims)
    jp = MS.joint_params(22, [0.05] * 22, None)
    loss, grad = MS.scene_loss_grad(c["x0"].cuda(), c["lens"], c["mean"], c["std"], prims, joint_radius=[0.05] * 22)
    l2, g2 = _scene_lg(c["x0"], c["lens"], c["mean"], c["std"], rec[None].expand(3, -1, -1), jp[None].expand(3, -1, -1))
    assert torch.equal(loss.cpu(), l2) and torch.equal(grad.cpu(), g2) and float(l2[0]) > 0
    per = [prims, prims[:2], []]
    loss, grad = MS.scene_loss_grad(c["x0"].cuda(), c["lens"], c["mean"], c["std"], per, joint_radius=[0.05] * 22)
    assert torch.equal(loss.cpu()[0], l2[0]) and torch.equal(grad.cpu()[0], g2[0])
    rl, rg = R.ref_scene_loss_grad(c["x0"], c["lens"], c["mean"], c["std"], MS.batch_scene(per, 3), jp[None].expand(3, -1, -1))
    assert abs(float(loss[0]) - float(rl[0])) <= 1e-5 * float(rl[0]) and float(loss[1]) == 0.0


# ---- bitwise ------------------------------------------------------------------------------------------------------------
def test_no_primitives_is_the_joint_loss_grad_bitwise():
    M = pkg("motion_control")
    c = _case(3, 40, 263, 5, "targets")
    none = torch.zeros(3, 0, 12)
    loss, grad = _scene_lg(c["x0"], c["lens"], c["mean"], c["std"], none, c["jp"], c["tg"], c["w"])
    l0, g0 = M.joint_loss_grad(c["x0"].cuda(), c["lens"], c["mean"], c["std"], c["tg"], c["w"])
    assert torch.equal(loss.view(torch.int32), l0.cpu().view(torch.int32))
    assert torch.equal(grad.view(torch.int32), g0.cpu().view(torch.int32))
    # padding records only, through the scene instantiation: the same values up to fp32 rounding (another instantiation may
    # contract its products differently)
    pad = torch.zeros(3, 4, 12)
    loss, grad = _scene_lg(c["x0"], c["lens"], c["mean"], c["std"], pad, c["jp"], c["tg"], c["w"])
    assert rel_inf(loss, l0.cpu()) <= 1e-6 and rel_inf(grad, g0.cpu()) <= 1e-6
    # neither a scene nor targets: zero
    loss, grad = _scene_lg(c["x0"], c["lens"], c["mean"], c["std"], none, c["jp"])
    assert not loss.any() and not grad.any()


def _guide(x, x0, mask, lens, mean, std, tg, w, scene, jp, scale, iters, coef, steps, t, shape=None, K=None):
    L = pkg("_lib")
    B, T, F = x0.shape if shape is None else shape
    K = (5 if scene is None else scene.shape[1]) if K is None else K
    return L.lib().mdm_joint_scene_guidance(_vp(x), _vp(x0), _vp(mask), _vp(lens), _vp(mean), _vp(std), _vp(tg), _vp(w), _vp(scene),
                                            C.c_int32(K), _vp(jp), C.c_int32(B), C.c_int32(T), C.c_int32(F), C.c_float(scale),
                                            C.c_int32(iters), _vp(coef), C.c_int32(steps), C.c_void_p(0), C.c_int32(t),
                                            C.c_void_p(L.stream_ptr()))


def _kernel_case(variant="targets"):
    c = _case(3, 40, 263, 5, variant)
    gen = torch.Generator().manual_seed(3)
    cu = lambda v: None if v is None else v.cuda().float().contiguous()  # noqa: E731
    return dict(x=torch.randn(3, 40, 263, generator=gen).cuda(), x0=cu(c["x0"]), mean=cu(c["mean"]), std=cu(c["std"]),
                tg=cu(c["tg"]), w=cu(c["w"]), scene=cu(c["scene"]), jp=cu(c["jp"]), lens=c["lens"].cuda().to(torch.int32))


def test_guidance_kernel_steps_and_update():
    L = pkg("_lib")
    d = _diffusion("ddim10")
    N = d.num_timesteps
    k = _kernel_case()
    x, x0, lens = k["x"], k["x0"], k["lens"]
    args = (lens, k["mean"], k["std"], k["tg"], k["w"], k["scene"], k["jp"])
    D = 67

    def grad_of(y):
        return _scene_lg(y, lens.cpu(), k["mean"], k["std"], k["scene"], k["jp"], k["tg"], k["w"])[1].cuda()

    scale = 0.01
    for kind in ("ddim", "dpmpp", "ddpm"):
        coef = d._device_coef(kind, 0.0, 2, "cuda")
        for t in (N - 1, N // 2, 0):
            c0 = float(coef[t, 1])
            xo, x0o = x.clone(), x0.clone()
            L.check(_guide(xo, x0o, None, *args, scale, 1, coef, N, t))
            # one fp32 step each way, a few ulp of the largest value involved: this case's gradients reach 1e4, so a step of
            # 0.01 moves entries by up to 1e2, far above |x0| (the §14 test's bound is on |x0| alone)
            want = x0 - scale * grad_of(x0)
            assert float((x0o - want).abs().max()) <= 1e-6 * float(torch.maximum(x0.abs(), want.abs()).max()), (kind, t)
            delta = x0o - x0
            big = max(1.0, float(x.abs().max()), abs(c0) * float(delta.abs().max()))
            assert float((xo - x - c0 * delta).abs().max()) <= 1e-6 * big, (kind, t)
            assert torch.equal(x0o[:, :, D:], x0[:, :, D:]) and torch.equal(xo[:, :, D:], x[:, :, D:])
            for b in range(3):  # frames past the length are not touched
                n = int(lens[b])
                assert torch.equal(x0o[b, n:], x0[b, n:]) and torch.equal(xo[b, n:], x[b, n:])
            assert not torch.equal(x0o, x0)
    # k iterations = k chained loss-grad steps, at a step size the loss's curvature keeps stable (§14's rule, scale x
    # curvature < 2: fractional weights on 22 joints over 40 frames, std up to 1.5, give about 0.8 x 40^2 x 1.5^2 x 11 = 3e4 on
    # the root path, so 1e-5; at 1e-4 two runs part by more than their rounding within 5 iterations)
    coef = d._device_coef("ddim", 0.0, 2, "cuda")
    scale = 1e-5
    for it in (2, 5):
        xo, x0o = x.clone(), x0.clone()
        L.check(_guide(xo, x0o, None, *args, scale, it, coef, N, 3))
        y = x0.clone()
        for _ in range(it):
            y = y - scale * grad_of(y)
        e = float((x0o - y).abs().max()) / float(x0.abs().max())
        print(f"[scene guidance] {it} iterations vs chained loss-grad steps: {e:.2e}")
        assert e <= 1e-5, (it, e)
    # a scene without targets moves x0 as well
    xo, x0o = x.clone(), x0.clone()
    L.check(_guide(xo, x0o, None, lens, k["mean"], k["std"], None, None, k["scene"], k["jp"], 0.01, 1, coef, N, 3))
    g = _scene_lg(x0, lens.cpu(), k["mean"], k["std"], k["scene"], k["jp"])[1].cuda()
    want = x0 - 0.01 * g
    assert float((x0o - want).abs().max()) <= 1e-6 * float(torch.maximum(x0.abs(), want.abs()).max())
    assert not torch.equal(x0o, x0)


def test_untouched_scene_and_masked_entries_are_bitwise_unchanged():
    L, MS = pkg("_lib"), pkg("motion_scene")
    d = _diffusion("ddim10")
    N = d.num_timesteps
    coef = d._device_coef("dpmpp", 0.0, 2, "cuda")
    k = _kernel_case("scene")
    x, x0, lens = k["x"].clone(), k["x0"].clone(), k["lens"]
    x0[0, :5, :10] = -0.0
    x[0, :5, :10] = -0.0
    # far from every joint: a sphere and a pillar 1 km away, a floor 1 km below, a keep-in box of 1 km half extents
    far = MS.pack_scene([MS.sphere((1000, 0, 0), 1.0, margin=0.5), MS.capsule((0, 0, 1000), (0, 5, 1000), 0.5), MS.floor(-1000.0),
                         MS.box((0, 0, 0), (1000, 1000, 1000), 0.3, inside=True)])[None].expand(3, -1, -1).contiguous().cuda()
    xo, x0o = x.clone(), x0.clone()
    L.check(_guide(xo, x0o, None, lens, k["mean"], k["std"], None, None, far, k["jp"], 0.05, 3, coef, N, 4))
    assert torch.equal(xo.view(torch.int32), x.view(torch.int32)) and torch.equal(x0o.view(torch.int32), x0.view(torch.int32))
    gen = torch.Generator().manual_seed(8)
    mask = (torch.rand(x0.shape, generator=gen) < 0.5).float().cuda()
    xo, x0o = x.clone(), x0.clone()
    L.check(_guide(xo, x0o, mask, lens, k["mean"], k["std"], None, None, k["scene"], k["jp"], 0.05, 3, coef, N, 4))
    keep = mask == 1
    assert torch.equal(x0o[keep].view(torch.int32), x0[keep].view(torch.int32))
    assert torch.equal(xo[keep].view(torch.int32), x[keep].view(torch.int32))
    assert not torch.equal(x0o[~keep], x0[~keep])


def test_argument_errors():
    L = pkg("_lib")
    lib = L.lib()
    d = _diffusion("ddim10")
    N = d.num_timesteps
    coef = d._device_coef("ddim", 0.0, 2, "cuda")
    k = _kernel_case()
    a = [k["x"].clone(), k["x0"].clone(), None, k["lens"], k["mean"], k["std"], k["tg"], k["w"], k["scene"], k["jp"], 0.001, 1,
         coef, N, 0, (3, 40, 263)]
    assert _guide(*a) == 0
    for i in (0, 1, 3, 4, 5, 6, 7, 9, 12):  # a null pointer; targets without weights and the reverse
        bad = list(a)
        bad[i] = None
        assert _guide(*bad) == 1, i
    assert _guide(*a, K=5) == 0 and _guide(*a, K=17) == 1 and _guide(*a, K=-1) == 1
    bad = list(a)
    bad[8] = None
    assert _guide(*bad, K=5) == 1  # a null scene with K > 0
    for i, v in ((10, float("nan")), (10, float("inf")), (11, 0), (11, L.CONTROL_MAX_ITERS + 1), (13, 0), (14, N), (14, -1)):
        bad = list(a)
        bad[i] = v
        assert _guide(*bad) == 1, (i, v)
    for shape in ((3, 40, 262), (3, 0, 263), (-1, 40, 263), (3, 205, 263)):
        assert _guide(*a[:-1], shape) == 1, shape
    assert lib.mdm_joint_scene_max_frames(263, 16) == 202 and lib.mdm_joint_scene_max_frames(251, 16) == 208
    big = torch.zeros(1, 203, 263, device="cuda")
    sc16 = torch.zeros(1, 16, 12, device="cuda")
    s = C.c_void_p(L.stream_ptr())
    loss = torch.empty(1, device="cuda")

    def lg(T_, K_):
        return lib.mdm_joint_scene_loss_grad(_vp(big), _vp(k["lens"]), _vp(k["mean"]), _vp(k["std"]), None, None, _vp(sc16),
                                             C.c_int32(K_), _vp(k["jp"]), C.c_int32(1), C.c_int32(T_), C.c_int32(263), _vp(loss),
                                             _vp(big), s)

    assert lg(203, 16) == 1 and lg(202, 16) == 0 and lg(203, 8) == 0 and lg(202, 17) == 1
    torch.cuda.synchronize()


# ---- the canvas kernel --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _canvas_case(canvases, F, with_targets):
    from test_long_control_gpu import _layout, _stats as _cstats, _weights as _cweights
    J, Tw = (F + 1) // 12, 200
    gen = torch.Generator().manual_seed(sum(canvases) * 7 + F)
    B, off, fr = _layout(canvases, Tw, sum(canvases) + F)
    x = torch.randn(B, Tw, F, generator=gen) * 0.7
    mean, std = _cstats(F, len(canvases), F + len(canvases))
    total = int(off[-1])
    tg = torch.randn(total, J, 3, generator=gen) * 2.0
    w = torch.cat([_cweights("frac", n, J, n + F) for n in canvases])
    jp = _joint_params("radii", len(canvases), J, total)
    flat = x.reshape(-1, F)
    scene, stats, loss, grad = [], [], [], torch.zeros(total, F, dtype=torch.float64)
    for m in range(len(canvases)):
        a, b = int(off[m]), int(off[m + 1])
        rows = flat[fr[a:b]]
        P = ref_positions(rows, mean[m], std[m]).detach()
        scene.append(R.place_scene(P, jp[m], 5, seed=m).float())
        stats.append(R.scene_stats(P, scene[-1], jp[m]))
        l, g = R.ref_scene_loss_grad(rows[None], [b - a], mean[m], std[m], scene[-1][None], jp[m][None],
                                     tg[a:b][None] if with_targets else None, w[a:b][None] if with_targets else None)
        loss.append(l[0])
        grad[a:b] = g[0]
    return dict(x=x, off=off, fr=fr, mean=mean, std=std, tg=tg if with_targets else None, w=w if with_targets else None, jp=jp,
                scene=torch.stack(scene), stats=stats, ref=(torch.stack(loss), grad))


def _canvas_lg(c):
    """mdm_canvas_scene_loss_grad on packed records (M, K, 12) and joint parameters (M, J, 2)."""
    L = pkg("_lib")
    F = c["x"].shape[-1]
    M, total = c["off"].numel() - 1, c["fr"].numel()
    f = lambda v: None if v is None else v.cuda().float().contiguous()  # noqa: E731
    x, mean, std, tg, w, scene, jp = (f(c[k]) for k in ("x", "mean", "std", "tg", "w", "scene", "jp"))
    off, fr = c["off"].cuda().to(torch.int32), c["fr"].cuda().to(torch.int32)
    loss, grad = torch.zeros(M, device="cuda"), torch.zeros(total, F, device="cuda")
    ws = torch.empty(int(L.lib().mdm_canvas_control_workspace_floats(total, F)), device="cuda")
    L.check(L.lib().mdm_canvas_scene_loss_grad(_vp(x), _vp(off), _vp(fr), _vp(mean), _vp(std), _vp(tg), _vp(w), _vp(scene),
                                               C.c_int32(scene.shape[1]), _vp(jp), C.c_int32(M), C.c_int32(F), _vp(loss), _vp(grad),
                                               _vp(ws), C.c_void_p(L.stream_ptr())))
    return loss.cpu(), grad.cpu()


@pytest.mark.parametrize("with_targets", [False, True])
def test_canvas_scene_loss_grad_matches_fp64_autograd(with_targets):
    canvases, F = (300, 700), 263
    c = _canvas_case(canvases, F, with_targets)
    jump = torch.stack([s[0] for s in c["stats"]])
    share = torch.stack([s[1] for s in c["stats"]])
    print(f"[canvas scene] least jump distance {float(jump.min()):.2e} m, share penalised {share.max(0).values.tolist()}")
    assert float(jump.min()) >= R.JUMP_CLEAR and bool((share.max(0).values >= 0.05).all())
    assert len(set((c["fr"] // 200).tolist())) > 1 and bool((c["fr"][1:] < c["fr"][:-1]).any())  # several rows, not in order
    loss, grad = _canvas_lg(c)
    rl, rg = c["ref"]
    assert torch.equal(grad[:, 67:], torch.zeros(sum(canvases), F - 67))
    for m, n in enumerate(canvases):
        a = int(c["off"][m])
        el = abs(float(loss[m]) - float(rl[m])) / float(rl[m])
        eg = rel_inf(grad[a:a + n], rg[a:a + n])
        print(f"[canvas scene n={n} targets={with_targets}] loss rel {el:.2e} gradient rel_inf {eg:.2e}")
        assert el <= 1e-5, (m, el)
        assert eg <= 1e-4, (m, eg)


def test_canvas_kernel_equals_the_window_kernel_on_a_short_motion():
    """The (3, 40) case's first sample (40 frames) as a one-motion canvas, its rows in order: the two kernels' summation
    orders differ, so they agree to the gates, not bit for bit; and the Python entry on lists of primitives."""
    c = _case(3, 40, 263, 5, "targets")
    one = dict(x=c["x0"][:1], off=torch.tensor([0, 40]), fr=torch.arange(40), mean=c["mean"][:1], std=c["std"][:1],
               tg=c["tg"][0], w=c["w"][0], jp=c["jp"][:1], scene=c["scene"][:1])
    loss, grad = _canvas_lg(one)
    wl, wg = _scene_lg(c["x0"][:1], c["lens"][:1], c["mean"][:1], c["std"][:1], c["scene"][:1], c["jp"][:1], c["tg"][:1], c["w"][:1])
    el, eg = abs(float(loss[0]) - float(wl[0])) / float(wl[0]), rel_inf(grad, wg[0])
    print(f"[canvas vs window] loss rel {el:.2e} gradient rel_inf {eg:.2e}")
    assert el <= 1e-5 and eg <= 1e-4
    MS = pkg("motion_scene")
    prims = [MS.sphere((0.3, 0.8, 0.2), 0.7), MS.floor(0.2)]
    l1, g1 = MS.canvas_scene_loss_grad(c["x0"][:1].cuda(), [0, 40], torch.arange(40), c["mean"][0], c["std"][0], [prims])
    l2, g2 = MS.scene_loss_grad(c["x0"][:1].cuda(), [40], c["mean"][0], c["std"][0], prims)
    assert float(l2[0]) > 0 and abs(float(l1[0]) - float(l2[0])) <= 1e-5 * float(l2[0]) and rel_inf(g1.cpu(), g2[0].cpu()) <= 1e-4


# ---- loops --------------------------------------------------------------------------------------------------------------
def _loop_scene():
    MS = pkg("motion_scene")
    return [MS.sphere((0.6, 0.4, 0.5), 0.8, margin=0.05), MS.capsule((-0.5, -1.0, 0.8), (-0.5, 2.0, 0.8), 0.3, weight=2.0),
            MS.box((0.2, 0.0, -0.9), (0.5, 0.6, 0.4), 0.5), MS.floor(-0.3)]


def _control(B, T, scale=0.001, iters=2):
    """A root path and a scene over the loops_tiny batch, as control_* kwargs (CPU tensors)."""
    M, MS = pkg("motion_control"), pkg("motion_scene")
    tg, w = M.root_path_targets(T, [[0.0, 0.0], [1.0, 0.5], [1.5, 2.0]], [0, T // 2, T - 1])
    mean, std = _stats(263, B, 21)
    jp = MS.joint_params(22, [0.03] * 22, [1.0] * 20 + [0.0, 2.0])
    return {"control_joints": tg.expand(B, -1, -1, -1).clone(), "control_weights": w.expand(B, -1, -1, -1).clone(),
            "control_mean": mean, "control_std": std, "control_scale": scale, "control_iters": iters,
            "control_scene": MS.batch_scene(_loop_scene(), B), "control_joint_params": jp[None].expand(B, -1, -1).clone()}


def _cuda(kw):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in kw.items()}


def _restated(d, mode, m, g, ctl, inputs, scale, eta=0.0, step_noise=None, known=None, mask=None):
    """As test_motion_control_gpu._restated: tests/sampler_ref.py's loop, teacher-forced, with ``iters`` autograd guidance
    steps down L + L_scene hooked in after the edit blend."""
    one_minus_m = 1.0 if mask is None else 1.0 - mask.double()

    def guide(x0):
        for _ in range(ctl["control_iters"]):
            _, gr = R.ref_scene_loss_grad(x0, g["length"], ctl["control_mean"], ctl["control_std"], ctl["control_scene"],
                                          ctl["control_joint_params"], ctl["control_joints"], ctl["control_weights"])
            x0 = x0 - ctl["control_scale"] * one_minus_m * gr
        return x0

    return S.loop_ref(d, mode, scale, S.device_eps(m, g["length"]), prompts=[(g["xf_proj"], g["xf_out"])],
                      uncond=m.uncond_embedding(g["x_T"].shape[0], "cuda"), inputs=inputs, eta=eta, step_noise=step_noise,
                      clip=True, known=known, mask=mask, x0_hook=guide)


def _check_against_restated(got, want, tag):
    worst = 0.0
    for i in range(len(got)):
        e = rel_inf(got[i], want[i])
        worst = max(worst, e)
        assert e <= 1e-4, (tag, i, e)
    print(f"[scene loop {tag}] worst per-step rel_inf {worst:.2e}")


@pytest.mark.parametrize("mode,eta,edit", [("cfg_dpmpp", 0.0, False), ("ddim", 0.5, False), ("cfg_dpmpp", 0.0, True)])
def test_scene_loops_match_the_restated_loop(mode, eta, edit):
    g, meta, m, noises, kw = _setup()
    d = _diffusion("ddim10")
    N, sc = d.num_timesteps, meta["cfg_scale"]
    B, T, F_ = g["x_T"].shape
    ctl = _control(B, T)
    ns = noises(f"scene.{mode}.{eta}", N)
    known = mask = None
    skw = dict(kw, **_cuda(ctl))
    if edit:
        known = pkg("synth").uniform_pm1((B, T, F_), "scene.known", meta["iseed"])
        mask = torch.broadcast_to(pkg("motion_edit").inbetween_mask(T, 3, 4), (B, T, F_))
        skw.update(inpaint_motion=known.cuda(), inpaint_mask=mask.cuda())
    outs = []
    for use_graph in (True, False):
        got = []
        out = S.run_loop(d, mode, m, skw, sc, eta, use_graph, x_T=g["x_T"].cuda(), step_noise=ns, clip=True,
                         cb=lambda i, t, x: got.append(x.clone().cpu())).cpu()
        assert len(got) == N and torch.equal(out, got[-1]) and torch.isfinite(out).all()
        outs.append(out)
        if use_graph:
            want = _restated(d, mode, m, g, ctl, [g["x_T"]] + got[:-1], sc, eta, ns, known, mask)
            _check_against_restated(got, want, f"{mode} eta {eta} edit {edit}")
    assert torch.equal(outs[0], outs[1])  # graph == eager
    if edit:
        assert torch.equal(outs[0][mask == 1], known[mask == 1])
    no_scene = {k: v for k, v in skw.items() if k not in ("control_scene", "control_joint_params")}
    plain = S.run_loop(d, mode, m, no_scene, sc, eta, True, x_T=g["x_T"].cuda(), step_noise=ns, clip=True).cpu()
    assert not torch.equal(plain, outs[0])
    # the scene alone, without targets
    alone = {k: v for k, v in skw.items() if k not in ("control_joints", "control_weights")}
    out = S.run_loop(d, mode, m, alone, sc, eta, True, x_T=g["x_T"].cuda(), step_noise=ns, clip=True).cpu()
    assert torch.isfinite(out).all() and not torch.equal(out, outs[0])


def test_trainer_scene_is_independent_of_the_batch_split():
    """The trainer samples unclipped, so the scene is made of horizontal half-spaces: heights are linear in x0 and a fixed
    step is stable whatever the size of the model's x0 (as test_motion_control_gpu._height_control)."""
    MS = pkg("motion_scene")
    g, meta, m, noises, kw = _setup()
    tr = _trainer(m, meta)
    caps = ["a", "b", "c", "d"]
    mean, std = (v[0].numpy() for v in _stats(263, 1, 21))
    scenes = [[MS.floor(1.0)], [MS.floor(0.5), MS.sphere((500, 0, 0), 1.0)], [MS.floor(1.0), MS.half_space((0, -1, 0), -3.0)],
              [MS.floor(0.0, margin=0.2)]]
    opts = dict(seed=3, sampler="ddim", sample_steps=10, eta=0.5, scene=scenes, scene_joint_radius=[0.05] * 22,
                control_scale=0.05, control_iters=2, mean=mean, std=std)
    same = torch.tensor([16, 16, 16, 16])
    one = torch.stack(tr.generate(caps, same, 263, batch_size=1, **opts)).cpu()
    two = torch.stack(tr.generate(caps, same, 263, batch_size=2, **opts)).cpu()
    assert torch.isfinite(one).all() and rel_inf(one, two) < 1e-5, rel_inf(one, two)
    plain = torch.stack(tr.generate(caps, same, 263, batch_size=2, seed=3, sampler="ddim", sample_steps=10, eta=0.5)).cpu()
    assert all(not torch.equal(plain[i], two[i]) for i in range(4))
    shared = torch.stack(tr.generate(caps, same, 263, batch_size=2, **dict(opts, scene=scenes[0]))).cpu()
    assert rel_inf(shared[0], two[0]) < 1e-5 and not torch.equal(shared[1], two[1])
    lens = torch.tensor([8, 16, 12, 4])
    serial = tr.generate(caps, lens, 263, batch_size=2, **opts)
    bucket = tr.generate_bucketed(caps, lens, 263, batch_size=2, unit_length=4, **opts)
    for i, n in enumerate(lens.tolist()):
        assert rel_inf(bucket[i][:n].cpu(), serial[i][:n].cpu()) < 1e-4, i
    ex = {k: v for k, v in opts.items() if k not in ("mean", "std")}
    joints = tr.generate_joints(caps, lens, 263, mean, std, batch_size=2, sigma=0.0, **ex)
    assert [tuple(j.shape) for j in joints] == [(n, 22, 3) for n in lens.tolist()]
    depth, share = MS.penetration(torch.stack([torch.nn.functional.pad(j, (0, 0, 0, 0, 0, 16 - j.shape[0])) for j in joints]),
                                  lens, scenes, [0.05] * 22)
    assert depth.shape == (4,) and share.shape == (4,) and bool(torch.isfinite(depth).all())
    with pytest.raises(ValueError):
        tr.generate(caps, same, 263, batch_size=2, seed=3, scene=scenes)  # no mean / std


# ---- a long motion ------------------------------------------------------------------------------------------------------
LENS, H, TW, CANVAS = [48, 40], 20, 48, 68


def _long_setup():
    """The loops_tiny widths at num_frames = 48 (seeded weights): two windows of 48 and 40 frames at overlap 20."""
    ML = pkg("motion_long")
    g, meta = load_golden("loops_tiny")
    meta = dict(meta, cfg=dict(meta["cfg"], num_frames=TW))
    m, _ = build_module(meta, precision=3)
    m.set_uncond_embedding(g["xf_proj_uncond"][:1].cuda(), g["xf_out_uncond"][:1].cuda())
    text = {"xf_proj": g["xf_proj"], "xf_out": g["xf_out"], "length": torch.tensor(LENS)}
    x_T = pkg("synth").uniform_pm1((2, TW, 263), "longscene.x_T", meta["iseed"]) * (3.0 ** 0.5)
    plans = ML.script_plans([[("walk", LENS[0]), ("sit", LENS[1])]], H, TW)
    assert plans[0][3] == CANVAS
    return g, meta, m, text, x_T, plans


def test_long_motion_with_a_scene_matches_the_restated_canvas_loop():
    from test_long_control_gpu import _blend_np, _owner, _run
    M, ML, MS = pkg("motion_control"), pkg("motion_long"), pkg("motion_scene")
    g, meta, m, text, x_T, plans = _long_setup()
    d = _diffusion("ddim10")
    N, scale = d.num_timesteps, meta["cfg_scale"]
    tg, w = M.root_path_targets(CANVAS, [[0.0, 0.0], [1.0, 0.5], [1.5, 2.0]], [0, CANVAS // 2, CANVAS - 1])
    mean, std = _stats(263, 1, 21)
    std[:, 0] = 0.05
    control = ML.canvas_control(plans, 263, [tg], [w], 2e-4, 2, mean[0], std[0], "cpu", [_loop_scene()], [0.03] * 22)
    ctl = control([0], TW)
    assert tuple(ctl["canvas_control_scene"].shape) == (1, 4, 12) and tuple(ctl["canvas_control_joint_params"].shape) == (1, 22, 2)
    tab_kw = ML.batch_tables(plans, [0], TW, H, "linear")
    tab = {k[len("handshake_"):]: v.numpy() for k, v in tab_kw.items()}
    kw = {"xf_proj": text["xf_proj"].cuda(), "xf_out": text["xf_out"].cuda(), "length": text["length"].cuda(), **tab_kw}
    fr = ctl["canvas_control_rows"].long()

    def guide_under(mask):
        one_minus_m = 1.0 if mask is None else 1.0 - mask.double().reshape(-1, 263)[fr]

        def guide(x0):
            flat = x0.clone().reshape(-1, 263)
            c = flat[fr]
            for _ in range(2):
                _, gr = R.ref_scene_loss_grad(c[None], [CANVAS], mean[0], std[0], ctl["canvas_control_scene"],
                                              ctl["canvas_control_joint_params"], tg[None], w[None])
                c = c - 2e-4 * one_minus_m * gr[0]
            flat[fr] = c
            return _owner(flat.view_as(x0), tab)

        return guide

    # a known canvas prefix that reaches into the overlap (canvas frames 28 - 47), kept under the guidance
    known_c = pkg("synth").uniform_pm1((CANVAS, 263), "longscene.known", meta["iseed"])
    starts = plans[0][2]
    known = ML.canvas_to_windows(known_c, starts, LENS, TW)
    mask = ML.canvas_to_windows(torch.broadcast_to(pkg("motion_edit").prefix_mask(CANVAS, 34), (CANVAS, 263)), starts, LENS, TW)
    for mode, eta, edit in (("cfg_dpmpp", 0.0, False), ("ddim", 0.5, False), ("cfg_dpmpp", 0.0, True)):
        ns = [pkg("synth").uniform_pm1((2, TW, 263), f"longscene.{mode}.{i}", meta["iseed"]) * (3.0 ** 0.5) for i in range(N)]
        if edit:
            kw = dict(kw, inpaint_motion=known.cuda(), inpaint_mask=mask.cuda())
        guide = guide_under(mask if edit else None)
        out, got, got0 = _run(d, mode, m, dict(kw, **_cuda(ctl)), scale, eta, True, x_T, ns)
        assert torch.isfinite(out).all()
        if edit:
            canvas = ML.windows_to_canvas(out, starts, LENS)
            assert torch.equal(canvas[:34], known_c[:34]) and not torch.equal(canvas[34:], known_c[34:])
        for v in got + got0:
            assert torch.equal(v[0, LENS[0] - H:LENS[0]], v[1, :H])
        want = S.loop_ref(d, mode, scale, S.device_eps(m, text["length"]), prompts=[(text["xf_proj"], text["xf_out"])],
                          uncond=m.uncond_embedding(2, "cuda"), inputs=[_owner(x_T, tab)] + got[:-1], eta=eta, step_noise=ns,
                          clip=True, eps_hook=lambda e: _blend_np(e, tab), noise_hook=lambda z: _owner(z, tab), x0_hook=guide,
                          known=known if edit else None, mask=mask if edit else None)
        worst = max(rel_inf(got[i], want[i]) for i in range(N))
        print(f"[long scene] {mode} eta {eta} edit {edit}: worst step rel_inf vs restated canvas loop {worst:.2e}")
        assert worst <= 1e-4, worst
        eager, _, _ = _run(d, mode, m, dict(kw, **_cuda(ctl)), scale, eta, False, x_T, ns)
        assert torch.equal(eager, out)
        no_scene = {k: v for k, v in ctl.items() if k not in ("canvas_control_scene", "canvas_control_joint_params")}
        plain, _, _ = _run(d, mode, m, dict(kw, **_cuda(no_scene)), scale, eta, True, x_T, ns)
        assert not torch.equal(plain, out)


def test_trainer_generate_long_with_a_scene():
    """generate_long(scene=) on horizontal half-spaces (the trainer samples unclipped): independent of the batch split, with
    and without targets, through the joints front end."""
    MS = pkg("motion_scene")
    g, meta, m, text, x_T, plans = _long_setup()
    tr = _trainer(m, meta)
    scripts = [[("walk", 48), ("sit", 40)], [("jump", 44)], [("run", 44), ("stop", 48)]]
    mean, std = np.zeros(263, np.float32), np.ones(263, np.float32)
    std[0] = 0.05
    scenes = [[MS.floor(1.0)], [MS.floor(0.5), MS.half_space((0, -1, 0), -3.0)], [MS.floor(0.0, margin=0.3)]]
    opts = dict(overlap=20, seed=3, sampler="ddim", sample_steps=10, eta=0.5, scene=scenes, scene_joint_radius=[0.05] * 22,
                control_scale=0.05, control_iters=2)
    outs = {bs: [o.cpu() for o in tr.generate_long(scripts, 263, batch_size=bs, mean=mean, std=std, **opts)] for bs in (2, 5)}
    assert [o.shape[0] for o in outs[2]] == [68, 44, 72]
    for a, b in zip(outs[2], outs[5]):
        assert torch.isfinite(a).all() and rel_inf(a, b) < 1e-5, rel_inf(a, b)
    plain = tr.generate_long(scripts, 263, batch_size=5, overlap=20, seed=3, sampler="ddim", sample_steps=10, eta=0.5)
    assert all(not torch.equal(p.cpu(), o) for p, o in zip(plain, outs[5]))
    joints = tr.generate_long_joints(scripts, 263, mean, std, batch_size=5, sigma=0.0, **opts)
    assert [tuple(j.shape) for j in joints] == [(68, 22, 3), (44, 22, 3), (72, 22, 3)]
    with pytest.raises(ValueError):
        tr.generate_long(scripts, 263, mean=mean, std=std, **dict(opts, scene=scenes[0]))  # one list, not one per motion


# ---- behaviour ----------------------------------------------------------------------------------------------------------
# L_scene of the final sample with scene= over L_scene without, the larger of the two samples, measured on an MI355X
# (DESIGN.md §24), and its gate: 4 x the measurement, never above 0.5
AVOID_RATIO_MEASURED = 5.3e-5
AVOID_RATIO_GATE = 0.5 if AVOID_RATIO_MEASURED is None else min(4 * AVOID_RATIO_MEASURED, 0.5)


def test_an_obstacle_on_the_path_is_avoided():
    """The setting of test_a_root_path_is_followed (loops_tiny, guided DDIM-20, x0 clipped, a straight pelvis path, mean 0, std
    1 except the heading velocity's 0.05, control_scale 0.002, control_iters 8) with a capsule pillar standing on the path and
    the floor: L_scene of the final sample with scene= against the run without it (the path alone).  The primitives' weights
    follow §14's rule scale x curvature < 2: a height is linear in x0, so the floor's curvature is 2 a std^2 and a = 100 gives
    0.002 x 200 = 0.4; the pillar's force reaches the root path, whose curvature is about 0.8 T^2 = 205 per unit weight at
    T = 16, so a = 5 keeps a single joint's 0.002 x 5 x 205 near 2 and the force is bounded by the pillar's radius."""
    M, MS = pkg("motion_control"), pkg("motion_scene")
    g, meta, m, noises, kw = _setup()
    d = _diffusion("ddim20")
    B, T, F_ = g["x_T"].shape
    tg, w = M.root_path_targets(T, [[0.0, 0.0], [2.0, 0.0], [2.0, 2.0]], [0, T // 2, T - 1])
    mean, std = torch.zeros(B, F_), torch.ones(B, F_)
    std[:, 0] = 0.05
    scene = [MS.capsule((1.0, -1.0, 0.0), (1.0, 2.0, 0.0), 0.3, margin=0.05, weight=5.0), MS.floor(0.0, weight=100.0)]
    ctl = {"control_joints": tg.expand(B, -1, -1, -1).clone(), "control_weights": w.expand(B, -1, -1, -1).clone(),
           "control_mean": mean, "control_std": std, "control_scale": 0.002, "control_iters": 8}
    sc = {"control_scene": MS.batch_scene(scene, B), "control_joint_params": MS.joint_params(22)[None].expand(B, -1, -1).clone()}
    outs = {}
    for name, k in (("path", dict(kw, **_cuda(ctl))), ("scene", dict(kw, **_cuda(ctl), **_cuda(sc)))):
        outs[name] = d.ddim_sample_loop_with_cfg(m, (B, T, F_), clip_denoised=True, model_kwargs=k, cfg_scale=2.5, seed=7)
    ls = {k: MS.scene_loss_grad(v, g["length"], mean, std, scene)[0].cpu() for k, v in outs.items()}
    lp = {k: M.joint_loss_grad(v, g["length"], mean, std, ctl["control_joints"], ctl["control_weights"])[0].cpu()
          for k, v in outs.items()}
    ratio = ls["scene"] / ls["path"]
    print(f"[avoid] L_scene without scene= {ls['path'].tolist()} with {ls['scene'].tolist()} ratio {ratio.tolist()}; "
          f"path loss without {lp['path'].tolist()} with {lp['scene'].tolist()}")
    assert bool((ls["path"] > 0).all())
    assert bool((ratio <= AVOID_RATIO_GATE).all()), ratio

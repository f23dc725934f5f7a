"""GPU: joint-position control (x0 moved down the gradient of a joint-position loss on every step of every sampler).

* mdm_joint_loss_grad against the fp64 autograd restatement of tests/test_motion_control_host.py (ragged lengths including
  0, 1 and T, F = 263 and 251, several weight maps, weights past the length), exact zeros where no gradient can arrive,
  and P equal to mdm_motion_postprocess at radius 0 to the last bits (the loss of its own output is at rounding level);
* mdm_joint_guidance: one iteration is x0 - scale * grad and moves x by c0[t] * delta, k iterations are k chained
  loss-grad steps, all-zero weights and masked entries leave x and x0 bit for bit, argument errors;
* every loop against the loop restated in tests/sampler_ref.py (the product's forward, the abar-derived update) with the
  autograd guidance hooked in after the edit blend, teacher-forced on the device's trajectory, also with an edit mask and
  with K = 2 composed prompts; graph == eager and two streams == one bitwise; the trainer's result independent of the batch
  split;
* behaviour: a root path cuts the final sample's loss to <= 0.1x the uncontrolled sample's; the configs[1] shape in bf16.
"""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from conftest import pkg, rel_inf
from test_motion_control_host import ref_loss_grad

import sampler_ref as S
from sampler_ref import caption_trainer as _trainer, loops_setup as _setup, make_diffusion as _diffusion, vp as _vp

pytestmark = pytest.mark.gpu


def _stats(F, B, seed):
    g = torch.Generator().manual_seed(seed)
    mean = torch.randn(B, F, generator=g) * 0.2
    std = torch.rand(B, F, generator=g) + 0.5
    std[:, 0] *= 0.1  # the heading velocity: small per frame, as in HumanML3D
    mean[:, 0] *= 0.1
    return mean, std


def _weights(kind, B, T, J, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.zeros(B, T, J, 3)
    if kind == "root_keys":  # root XZ on a few keyframes
        for f in sorted({0, T // 3, T // 2, T - 1}):
            w[:, f, 0, 0] = w[:, f, 0, 2] = 1.0
    elif kind == "all":
        w[:] = 1.0
    else:  # fractional weights, some zero
        w = torch.rand(B, T, J, 3, generator=g)
        w[w < 0.3] = 0.0
    return w


# ---- mdm_joint_loss_grad ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [263, 251])
@pytest.mark.parametrize("B,T", [(1, 2), (3, 40), (32, 196)])
def test_loss_grad_matches_fp64_autograd(B, T, F):
    M = pkg("motion_control")
    J, D = (F + 1) // 12, 3 * ((F + 1) // 12) + 1
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
    worst = 0.0
    for kind in ("root_keys", "all", "frac"):
        w = _weights(kind, B, T, J, T + F)  # non-zero past each length as well: ignored
        loss, grad = M.joint_loss_grad(x0.cuda(), lens, mean, std, tg, w)
        loss, grad = loss.cpu(), grad.cpu()
        rl, rg = ref_loss_grad(x0, lens, mean, std, tg, w)
        for b in range(B):
            n = int(lens[b])
            assert torch.equal(grad[b, :, D:], torch.zeros(T, F - D)), (kind, b)
            assert torch.equal(grad[b, n:], torch.zeros(T - n, F)), (kind, b)
            if n == 0:
                assert float(loss[b]) == 0.0
                continue
            el = abs(float(loss[b]) - float(rl[b])) / max(float(rl[b]), 1e-30)
            assert el <= 1e-5, (kind, b, el)
            if float(rg[b].abs().max()) > 0:
                eg = rel_inf(grad[b], rg[b])
                worst = max(worst, eg)
                assert eg <= 1e-4, (kind, b, n, eg)
    print(f"[loss_grad B={B} T={T} F={F}] worst gradient rel_inf {worst:.2e}")


def test_positions_equal_the_postprocess_kernel():
    """Targets = mdm_motion_postprocess's output at radius 0: P agrees with it to the last bits (the two kernels' fp32
    products may contract differently), so the loss is at rounding level: RMS(P - G) <= 1e-6 max |G|."""
    M = pkg("motion_control")
    P = pkg("postprocess")
    gen = torch.Generator().manual_seed(5)
    B, T, F = 4, 60, 263
    x0 = torch.randn(B, T, F, generator=gen) * 0.7
    mean, std = _stats(F, 1, 9)
    lens = torch.tensor([60, 33, 1, 59])
    joints = P.motion_to_joints(x0.cuda(), mean[0].numpy(), std[0].numpy(), lens, 22, sigma=0.0)
    loss, grad = M.joint_loss_grad(x0.cuda(), lens, mean[0], std[0], joints, torch.ones(B, T, 22, 3))
    for b in range(B):
        n = int(lens[b])
        rms = (float(loss[b]) / (n * 22 * 3)) ** 0.5
        print(f"[positions] sample {b} (length {n}): loss {float(loss[b]):.3e}, RMS(P - G) {rms:.3e}")
        assert rms <= 1e-6 * float(joints[b, :n].abs().max()), (b, rms)


# ---- mdm_joint_guidance -------------------------------------------------------------------------------------------------
def _guide(x, x0, mask, lens, mean, std, tg, w, scale, iters, coef, steps, t, shape=None):
    L = pkg("_lib")
    B, T, F = x0.shape if shape is None else shape
    return L.lib().mdm_joint_guidance(_vp(x), _vp(x0), _vp(mask), _vp(lens), _vp(mean), _vp(std), _vp(tg), _vp(w),
                                      C.c_int32(B), C.c_int32(T), C.c_int32(F), C.c_float(scale), C.c_int32(iters),
                                      _vp(coef), C.c_int32(steps), C.c_void_p(0), C.c_int32(t), C.c_void_p(L.stream_ptr()))


def _kernel_case(B=3, T=40, F=263, seed=3):
    gen = torch.Generator().manual_seed(seed)
    J = (F + 1) // 12
    x0 = (torch.randn(B, T, F, generator=gen) * 0.7).cuda()
    x = (torch.randn(B, T, F, generator=gen)).cuda()
    mean, std = (v.cuda().contiguous() for v in _stats(F, B, seed))
    tg = (torch.randn(B, T, J, 3, generator=gen) * 2.0).cuda()
    w = _weights("frac", B, T, J, seed).cuda()
    lens = torch.tensor([T, T // 2, 1][:B], dtype=torch.int32).cuda()
    return x, x0, mean, std, tg, w, lens


def test_guidance_kernel_steps_and_update():
    M = pkg("motion_control")
    L = pkg("_lib")
    d = _diffusion("ddim10")
    N = d.num_timesteps
    x, x0, mean, std, tg, w, lens = _kernel_case()
    B, T, F = x0.shape
    D = 67
    scale = 0.01
    for kind in ("ddim", "dpmpp", "ddpm"):
        coef = d._device_coef(kind, 0.0, 2, "cuda")
        for t in (N - 1, N // 2, 0):
            c0 = float(coef[t, 1])
            xo, x0o = x.clone(), x0.clone()
            L.check(_guide(xo, x0o, None, lens, mean, std, tg, w, scale, 1, coef, N, t))
            _, g = M.joint_loss_grad(x0, lens, mean, std, tg, w)
            want = x0 - scale * g
            assert float((x0o - want).abs().max()) <= 1e-6 * float(x0.abs().max()), (kind, t)
            delta = x0o - x0
            assert float((xo - x - c0 * delta).abs().max()) <= 1e-6 * max(1.0, float(x.abs().max())), (kind, t)
            assert torch.equal(x0o[:, :, D:], x0[:, :, D:]) and torch.equal(xo[:, :, D:], x[:, :, D:])
            for b in range(B):  # frames past the length are not touched
                n = int(lens[b])
                assert torch.equal(x0o[b, n:], x0[b, n:]) and torch.equal(xo[b, n:], x[b, n:])
            assert not torch.equal(x0o, x0)
    # k iterations = k chained loss-grad steps, at a step size the loss's curvature keeps stable (dense weights over 40
    # frames: at 1e-3 the heading steps overshoot within 5 iterations, and two runs then part by far more than their rounding)
    coef = d._device_coef("ddim", 0.0, 2, "cuda")
    scale = 1e-4
    for k in (2, 5):
        xo, x0o = x.clone(), x0.clone()
        L.check(_guide(xo, x0o, None, lens, mean, std, tg, w, scale, k, coef, N, 3))
        y = x0.clone()
        for _ in range(k):
            _, g = M.joint_loss_grad(y, lens, mean, std, tg, w)
            y = y - scale * g
        e = float((x0o - y).abs().max()) / float(x0.abs().max())
        print(f"[guidance] {k} iterations vs chained loss-grad steps: {e:.2e}")
        assert e <= 1e-5, (k, e)


def test_guidance_all_zero_weights_and_masked_entries_are_bitwise_unchanged():
    L = pkg("_lib")
    d = _diffusion("ddim10")
    N = d.num_timesteps
    coef = d._device_coef("dpmpp", 0.0, 2, "cuda")
    x, x0, mean, std, tg, w, lens = _kernel_case()
    x0[0, :5, :10] = -0.0
    x[0, :5, :10] = -0.0
    xo, x0o = x.clone(), x0.clone()
    L.check(_guide(xo, x0o, None, lens, mean, std, tg, torch.zeros_like(w), 0.05, 3, coef, N, 4))
    assert torch.equal(xo.view(torch.int32), x.view(torch.int32)) and torch.equal(x0o.view(torch.int32), x0.view(torch.int32))
    gen = torch.Generator().manual_seed(8)
    mask = (torch.rand(x0.shape, generator=gen) < 0.5).float().cuda()
    xo, x0o = x.clone(), x0.clone()
    L.check(_guide(xo, x0o, mask, lens, mean, std, tg, w, 0.05, 3, coef, N, 4))
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
    x, x0, mean, std, tg, w, lens = _kernel_case()
    B, T, F = x0.shape
    a = [x, x0, None, lens, mean, std, tg, w, 0.1, 1, coef, N, 0, (B, T, F)]
    assert _guide(*a) == 0
    for i in (0, 1, 3, 4, 5, 6, 7, 10):
        bad = list(a)
        bad[i] = None
        assert _guide(*bad) == 1, i
    for i, v in ((8, float("nan")), (8, float("inf")), (9, 0), (9, L.CONTROL_MAX_ITERS + 1), (11, 0), (12, N), (12, -1)):
        bad = list(a)
        bad[i] = v
        assert _guide(*bad) == 1, (i, v)
    s = C.c_void_p(L.stream_ptr())
    ptrs = [_vp(v) for v in (x0, lens, mean, std, tg, w)]
    loss, grad = torch.empty(B, device="cuda"), torch.empty_like(x0)

    def lg(p, B_=B, T_=T, F_=F, lo=loss, gr=grad):
        return lib.mdm_joint_loss_grad(*p, C.c_int32(B_), C.c_int32(T_), C.c_int32(F_), _vp(lo), _vp(gr), s)

    assert lg(ptrs) == 0
    for i in range(6):
        bad = list(ptrs)
        bad[i] = C.c_void_p(0)
        assert lg(bad) == 1, i
    assert lg(ptrs, lo=None) == 1 and lg(ptrs, gr=None) == 1
    assert lg(ptrs, F_=262) == 1 and lg(ptrs, T_=0) == 1 and lg(ptrs, B_=-1) == 1
    big = torch.zeros(1, 206, 263, device="cuda")
    assert lib.mdm_joint_loss_grad(_vp(big), *ptrs[1:], C.c_int32(1), C.c_int32(206), C.c_int32(263), _vp(loss),
                                   _vp(big), s) == 1
    assert lib.mdm_joint_control_max_frames(263) == 205 and lib.mdm_joint_control_max_frames(251) == 211
    assert lib.mdm_joint_control_max_frames(262) == 0
    torch.cuda.synchronize()


# ---- loops --------------------------------------------------------------------------------------------------------------
def _control(B, T, F_=263, scale=0.001, iters=2):
    M = pkg("motion_control")
    tg, w = M.root_path_targets(T, [[0.0, 0.0], [1.0, 0.5], [1.5, 2.0]], [0, T // 2, T - 1])
    kj = torch.zeros(T, 22, 3)
    kj[T - 4, 21] = torch.tensor([0.3, 1.2, 1.8])
    ktg, kw_ = M.keyframe_targets(kj, [T - 4], [21])
    tg, w = tg + ktg, w + kw_
    mean, std = _stats(F_, B, 21)
    return {"control_joints": tg.expand(B, -1, -1, -1).clone(), "control_weights": w.expand(B, -1, -1, -1).clone(),
            "control_mean": mean, "control_std": std, "control_scale": scale, "control_iters": iters}


def _cuda(kw):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in kw.items()}


def _restated(d, mode, m, g, ctl, inputs, scale, eta=0.0, step_noise=None, known=None, mask=None, prompts=None, pw=None):
    """x_{t-1} of every step from the device's x_t (teacher forcing) by tests/sampler_ref.py's loop: the product's forward
    (once per prompt and once unconditionally), x0 from abar clamped to [-1, 1], the CFG / composed combination, the edit
    blend, then ``iters`` autograd guidance steps x0 -= scale (1 - m) grad, then the update restated from abar in f64.  The
    loops run clipped: the random-weight model's x0 at the first steps is ~1/sqrt(abar) times too large unclipped, and the
    joint loss's curvature grows with the square of the positions, so no fixed step size would be stable there."""
    one_minus_m = 1.0 if mask is None else 1.0 - mask.double()

    def guide(x0):
        for _ in range(ctl["control_iters"]):
            _, gr = ref_loss_grad(x0, g["length"], ctl["control_mean"], ctl["control_std"], ctl["control_joints"],
                                  ctl["control_weights"])
            x0 = x0 - ctl["control_scale"] * one_minus_m * gr
        return x0

    return S.loop_ref(d, mode, scale, S.device_eps(m, g["length"]), prompts=prompts or [(g["xf_proj"], g["xf_out"])], weights=pw,
                      uncond=m.uncond_embedding(g["x_T"].shape[0], "cuda"), inputs=inputs, eta=eta, step_noise=step_noise,
                      clip=True, known=known, mask=mask, x0_hook=guide)


def _check_against_restated(got, want, tag):
    worst = 0.0
    for i in range(len(got)):
        e = rel_inf(got[i], want[i])
        worst = max(worst, e)
        assert e <= 1e-4, (tag, i, e)
    print(f"[control loop {tag}] worst per-step rel_inf {worst:.2e}")


SOLVERS = [("cfg", 0.0), ("ddpm", 0.0), ("ddim", 0.0), ("ddim", 0.5), ("cfg_ddim", 0.5), ("cfg_dpmpp", 0.0)]


@pytest.mark.parametrize("schedule", ["plain25", "ddim10"])
@pytest.mark.parametrize("mode,eta", SOLVERS)
def test_controlled_loops_match_the_restated_loop(mode, eta, schedule):
    g, meta, m, noises, kw = _setup()
    d = _diffusion(schedule)
    N, sc = d.num_timesteps, meta["cfg_scale"]
    B, T, F_ = g["x_T"].shape
    ctl = _control(B, T)
    ns = noises(f"ctl.{mode}.{eta}", N)
    got = []
    out = S.run_loop(d, mode, m, dict(kw, **_cuda(ctl)), sc, eta, True, x_T=g["x_T"].cuda(), step_noise=ns, clip=True,
                     cb=lambda i, t, x: got.append(x.clone().cpu())).cpu()
    assert len(got) == N and torch.equal(out, got[-1]) and torch.isfinite(out).all()
    want = _restated(d, mode, m, g, ctl, [g["x_T"]] + got[:-1], sc, eta, ns)
    _check_against_restated(got, want, f"{mode} eta {eta} {schedule}")
    plain = S.run_loop(d, mode, m, kw, sc, eta, True, x_T=g["x_T"].cuda(), step_noise=ns, clip=True).cpu()
    assert not torch.equal(plain, out)


@pytest.mark.parametrize("mode,eta", [("cfg_ddim", 0.0), ("cfg_dpmpp", 0.0), ("ddim", 0.5)])
def test_control_with_an_edit_mask(mode, eta):
    E = pkg("motion_edit")
    synth = pkg("synth")
    g, meta, m, noises, kw = _setup()
    d = _diffusion("ddim10")
    N, sc = d.num_timesteps, meta["cfg_scale"]
    B, T, F_ = g["x_T"].shape
    ctl = _control(B, T)
    known = synth.uniform_pm1((B, T, F_), "ctl.known", meta["iseed"])
    mask = torch.broadcast_to(E.inbetween_mask(T, 3, 4), (B, T, F_))
    ns = noises("ctl.edit", N)
    ekw = dict(kw, inpaint_motion=known.cuda(), inpaint_mask=mask.cuda(), **_cuda(ctl))
    got = []
    out = S.run_loop(d, mode, m, ekw, sc, eta, True, x_T=g["x_T"].cuda(), step_noise=ns, clip=True,
                     cb=lambda i, t, x: got.append(x.clone().cpu())).cpu()
    keep = mask == 1
    assert torch.equal(out[keep], known[keep])
    want = _restated(d, mode, m, g, ctl, [g["x_T"]] + got[:-1], sc, eta, ns, known=known, mask=mask)
    _check_against_restated(got, want, f"edit {mode}")


@pytest.mark.parametrize("mode,eta", [("cfg_ddim", 0.5), ("cfg_dpmpp", 0.0), ("cfg", 0.0)])
def test_control_with_two_composed_prompts(mode, eta):
    synth = pkg("synth")
    g, meta, m, noises, kw = _setup()
    d = _diffusion("ddim10" if mode != "cfg" else "plain25")
    N, sc = d.num_timesteps, meta["cfg_scale"]
    B, T, F_ = g["x_T"].shape
    Dt = g["xf_proj"].shape[1]
    ctl = _control(B, T)
    xo2 = synth.uniform_pm1((B, g["xf_out"].shape[1], Dt), "ctl.prompt2", meta["iseed"])
    prompts = [(g["xf_proj"], g["xf_out"]), (xo2.mean(1), xo2)]
    pw = torch.zeros(B, 2, T, F_)
    pw[:, 0, : T // 2] = 1.0
    pw[:, 1, T // 2:] = 1.0
    pw[:, 1, :, :4] += 0.5
    ckw = {"length": kw["length"], "compose_weights": pw.cuda(),
           "compose_xf_proj": torch.stack([p[0] for p in prompts], 1).cuda(),
           "compose_xf_out": torch.stack([p[1] for p in prompts], 1).cuda(), **_cuda(ctl)}
    ns = noises("ctl.compose", N)
    got = []
    S.run_loop(d, mode, m, ckw, sc, eta, True, x_T=g["x_T"].cuda(), step_noise=ns, clip=True,
               cb=lambda i, t, x: got.append(x.clone().cpu()))
    want = _restated(d, mode, m, g, ctl, [g["x_T"]] + got[:-1], sc, eta, ns, prompts=prompts, pw=pw)
    _check_against_restated(got, want, f"compose {mode}")


@pytest.mark.parametrize("mode,eta", [("cfg", 0.0), ("cfg_ddim", 0.5), ("cfg_dpmpp", 0.0), ("ddim", 0.0)])
def test_graph_equals_eager_and_two_streams_equal_one_bitwise(mode, eta):
    g, meta, m, noises, kw = _setup()
    d = _diffusion([4, 3, 3])
    B, T, F_ = g["x_T"].shape
    ckw = dict(kw, **_cuda(_control(B, T, iters=3)))
    outs = {}
    for use_graph, streams in ((True, 1), (False, 1), (True, 2)):
        r = d._runner(m, (B, T, F_), ckw, "cuda", mode, meta["cfg_scale"], eta, True, use_graph, streams)
        outs[(use_graph, streams)] = r.run(g["x_T"].cuda(), None, False, None, seed=11).cpu()
    assert torch.isfinite(outs[(True, 1)]).all()
    assert torch.equal(outs[(True, 1)], outs[(False, 1)])
    assert torch.equal(outs[(True, 1)], outs[(True, 2)])


def test_progressive_loop_and_single_step_carry_the_control():
    g, meta, m, noises, kw = _setup()
    d = _diffusion("ddim10")
    B, T, F_ = g["x_T"].shape
    ckw = dict(kw, **_cuda(_control(B, T)))
    steps = list(d.ddim_sample_loop_progressive(m, (B, T, F_), noise=g["x_T"].cuda(), clip_denoised=True,
                                                model_kwargs=ckw, eta=0.0))
    loop = d.ddim_sample_loop(m, (B, T, F_), noise=g["x_T"].cuda(), clip_denoised=True, model_kwargs=ckw,
                              use_graph=False).cpu()
    assert torch.equal(steps[-1]["sample"].cpu(), loop)
    t = torch.full((B,), d.num_timesteps - 1, dtype=torch.int64, device="cuda")
    one = d.ddim_sample_with_cfg(m, g["x_T"].cuda(), t, clip_denoised=False, model_kwargs=ckw, cfg_scale=2.5)
    plain = d.ddim_sample_with_cfg(m, g["x_T"].cuda(), t, clip_denoised=False, model_kwargs=kw, cfg_scale=2.5)
    assert not torch.equal(one["pred_xstart"], plain["pred_xstart"])
    with pytest.raises(ValueError):
        d.ddim_sample(m, g["x_T"].cuda(), t, clip_denoised=False,
                      model_kwargs=dict(kw, control_joints=ckw["control_joints"]))


# ---- trainer ------------------------------------------------------------------------------------------------------------
def _height_control(B, T):
    """Every joint's height pulled to 1 on every frame: the trainer samples unclipped, and heights are linear in x0 (no
    rotation enters them), so the loss is quadratic and a fixed step is stable whatever the size of the model's x0."""
    tg, w = torch.zeros(B, T, 22, 3), torch.zeros(B, T, 22, 3)
    tg[..., 1], w[..., 1] = 1.0, 1.0
    return tg, w


def test_trainer_control_is_independent_of_the_batch_split():
    g, meta, m, noises, kw = _setup()
    tr = _trainer(m, meta)
    caps = ["a", "b", "c", "d"]
    c = _control(4, 16)
    mean, std = c["control_mean"][0].numpy(), c["control_std"][0].numpy()
    tg, w = _height_control(4, 16)
    opts = dict(seed=3, sampler="ddim", sample_steps=10, eta=0.5, control_joints=tg, control_weights=w, control_scale=0.05,
                control_iters=2, mean=mean, std=std)
    same = torch.tensor([16, 16, 16, 16])
    one = torch.stack(tr.generate(caps, same, 263, batch_size=1, **opts)).cpu()
    two = torch.stack(tr.generate(caps, same, 263, batch_size=2, **opts)).cpu()
    assert torch.isfinite(one).all() and rel_inf(one, two) < 1e-5, rel_inf(one, two)
    plain = torch.stack(tr.generate(caps, same, 263, batch_size=2, seed=3, sampler="ddim", sample_steps=10,
                                    eta=0.5)).cpu()
    assert not torch.equal(plain, two)
    lens = torch.tensor([8, 16, 12, 4])
    for extra in (dict(opts), dict(opts, sampler="dpmpp2m", eta=0.0, control_iters=1)):
        serial = tr.generate(caps, lens, 263, batch_size=2, **extra)
        bucket = tr.generate_bucketed(caps, lens, 263, batch_size=2, unit_length=4, **extra)
        for i, n in enumerate(lens.tolist()):
            e = rel_inf(bucket[i][:n].cpu(), serial[i][:n].cpu())
            assert e < 1e-4, (i, e)
    ex = {k: v for k, v in opts.items() if k not in ("mean", "std")}
    joints = tr.generate_joints(caps, lens, 263, mean, std, batch_size=2, sigma=0.0, **ex)
    assert [tuple(j.shape) for j in joints] == [(n, 22, 3) for n in lens.tolist()]
    with pytest.raises(ValueError):
        tr.generate(caps, same, 263, batch_size=2, seed=3, control_joints=tg)
    with pytest.raises(ValueError):
        tr.generate(caps, same, 263, batch_size=2, seed=3, control_joints=tg, control_weights=w)


# ---- behaviour ----------------------------------------------------------------------------------------------------------
def test_a_root_path_is_followed():
    """Synthetic small model, guided DDIM-20, a root path: the final sample's loss under its targets is <= 0.1x the loss
    of the uncontrolled sample from the same seed.  control_scale = 0.002, control_iters = 8, x0 clipped to [-1, 1] before
    the guidance; mean 0, std 1 except the heading velocity's 0.05."""
    M = pkg("motion_control")
    g, meta, m, noises, kw = _setup()
    d = _diffusion("ddim20")
    B, T, F_ = g["x_T"].shape
    tg, w = M.root_path_targets(T, [[0.0, 0.0], [2.0, 0.0], [2.0, 2.0]], [0, T // 2, T - 1])
    mean, std = torch.zeros(B, F_), torch.ones(B, F_)
    std[:, 0] = 0.05
    ctl = {"control_joints": tg.expand(B, -1, -1, -1).clone(), "control_weights": w.expand(B, -1, -1, -1).clone(),
           "control_mean": mean, "control_std": std, "control_scale": 0.002, "control_iters": 8}
    outs = {}
    for name, k in (("plain", kw), ("ctl", dict(kw, **_cuda(ctl)))):
        outs[name] = d.ddim_sample_loop_with_cfg(m, (B, T, F_), clip_denoised=True, model_kwargs=k, cfg_scale=2.5,
                                                 seed=7)
    lp, _ = M.joint_loss_grad(outs["plain"], g["length"], mean, std, ctl["control_joints"], ctl["control_weights"])
    lc, _ = M.joint_loss_grad(outs["ctl"], g["length"], mean, std, ctl["control_joints"], ctl["control_weights"])
    ratio = (lc / lp).cpu()
    print(f"[behaviour] loss uncontrolled {lp.tolist()} controlled {lc.tolist()} ratio {ratio.tolist()}")
    assert bool((ratio <= 0.1).all()), ratio


def test_configs1_shape_bf16_with_control():
    """configs[1] shape (small, 8 experts, B=32, T=196, guided, 1000-step schedule) in bf16: DPM-Solver++(2M)-20 with a
    every joint's height pulled to 1 (quadratic in x0, stable unclipped) through DDPMTrainer.generate gives finite motions."""
    T_ = pkg("transformer")
    synth = pkg("synth")
    m = T_.MotionTransformer(263, num_frames=196, latent_dim=512, ff_size=1024, num_layers=4, num_heads=4,
                             text_latent_dim=256, moe_num_experts=8, model_size="small", precision=1)
    m.load_state_dict(synth.synth_state_dict(m._layout, 0), strict=True)
    m.set_ephemerals(synth.synth_ephemerals(512, 256, 4, 7)), m.set_projections(synth.synth_projections(128, 4, 7))
    B, T = 32, 196
    _, _, length, xf_proj, xf_out = synth.synth_inputs(B, T, 263, 28, 256, 0, min_len=40)
    length[0] = T
    xo_u = synth.uniform_pm1((1, 28, 256), "in.uncond", 0) * (3.0 ** 0.5)
    m = m.cuda().eval()
    m.set_uncond_embedding(xo_u.mean(1).cuda(), xo_u.cuda())
    m.text_encoder_fn = lambda text, device: (xf_proj[:len(text)].to(device), xf_out[:len(text)].to(device))
    Tr = pkg("trainer")
    tr = Tr.DDPMTrainer(types.SimpleNamespace(device=torch.device("cuda"), diffusion_steps=1000, is_train=False,
                                              cfg_scale=7.5), m)
    caps = [f"caption {i}" for i in range(B)]
    tg, w = _height_control(B, T)
    mean, std = np.zeros(263, np.float32), np.ones(263, np.float32)
    std[0] = 0.05
    out = torch.stack(tr.generate(caps, length, 263, batch_size=B, seed=5, sampler="dpmpp2m", sample_steps=20,
                                  control_joints=tg, control_weights=w, control_scale=0.05, control_iters=2, mean=mean,
                                  std=std)).cpu()
    assert torch.isfinite(out).all()
    plain = torch.stack(tr.generate(caps, length, 263, batch_size=B, seed=5, sampler="dpmpp2m", sample_steps=20)).cpu()
    assert not torch.equal(out, plain)

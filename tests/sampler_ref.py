"""The sampling loops restated in f64 from alphas_cumprod, and the harness the sampler GPU tests share.

One restatement of the DDPM posterior step, the DDIM step, DPM-Solver++(2M) and the upward DDIM-inversion step
(``update_ref``), of the guided / composed / edited x0 (``x0_ref``) and of the loop around them (``loop_ref``).  It reads abar
and the timestep map of the schedule and nothing else of the product: tests/test_sampler_ref_host.py pins it to the reference's
recorded loops and to ``GaussianDiffusion.solver_coefficients`` on the CPU, so a GPU mismatch against it lies on the device
side.  A new sampling feature extends ``loop_ref`` with a hook, not with a copy.

CPU-only, except ``loops_setup`` / ``caption_trainer`` / ``run_loop`` / ``device_eps`` (which drive the product) and
``guided_update`` (a ctypes caller).
"""
import ctypes as C
import os
import sys
import types

import numpy as np
import torch

from conftest import ROOT, build_module, golden_state, load_golden, pkg

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import denoiser_ref as R  # noqa: E402

KIND = {"cfg": "ddpm", "ddpm": "ddpm", "cfg_ddim": "ddim", "ddim": "ddim", "cfg_dpmpp": "dpmpp"}
f32 = lambda v: float(np.float32(v))  # noqa: E731


# ---- schedule and loop plumbing ----------------------------------------------------------------------------------------
def diffusion_kwargs(steps, var="FIXED_SMALL"):
    D = pkg("diffusion")
    return dict(betas=D.get_named_beta_schedule("linear", steps), model_mean_type=D.ModelMeanType.EPSILON,
                model_var_type=getattr(D.ModelVarType, var), loss_type=D.LossType.MSE)


def make_diffusion(schedule):
    """"plain25": the 25-step schedule; a "ddimN" string or a list of section counts: that respacing of 1000 steps."""
    D = pkg("diffusion")
    if schedule == "plain25":
        return D.GaussianDiffusion(**diffusion_kwargs(25))
    return D.SpacedDiffusion(D.space_timesteps(1000, schedule), **diffusion_kwargs(1000))


def vp(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def run_loop(d, mode, m, kw, scale, eta, use_graph, *, x_T=None, step_noise=None, cb=None, seed=None, clip=False, shape=None,
             **more):
    """The product's loop of ``mode``; ``cb(i, t, x)`` after every step (i is None for "ddpm", which has before_step_fn
    only).  ``shape`` defaults to x_T's; ``more`` (init_motion, start_step, noise) is passed through."""
    shape = tuple(x_T.shape) if shape is None else shape
    common = dict(clip_denoised=clip, model_kwargs=kw, step_noise=step_noise, use_graph=use_graph, seed=seed, **more)
    if x_T is not None:
        common["noise"] = x_T
    if mode == "cfg":
        return d.p_sample_loop_with_cfg(m, shape, cfg_scale=scale, callback=cb, **common)
    if mode == "ddpm":
        return d.p_sample_loop(m, shape, before_step_fn=None if cb is None else (lambda t, x: cb(None, t, x)), **common)
    if mode == "ddim":
        return d.ddim_sample_loop(m, shape, eta=eta, callback=cb, **common)
    if mode == "cfg_ddim":
        return d.ddim_sample_loop_with_cfg(m, shape, cfg_scale=scale, eta=eta, callback=cb, **common)
    return d.dpm_solver_sample_loop_with_cfg(m, shape, cfg_scale=scale, callback=cb, **common)


# ---- fixtures ----------------------------------------------------------------------------------------------------------
def loops_setup(B=None):
    """loops_tiny, its precision-3 module with the uncond embedding set, the ``noises(tag, n)`` factory (of ``B`` rows, the
    golden's batch by default) and the golden batch's model kwargs."""
    g, meta = load_golden("loops_tiny")
    m, _ = build_module(meta, precision=3)
    synth = pkg("synth")
    Bg, T, F_ = g["x_T"].shape
    rows = Bg if B is None else B

    def noises(tag, n):
        return [synth.uniform_pm1((rows, T, F_), f"noise.{tag}.{i}", meta["iseed"]) * (3.0 ** 0.5) for i in range(n)]

    kw = {"xf_proj": g["xf_proj"].cuda(), "xf_out": g["xf_out"].cuda(), "length": g["length"].cuda(),
          "text": ["a person walks"] * Bg}
    m.set_uncond_embedding(g["xf_proj_uncond"][:1].cuda(), g["xf_out_uncond"][:1].cuda())
    return g, meta, m, noises, kw


def caption_trainer(m, meta, steps=1000, cfg_scale=2.5):
    Tr = pkg("trainer")
    synth = pkg("synth")
    Dt = meta["text_latent_dim"]

    def enc(text, device):  # a different embedding per caption, so a mixed-up order would show
        xo = torch.stack([synth.uniform_pm1((6, Dt), "cap." + t, 1) * (3.0 ** 0.5) for t in text])
        return xo.mean(1).to(device), xo.to(device)

    m.text_encoder_fn = enc
    args = types.SimpleNamespace(device=torch.device("cuda"), diffusion_steps=steps, is_train=False, cfg_scale=cfg_scale)
    return Tr.DDPMTrainer(args, m)


def golden_text(g):
    """The golden's caption and empty-caption embeddings as ``loop_ref``'s ``prompts`` and ``uncond``."""
    return dict(prompts=[(g["xf_proj"], g["xf_out"])], uncond=(g["xf_proj_uncond"][:1], g["xf_out_uncond"][:1]))


# ---- the restated arithmetic: f64, from abar only ----------------------------------------------------------------------
def x0_ref(abar, x, eps, eps_u=None, scale=1.0, weights=None, clip=False, known=None, mask=None):
    """pred_xstart of one step from f64 ``x`` and eps: a x - b eps with the two f32 table entries the kernels read, each x0
    clamped to [-1, 1] under ``clip`` before any combination; then CFG x0_u + s (x0_c - x0_u) (``eps_u`` given), or composed
    x0_u + s sum_k w_k (x0_k - x0_u) (``eps`` a list, ``weights`` (B, K, ...)); then the edit blend (1 - m) x0 + m k."""
    a, b = f32((1 / abar) ** 0.5), f32((1 / abar - 1) ** 0.5)

    def pred(e):
        v = a * x - b * e
        return v.clamp(-1, 1) if clip else v

    if weights is None:
        x0 = pred(eps)
        if eps_u is not None:
            x0u = pred(eps_u)
            x0 = x0u + scale * (x0 - x0u)
    else:
        x0u, acc = pred(eps_u), 0
        for k, ek in enumerate(eps):
            acc = acc + weights[:, k].double() * (pred(ek) - x0u)
        x0 = x0u + scale * acc
    if known is not None:
        x0 = (1 - mask.double()) * x0 + mask.double() * known.double()
    return x0


def update_ref(kind, acp, t, x, x0, x0_prev=None, eta=0.0, z=None):
    """x_{t-1} from x_t and the step's x0 (abar_{-1} = 1; the noise ``z`` enters at t > 0 only): "ddpm" the posterior step,
    "ddim" with eps re-derived from x0, "dpmpp" DPM-Solver++(2M) in lambda = log(alpha / sigma) with ``x0_prev`` (the x0 of
    step t + 1) None meaning first order.  "ddim_inverse": the deterministic DDIM step upwards, x_{t+1} from x_t."""
    ab = acp[t]
    if kind == "ddim_inverse":
        eps = (x - ab ** 0.5 * x0) / (1 - ab) ** 0.5
        return acp[t + 1] ** 0.5 * x0 + (1 - acp[t + 1]) ** 0.5 * eps
    abp = acp[t - 1] if t > 0 else 1.0
    if kind == "ddpm":
        beta = 1 - ab / abp
        x = beta * abp ** 0.5 / (1 - ab) * x0 + (1 - abp) * (1 - beta) ** 0.5 / (1 - ab) * x
        return x + (beta * (1 - abp) / (1 - ab)) ** 0.5 * z if t > 0 else x
    if kind == "ddim":
        eps = (x - ab ** 0.5 * x0) / (1 - ab) ** 0.5
        sig = eta * ((1 - abp) / (1 - ab)) ** 0.5 * (1 - ab / abp) ** 0.5
        x = abp ** 0.5 * x0 + max(1 - abp - sig ** 2, 0.0) ** 0.5 * eps
        return x + sig * z if t > 0 and eta > 0 else x
    assert kind == "dpmpp", kind
    if t == 0:
        return x0
    lam = lambda i: 0.5 * np.log(acp[i] / (1 - acp[i]))  # noqa: E731
    h = lam(t - 1) - lam(t)
    D_ = x0
    if x0_prev is not None:
        r = (lam(t) - lam(t + 1)) / h
        D_ = (1 + 1 / (2 * r)) * x0 - (1 / (2 * r)) * x0_prev
    return ((1 - abp) / (1 - ab)) ** 0.5 * x - abp ** 0.5 * np.expm1(-h) * D_


def loop_ref(d, mode, scale, eps_fn, *, prompts, uncond=None, x_T=None, inputs=None, check=None, eta=0.0, step_noise=None,
             order=2, start=None, direction=-1, clip=False, weights=None, known=None, mask=None, eps_hook=None,
             noise_hook=None, x0_hook=None):
    """{step index i: f64 x after step i} of the loop of ``mode`` over the schedule ``d`` (abar and timestep map only).

    ``eps_fn(x, t_orig, xf_proj, xf_out)`` is the denoiser in f64, always given the original timestep; ``prompts`` the
    (xf_proj, xf_out) pairs: one for the caption, K with ``weights`` (B, K, T, F) for composed guidance; ``uncond`` the empty
    caption's pair (one row or B), needed by the "cfg*" modes.
    ``inputs`` None: free-running from ``x_T``, x carried in f64.  Otherwise teacher-forced: step i starts from inputs[i].
    ``check``: only those steps (teacher-forced); a second-order step's predecessor x0 is recomputed from inputs[i - 1].
    ``start``: the walk begins at row ``start`` instead of the last one, and i counts from there, so DPM-Solver++'s first step
    run is first order.  ``direction`` +1: the DDIM-inversion walk, step i takes level i to level i + 1.
    ``order`` 1: DPM-Solver++ first order on every step.  ``clip``, ``known`` / ``mask``: see x0_ref.
    ``eps_hook(eps)`` on every model output (the long motions' blend of shared frames), ``noise_hook(z)`` on the step noise
    (their owner copy), ``x0_hook(x0)`` after the edit blend (the joint control's guidance iterations)."""
    acp, N = d.alphas_cumprod, d.num_timesteps
    tmap = d.timestep_map if d.timestep_map is not None else np.arange(N)
    kind = KIND[mode] if direction < 0 else "ddim_inverse"
    rows = list(range(N - 1 if start is None else start, -1, -1)) if direction < 0 else list(range(N - 1))
    x0s = {}

    def x0_at(i, x):
        if i not in x0s:
            t, B = rows[i], x.shape[0]

            def eps(xf_proj, xf_out):
                e = eps_fn(x, int(tmap[t]), xf_proj, xf_out)
                return e if eps_hook is None else eps_hook(e)

            eu = eps(uncond[0].expand(B, -1), uncond[1].expand(B, -1, -1)) if mode.startswith("cfg") else None
            ec = [eps(*p) for p in prompts]
            x0 = x0_ref(acp[t], x, ec if weights is not None else ec[0], eu, scale, weights, clip, known, mask)
            x0s[i] = x0 if x0_hook is None else x0_hook(x0)
        return x0s[i]

    x, out = None if x_T is None else x_T.double(), {}
    for i in range(len(rows)) if check is None else check:
        if inputs is not None:
            x = inputs[i].double()
        x0, x0_prev, z = x0_at(i, x), None, None
        if kind == "dpmpp" and order == 2 and i > 0:
            x0_prev = x0s[i - 1] if inputs is None else x0_at(i - 1, inputs[i - 1].double())
        if step_noise is not None:
            z = (step_noise[i] if noise_hook is None else noise_hook(step_noise[i])).double()
        x = out[i] = update_ref(kind, acp, rows[i], x, x0, x0_prev, eta, z)
    return out


def oracle_eps(g, meta, length=None):
    """eps_fn over the oracle's denoiser with the golden case's weights (``length`` defaults to the golden's)."""
    sd, eph, proj, mcfg = golden_state(meta)
    length = g["length"] if length is None else length

    def eps_fn(x, t_orig, xf_proj, xf_out):
        tt = torch.full((x.shape[0],), t_orig, dtype=torch.int64)
        with torch.no_grad():
            return R.denoiser_forward(sd, mcfg, x.float(), tt, length, xf_proj, xf_out, eph, proj).double()

    return eps_fn


def device_eps(m, length):
    """eps_fn over the product's forward."""
    @torch.no_grad()
    def eps_fn(x, t_orig, xf_proj, xf_out):
        tt = torch.full((x.shape[0],), t_orig, dtype=torch.int64)
        return m(x.float().cuda(), tt.cuda(), length.cuda(), xf_proj=xf_proj.cuda(), xf_out=xf_out.cuda()).double().cpu()

    return eps_fn


# ---- kernel-level callers ----------------------------------------------------------------------------------------------
def guided_update(x, ec, eu, xp, nz, known, mask, tab, coef, steps, t, scale, clip, xo, x0o):
    """mdm_guided_update, or mdm_guided_update_inpaint when ``known`` is given."""
    L = pkg("_lib")
    args = [vp(x), vp(ec), vp(eu), vp(xp), vp(nz)]
    tail = [C.c_int64(x.numel()), vp(tab), vp(coef), C.c_int32(steps), C.c_void_p(0), C.c_int32(t), C.c_float(scale),
            C.c_int32(clip), vp(xo), vp(x0o), C.c_void_p(L.stream_ptr())]
    if known is None:
        L.check(L.lib().mdm_guided_update(*args, *tail), "mdm_guided_update")
    else:
        L.check(L.lib().mdm_guided_update_inpaint(*args, vp(known), vp(mask), *tail), "mdm_guided_update_inpaint")


def update_kernel_ref(d, coef64, t, x, ec, eu, xp, nz, known, mask, scale, clip):
    """f64 arithmetic on the update kernels' inputs: the f64 table entries and coefficients rounded to f32 as they are handed
    over.  Returns (x_out, x0); ``known`` None: no blend."""
    a, b = f32(d.sqrt_recip_alphas_cumprod[t]), f32(d.sqrt_recipm1_alphas_cumprod[t])
    x, ec = x.double(), ec.double()
    x0 = a * x - b * ec
    if clip:
        x0 = x0.clamp(-1, 1)
    if eu is not None:
        x0u = a * x - b * eu.double()
        if clip:
            x0u = x0u.clamp(-1, 1)
        x0 = x0u + scale * (x0 - x0u)
    if known is not None:
        x0 = (1 - mask.double()) * x0 + mask.double() * known.double()
    cx, c0, c1, cn = (f32(c) for c in coef64[t])
    out = cx * x + c0 * x0
    if xp is not None:
        out = out + c1 * xp.double()
    if nz is not None:
        out = out + cn * nz.double()
    return out, x0

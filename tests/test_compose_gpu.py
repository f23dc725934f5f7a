"""GPU: composed multi-prompt guidance (x0 = x0_u + s * sum_k w_k (x0_k - x0_u) on every step of every guided sampler).

* mdm_composed_update against an f64 restatement (K = 1, 2, 3, 8, fractional and negative weights, clip, noise, x0_prev,
  editing, aligned and misaligned buffers, n % 4 != 0), and K = 1 with w = 1 bitwise equal to mdm_guided_update and
  mdm_guided_update_inpaint;
* every guided loop against the oracle's denoiser run once per prompt, with the composition and the loop restated in
  tests/sampler_ref.py from abar, teacher-forced on the device's trajectory, under timeline, body-part and negative-weight
  compositions, with an edit mask, and with prompt captions of another token count than the empty one (both ragged_text
  modes);
* row bookkeeping (identical prompts split w / 1 - w), graph == eager and two streams == one bitwise, the trainer's
  prompt_weights (K = 1 equal to plain generation, batch-split independence, bucketed == serial), the configs[1] shape in bf16.
"""
import ctypes as C
import types

import pytest
import torch

from conftest import pkg, rel_inf

import sampler_ref as S
from sampler_ref import caption_trainer as _trainer, f32, make_diffusion as _diffusion, vp as _vp
from test_motion_edit_gpu import _setup

pytestmark = pytest.mark.gpu


# ---- kernel level ------------------------------------------------------------------------------------------------------
def _composed(x, eps, K, w, xp, nz, known, mask, tab, coef, steps, t, scale, clip, xo, x0o):
    L = pkg("_lib")
    L.check(L.lib().mdm_composed_update(
        _vp(x), _vp(eps), C.c_int32(K), _vp(w), _vp(xp), _vp(nz), _vp(known), _vp(mask), C.c_int64(x.numel()), _vp(tab),
        _vp(coef), C.c_int32(steps), C.c_void_p(0), C.c_int32(t), C.c_float(scale), C.c_int32(clip), _vp(xo), _vp(x0o),
        C.c_void_p(L.stream_ptr())), "mdm_composed_update")


def _composed_ref(d, coef64, t, x, eps, K, w, xp, nz, known, mask, scale, clip):
    a, b = f32(d.sqrt_recip_alphas_cumprod[t]), f32(d.sqrt_recipm1_alphas_cumprod[t])
    x = x.double()
    e = eps.double().view(K + 1, *x.shape)

    def pred(ek):
        v = a * x - b * ek
        return v.clamp(-1, 1) if clip else v

    x0u = pred(e[K])
    x0 = x0u + scale * sum(w[k].double() * (pred(e[k]) - x0u) for k in range(K))
    if known is not None:
        x0 = (1 - mask.double()) * x0 + mask.double() * known.double()
    cx, c0, c1, cn = (f32(c) for c in coef64[t])
    out = cx * x + c0 * x0
    if xp is not None:
        out = out + c1 * xp.double()
    if nz is not None:
        out = out + cn * nz.double()
    return out, x0


@pytest.mark.parametrize("shape", [(4, 10, 263), (3, 10, 263)])  # n % 4 == 0 (dwordx4 path) and n % 4 == 2 (element-wise)
def test_composed_update_kernel_matches_f64(shape):
    d = _diffusion("ddim10")
    N, scale = d.num_timesteps, 2.5
    gen = torch.Generator().manual_seed(5)
    x, xp, nz, kn = (torch.randn(shape, generator=gen).cuda() for _ in range(4))
    mk = torch.rand(shape, generator=gen)
    mk[0, :2] = 1.0
    mk = mk.cuda()
    tab = d._device_table("cuda")
    for K in (1, 2, 3, 8):
        eps = torch.randn((K + 1,) + shape, generator=gen).cuda()
        w = (torch.rand((K,) + shape, generator=gen) * 2.5 - 1.0).cuda()  # fractional, some negative
        for kind, eta in (("ddpm", 0.0), ("ddim", 0.5), ("dpmpp", 0.0)):
            coef, coef64 = d._device_coef(kind, eta, 2, "cuda"), d.solver_coefficients(kind, eta, 2)
            for t in (N - 1, N // 2):
                for clip in (0, 1):
                    for nz_ in (nz, None):
                        for edit in (False, True):
                            xp_ = xp if kind == "dpmpp" else None
                            k_, m_ = (kn, mk) if edit else (None, None)
                            xo, x0o = torch.empty(shape, device="cuda"), torch.empty(shape, device="cuda")
                            _composed(x, eps, K, w, xp_, nz_, k_, m_, tab, coef, N, t, scale, clip, xo, x0o)
                            ref, ref0 = _composed_ref(d, coef64, t, x.cpu(), eps.cpu(), K, w.cpu(),
                                                      None if xp_ is None else xp_.cpu(), None if nz_ is None else nz_.cpu(),
                                                      None if k_ is None else kn.cpu(), None if m_ is None else mk.cpu(),
                                                      scale, clip)
                            case = (K, kind, t, clip, nz_ is None, edit)
                            # x0_k - x0_u cancels terms of ~a*|x|, each weighted: f32 error against their weighted size
                            size = d.sqrt_recip_alphas_cumprod[t] * float(x.abs().max()) * (
                                1 + scale * float(w.abs().sum(0).max()))
                            e0 = float((x0o.cpu().double() - ref0).abs().max()) / max(float(ref0.abs().max()), size)
                            e = float((xo.cpu().double() - ref).abs().max()) / max(float(ref.abs().max()),
                                                                                     f32(coef64[t][1]) * size)
                            assert e < 1e-5 and e0 < 1e-5, (case, e, e0)
                            if edit:
                                assert torch.equal(x0o[0, :2], kn[0, :2]), case
    # in place (x_out = x, x0_out = x0_prev) on buffers that are not 16-byte aligned, and aligned
    K = 3
    eps = torch.randn((K + 1,) + shape, generator=gen)
    w = torch.rand((K,) + shape, generator=gen) * 2 - 0.5
    coef, coef64 = d._device_coef("dpmpp", 0.0, 2, "cuda"), d.solver_coefficients("dpmpp", 0.0, 2)
    t = N // 2
    ref, ref0 = _composed_ref(d, coef64, t, x.cpu(), eps, K, w, xp.cpu(), None, kn.cpu(), mk.cpu(), scale, False)
    for off in (1, 0):
        def buf(v):
            b = torch.zeros(v.numel() + off, device="cuda")
            out = b[off:].view(v.shape)
            out.copy_(v)
            return out
        xi, pi, ki, mi, ei, wi = (buf(v) for v in (x, xp, kn, mk, eps.cuda(), w.cuda()))
        _composed(xi, ei, K, wi, pi, None, ki, mi, tab, coef, N, t, scale, 0, xi, pi)
        assert rel_inf(xi.cpu(), ref) < 1e-5 and rel_inf(pi.cpu(), ref0) < 1e-5, off
    # a zero coefficient's operand is not read: NaN in x0_prev does not reach a DDIM update (c1 = 0)
    coef = d._device_coef("ddim", 0.0, 2, "cuda")
    xo = torch.empty(shape, device="cuda")
    _composed(x, eps.cuda(), K, w.cuda(), torch.full(shape, float("nan"), device="cuda"), None, None, None, tab, coef, N, t,
              scale, 0, xo, None)
    assert torch.isfinite(xo).all()


@pytest.mark.parametrize("shape", [(4, 10, 263), (3, 10, 263)])
def test_one_prompt_of_weight_one_is_the_guided_update_bitwise(shape):
    d = _diffusion("ddim10")
    N = d.num_timesteps
    gen = torch.Generator().manual_seed(6)
    x, ec, eu, xp, nz, kn = (torch.randn(shape, generator=gen).cuda() for _ in range(6))
    mk = torch.rand(shape, generator=gen).cuda()
    eps, ones = torch.cat([ec, eu]), torch.ones(shape, device="cuda")
    tab = d._device_table("cuda")
    for kind, eta in (("ddpm", 0.0), ("ddim", 0.5), ("dpmpp", 0.0)):
        coef = d._device_coef(kind, eta, 2, "cuda")
        for t in (N - 1, N // 2, 0):
            for clip in (0, 1):
                for nz_ in (nz, None):
                    for k_, m_ in ((None, None), (kn, mk)):
                        xp_ = xp if kind == "dpmpp" else None
                        a, a0, b, b0 = (torch.empty(shape, device="cuda") for _ in range(4))
                        _composed(x, eps, 1, ones, xp_, nz_, k_, m_, tab, coef, N, t, 7.5, clip, a, a0)
                        S.guided_update(x, ec, eu, xp_, nz_, k_, m_, tab, coef, N, t, 7.5, clip, b, b0)
                        case = (kind, t, clip, nz_ is None, k_ is None)
                        assert torch.equal(a, b) and torch.equal(a0, b0), case


# ---- loops against the oracle ------------------------------------------------------------------------------------------
def _prompts(g, meta, K):
    """K prompts of the loops_tiny batch: the golden caption, then seeded extra embeddings (CPU)."""
    synth = pkg("synth")
    B, Nt, Dt = g["xf_out"].shape
    out = [(g["xf_proj"], g["xf_out"])]
    for k in range(1, K):
        xo = synth.uniform_pm1((B, Nt, Dt), f"compose.prompt.{k}", meta["iseed"]) * (3.0 ** 0.5)
        out.append((xo.mean(1), xo))
    return out


def _weights(kind, B, K, T, F_):
    MC, E = pkg("motion_compose"), pkg("motion_edit")
    if kind == "timeline":
        w = MC.timeline_weights(T, [T // K * (k + 1) for k in range(K - 1)], blend=4)[None]
    elif kind == "body":
        parts = [E.UPPER_BODY, E.LOWER_BODY] if K == 2 else [E.LOWER_BODY, (16, 17, 18, 19, 20, 21),
                                                            (3, 6, 9, 12, 13, 14, 15)]
        w = MC.body_part_weights(parts)[None, :, None]
    else:  # negative prompts: the last prompt pushed away from, per-sample weights
        w = torch.tensor([[1.0, 0.75, -0.5][:K], [1.25, -0.4, 0.3][:K]])[:, :, None, None]
    return torch.broadcast_to(w, (B, K, T, F_)).contiguous()


def _ckw(kw, prompts, w):
    return {"length": kw["length"], "compose_weights": w.cuda(),
            "compose_xf_proj": torch.stack([p[0] for p in prompts], 1).cuda(),
            "compose_xf_out": torch.stack([p[1] for p in prompts], 1).cuda()}


def _check_loop(g, meta, m, d, mode, eta, ckw, prompts, w, noises, known=None, mask=None, uncond=None, graph_vs_eager=True):
    N, scale = d.num_timesteps, meta["cfg_scale"]
    uncond = S.golden_text(g)["uncond"] if uncond is None else uncond
    ns = noises(f"compose.{mode}.{eta}", N)
    finals = []
    for use_graph in ((True, False) if graph_vs_eager else (True,)):
        got = []
        out = S.run_loop(d, mode, m, ckw, scale, eta, use_graph, x_T=g["x_T"].cuda(), step_noise=ns,
                         cb=lambda i, t, x: got.append(x.clone().cpu())).cpu()
        assert len(got) == N and torch.equal(out, got[-1]) and torch.isfinite(out).all()
        if use_graph:
            check = sorted({0, 1, N // 2, N - 2, N - 1})
            want = S.loop_ref(d, mode, scale, S.oracle_eps(g, meta), prompts=prompts, weights=w, uncond=uncond,
                              inputs=[g["x_T"]] + got[:-1], check=check, eta=eta, step_noise=ns, known=known, mask=mask)
            for i in check:
                e = rel_inf(got[i], want[i])
                assert e < 1e-3, (i, e)
        finals.append(out)
    if graph_vs_eager:
        assert torch.equal(finals[0], finals[1])
    return finals[0]


LOOPS = [("cfg", 0.0), ("cfg_ddim", 0.0), ("cfg_ddim", 0.5), ("cfg_dpmpp", 0.0)]
COMPS = [("timeline", 2), ("timeline", 3), ("body", 2), ("body", 3), ("negative", 2), ("negative", 3)]


@pytest.mark.parametrize("comp,K", COMPS)
@pytest.mark.parametrize("schedule", ["plain25", "ddim10"])
@pytest.mark.parametrize("mode,eta", LOOPS)
def test_composed_loops_match_the_oracle(mode, eta, schedule, comp, K):
    g, meta, m, noises, kw, known = _setup()
    d = _diffusion(schedule)
    B, T, F_ = g["x_T"].shape
    prompts, w = _prompts(g, meta, K), _weights(comp, B, K, T, F_)
    _check_loop(g, meta, m, d, mode, eta, _ckw(kw, prompts, w), prompts, w, noises)


@pytest.mark.parametrize("mode,eta", [("cfg", 0.0), ("cfg_dpmpp", 0.0)])
def test_composition_with_an_edit_mask_matches_the_oracle(mode, eta):
    g, meta, m, noises, kw, known = _setup()
    E = pkg("motion_edit")
    d = _diffusion([4, 3, 3])
    B, T, F_ = g["x_T"].shape
    prompts, w = _prompts(g, meta, 3), _weights("timeline", B, 3, T, F_)
    mask = torch.broadcast_to(E.prefix_mask(T, 4), (B, T, F_))
    ckw = dict(_ckw(kw, prompts, w), inpaint_motion=known.cuda(), inpaint_mask=mask.cuda())
    out = _check_loop(g, meta, m, d, mode, eta, ckw, prompts, w, noises, known, mask)
    assert torch.equal(out[:, :4], known[:, :4])


@pytest.mark.parametrize("ragged_text", ["mask", "split"])
def test_ragged_prompt_captions_match_the_oracle(ragged_text):
    """Prompt captions of 6 tokens against an empty caption of 3: per-row token counts over (K + 1)B rows ("mask") or
    K + 1 forwards with their own text caches ("split")."""
    g, meta, m, noises, kw, known = _setup()
    synth = pkg("synth")
    m.ragged_text = ragged_text
    B, T, F_ = g["x_T"].shape
    xo_u = synth.uniform_pm1((1, 3, meta["text_latent_dim"]), "compose.u.short", 5) * 1.7
    m.set_uncond_embedding(xo_u.mean(1).cuda(), xo_u.cuda())
    d = _diffusion("ddim10")
    prompts, w = _prompts(g, meta, 2), _weights("negative", B, 2, T, F_)
    for mode, eta in (("cfg_ddim", 0.5), ("cfg_dpmpp", 0.0)):
        _check_loop(g, meta, m, d, mode, eta, _ckw(kw, prompts, w), prompts, w, noises, uncond=(xo_u.mean(1), xo_u),
                    graph_vs_eager=mode == "cfg_dpmpp")


# ---- bookkeeping, graph, streams ---------------------------------------------------------------------------------------
def test_identical_prompts_split_by_weight_equal_one_prompt():
    g, meta, m, noises, kw, known = _setup()
    MC = pkg("motion_compose")
    d = _diffusion("ddim10")
    B, T, F_ = g["x_T"].shape
    p = _prompts(g, meta, 2)[1]
    one = _ckw(kw, [p], torch.ones(B, 1, T, F_))
    base = d.dpm_solver_sample_loop_with_cfg(m, (B, T, F_), noise=g["x_T"].cuda(), clip_denoised=False, model_kwargs=one,
                                             cfg_scale=meta["cfg_scale"]).cpu()
    def run(w):
        w = torch.broadcast_to(w.reshape(1, 2, -1, 1), (B, 2, T, F_))
        return d.dpm_solver_sample_loop_with_cfg(m, (B, T, F_), noise=g["x_T"].cuda(), clip_denoised=False,
                                                 model_kwargs=_ckw(kw, [p, p], w), cfg_scale=meta["cfg_scale"]).cpu()

    first = run(torch.tensor([1.0, 0.0]))  # the same (K + 1)B-row forward, all weight on the first copy
    binary = MC.timeline_weights(T, [7])[None]                    # w in {0, 1}: each frame takes one of the copies
    frac = MC.timeline_weights(T, [8], blend=10)[None]            # fractional w, 1 - w
    for w, exact in ((binary, True), (frac, False), (torch.tensor([0.3, 0.7]), False)):
        out = run(w)
        e, e1 = rel_inf(out, first), rel_inf(out, base)
        print(f"[w / 1 - w] binary={exact}: rel_inf {e:.3e} against weights (1, 0), {e1:.3e} against one prompt "
              f"(bitwise: {torch.equal(out, base)})")
        if exact:
            assert torch.equal(out, first)
        else:
            assert e < 1e-5, e
        assert e1 < 1e-5, e1  # one prompt runs a forward of 2B rows instead of 3B
    # one step: w d + (1 - w) d against d, within 1e-6
    t = torch.full((B,), d.num_timesteps // 2, dtype=torch.int64, device="cuda")
    x_t = g["x_T"].cuda()
    a = d.ddim_sample_with_cfg(m, x_t, t, clip_denoised=False, model_kwargs=one, cfg_scale=meta["cfg_scale"], eta=0.0)
    w = torch.broadcast_to(frac.reshape(1, 2, T, 1), (B, 2, T, F_))
    b = d.ddim_sample_with_cfg(m, x_t, t, clip_denoised=False, model_kwargs=_ckw(kw, [p, p], w),
                               cfg_scale=meta["cfg_scale"], eta=0.0)
    for k in ("sample", "pred_xstart"):
        assert rel_inf(b[k].cpu(), a[k].cpu()) < 1e-6, k


@pytest.mark.parametrize("mode,eta", [("cfg", 0.0), ("cfg_ddim", 0.5), ("cfg_dpmpp", 0.0)])
def test_graph_equals_eager_and_two_streams_equal_one_bitwise(mode, eta):
    g, meta, m, noises, kw, known = _setup()
    d = _diffusion([4, 3, 3])
    B, T, F_ = g["x_T"].shape
    prompts = _prompts(g, meta, 3)
    ckw = _ckw(kw, prompts, _weights("timeline", B, 3, T, F_))
    outs = {}
    for use_graph, streams in ((True, 1), (False, 1), (True, 2)):
        r = d._runner(m, (B, T, F_), ckw, "cuda", mode, meta["cfg_scale"], eta, False, use_graph, streams)
        assert r.R == 4 * B and (streams == 1 or r.chunks is not None)
        outs[(use_graph, streams)] = r.run(g["x_T"].cuda(), None, False, None, seed=11).cpu()
    assert torch.isfinite(outs[(True, 1)]).all()
    assert torch.equal(outs[(True, 1)], outs[(False, 1)])
    assert torch.equal(outs[(True, 1)], outs[(True, 2)])


def test_progressive_loops_single_steps_and_unguided_modes():
    g, meta, m, noises, kw, known = _setup()
    d = _diffusion("ddim10")
    B, T, F_ = g["x_T"].shape
    prompts = _prompts(g, meta, 2)
    ckw = _ckw(kw, prompts, _weights("body", B, 2, T, F_))
    sc = meta["cfg_scale"]
    ns = noises("compose.single", d.num_timesteps)
    x_t = g["x_T"].cuda()
    t = torch.full((B,), d.num_timesteps - 1, dtype=torch.int64, device="cuda")
    loop = d.ddim_sample_loop_with_cfg(m, (B, T, F_), noise=x_t, clip_denoised=False, model_kwargs=ckw, cfg_scale=sc,
                                       eta=0.5, step_noise=ns, use_graph=False).cpu()
    step = d.ddim_sample_with_cfg(m, x_t, t, clip_denoised=False, model_kwargs=ckw, cfg_scale=sc, eta=0.5,
                                  noise=ns[0].cuda())
    ref = dict(prompts=prompts, weights=ckw["compose_weights"].cpu(), uncond=S.golden_text(g)["uncond"])
    want = S.loop_ref(d, "cfg_ddim", sc, S.oracle_eps(g, meta), inputs=[g["x_T"]], check=[0], eta=0.5, step_noise=ns, **ref)
    assert rel_inf(step["sample"].cpu(), want[0]) < 1e-3
    got = []
    again = d.ddim_sample_loop_with_cfg(m, (B, T, F_), noise=x_t, clip_denoised=False, model_kwargs=ckw, cfg_scale=sc,
                                        eta=0.5, step_noise=ns, callback=lambda i, t_, x: got.append(x.clone())).cpu()
    assert torch.equal(got[0].cpu(), step["sample"].cpu()) and torch.equal(loop, again)
    one = d.p_sample_with_cfg(m, x_t, torch.full((B,), 3, dtype=torch.int64, device="cuda"), clip_denoised=False,
                              model_kwargs=ckw, cfg_scale=sc, noise=ns[0].cuda())
    want = S.loop_ref(d, "cfg", sc, S.oracle_eps(g, meta), inputs={d.num_timesteps - 4: g["x_T"]}, check=[d.num_timesteps - 4],
                      step_noise={d.num_timesteps - 4: ns[0]}, **ref)
    assert rel_inf(one["sample"].cpu(), want[d.num_timesteps - 4]) < 1e-3
    for bad in (lambda: d.ddim_sample_loop(m, (B, T, F_), noise=x_t, model_kwargs=ckw),
                lambda: d.p_sample_loop(m, (B, T, F_), noise=x_t, model_kwargs=ckw),
                lambda: list(d.ddim_sample_loop_progressive(m, (B, T, F_), noise=x_t, model_kwargs=ckw)),
                lambda: d.ddim_sample(m, x_t, t, model_kwargs=ckw),
                lambda: d.ddim_sample_loop_with_cfg(m, (B, T, F_), noise=x_t, model_kwargs=dict(ckw, xf_proj=kw["xf_proj"],
                                                                                               xf_out=kw["xf_out"]))):
        with pytest.raises(ValueError):
            bad()


# ---- trainer -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler,steps", [("ddim", 10), ("dpmpp2m", 10), ("ddpm", None)])
def test_one_prompt_of_weight_one_equals_plain_generation(sampler, steps):
    g, meta, m, noises, kw, known = _setup()
    tr = _trainer(m, meta, steps=25 if sampler == "ddpm" else 1000)
    caps = ["a", "b", "c"]
    lens = torch.tensor([16, 12, 16])
    opts = dict(seed=4, sampler=sampler, sample_steps=steps, batch_size=3)
    comp = torch.stack(tr.generate([(c,) for c in caps], lens, 263, prompt_weights=1, **opts)).cpu()
    plain = torch.stack(tr.generate(caps, lens, 263, **opts)).cpu()
    if sampler != "ddpm":
        assert torch.equal(comp, plain)
        return
    # guided DDPM: composed, it runs the "ddpm" coefficient table through the fused update, as an all-zero edit mask does
    zero = torch.stack(tr.generate(caps, lens, 263, edit_motion=torch.zeros(3, 16, 263), edit_mask=0.0, **opts)).cpu()
    assert torch.equal(comp, zero)
    e = rel_inf(comp, plain)
    print(f"[K = 1] guided DDPM-25 against mdm_cfg_posterior_step: rel_inf {e:.3e}")
    assert e <= 1e-5, e


def test_trainer_composition_is_independent_of_the_batch_split():
    g, meta, m, noises, kw, known = _setup()
    MC, E = pkg("motion_compose"), pkg("motion_edit")
    tr = _trainer(m, meta)
    caps = [("walk", "sit", "wave"), ("run", "jump", "kick"), ("turn", "crouch", "bow"), ("step", "spin", "clap")]
    w = torch.stack([MC.timeline_weights(16, [6], blend=2)[0], MC.timeline_weights(16, [6], blend=2)[1],
                     -0.5 * torch.ones(16, 1)])[None] * torch.tensor([1.0, 0.8, 1.2, 1.0])[:, None, None, None]
    opts = dict(seed=3, sampler="ddim", sample_steps=10, eta=0.5, prompt_weights=w)
    same = torch.tensor([16, 16, 16, 16])
    one = torch.stack(tr.generate(caps, same, 263, batch_size=1, **opts)).cpu()
    two = torch.stack(tr.generate(caps, same, 263, batch_size=2, **opts)).cpu()
    assert torch.isfinite(one).all() and rel_inf(one, two) < 1e-5, rel_inf(one, two)
    plain = torch.stack(tr.generate([c[0] for c in caps], same, 263, batch_size=2, seed=3, sampler="ddim",
                                    sample_steps=10, eta=0.5)).cpu()
    assert not torch.equal(plain, one)
    lens = torch.tensor([8, 16, 12, 4])
    k = pkg("synth").uniform_pm1((4, 16, 263), "compose.trainer", 3).cuda()
    bp = MC.body_part_weights([E.UPPER_BODY, E.LOWER_BODY, []])
    for extra in (dict(opts), dict(opts, sampler="dpmpp2m", eta=0.0, prompt_weights=bp[None, :, None]),
                  dict(opts, sampler="dpmpp2m", eta=0.0, edit_motion=k, edit_mask=E.prefix_mask(16, 3))):
        serial = tr.generate(caps, lens, 263, batch_size=2, **extra)
        bucket = tr.generate_bucketed(caps, lens, 263, batch_size=2, unit_length=4, **extra)
        for i, n in enumerate(lens.tolist()):
            e = rel_inf(bucket[i][:n].cpu(), serial[i][:n].cpu())
            assert e < 1e-4, (i, e)
            if "edit_motion" in extra:
                assert torch.equal(serial[i][:3], k[i, :3]) and torch.equal(bucket[i][:3], k[i, :3])
    joints = tr.generate_joints(caps, lens, 263, torch.zeros(263).numpy(), torch.ones(263).numpy(), batch_size=2, **opts)
    assert [tuple(j.shape) for j in joints] == [(n, 22, 3) for n in lens.tolist()]


def test_configs1_shape_bf16_two_prompts():
    """configs[1] shape (small, 8 experts, B=32, T=196, guided, 1000-step schedule) in bf16: DPM-Solver++(2M)-20 with two
    prompts through DDPMTrainer.generate is finite, and two copies of each caption under a timeline split give the plain
    generation."""
    T_ = pkg("transformer")
    synth = pkg("synth")
    MC = pkg("motion_compose")
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
    index = {f"caption {i}": i for i in range(B)}
    index.update({f"other {i}": (i + 7) % B for i in range(B)})

    def enc(text, device):
        ids = torch.tensor([index[t] for t in text])
        return xf_proj[ids].to(device), xf_out[ids].to(device)

    m.text_encoder_fn = enc
    Tr = pkg("trainer")
    tr = Tr.DDPMTrainer(types.SimpleNamespace(device=torch.device("cuda"), diffusion_steps=1000, is_train=False,
                                              cfg_scale=7.5), m)
    opts = dict(batch_size=B, seed=5, sampler="dpmpp2m", sample_steps=20)
    caps = [f"caption {i}" for i in range(B)]
    w = MC.timeline_weights(T, [98], blend=20)[None]
    two = torch.stack(tr.generate([(c, f"other {i}") for i, c in enumerate(caps)], length, 263, prompt_weights=w,
                                  **opts)).cpu()
    assert torch.isfinite(two).all()
    plain = torch.stack(tr.generate(caps, length, 263, **opts)).cpu()
    same = torch.stack(tr.generate([(c, c) for c in caps], length, 263, prompt_weights=MC.timeline_weights(T, [98])[None],
                                   **opts)).cpu()
    first = torch.stack(tr.generate([(c, c) for c in caps], length, 263, prompt_weights=torch.tensor([[1.0, 0.0]]),
                                    **opts)).cpu()
    e = rel_inf(same, plain)
    print(f"[configs[1] bf16] two copies of each caption split at frame 98 against plain: rel_inf {e:.3e} (bitwise: "
          f"{torch.equal(same, plain)}); two prompts against plain: {rel_inf(two, plain):.3e}")
    assert torch.equal(same, first)  # the same rows, whichever copy each frame takes
    assert e < 5e-2, e  # plain generation runs a forward of 2B rows instead of 3B

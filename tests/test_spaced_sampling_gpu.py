"""GPU: timestep respacing and the few-step guided samplers (guided DDIM, DPM-Solver++(2M)).

* the two new kernels (csrc/solver.hip) against an f64 restatement on random inputs;
* the spaced loops against the oracle's denoiser fed the ORIGINAL timesteps, with the solver arithmetic restated in
  tests/sampler_ref.py from abar and lambda (not from the product's coefficient tables), free-running;
* consistency: every step kept == the plain schedule, order-1 DPM-Solver++ == DDIM at eta 0, graph == eager and two
  streams == one bitwise, the trainer's result independent of the batch split;
* the configs[1] shape in bf16 through DDPMTrainer.generate.
"""
import ctypes as C
import types

import pytest
import torch

from conftest import pkg, rel_inf

import sampler_ref as S
from sampler_ref import caption_trainer as _trainer, diffusion_kwargs as _kw, loops_setup as _setup, vp as _vp

pytestmark = pytest.mark.gpu


def _spaced(spacing, steps=1000):
    D = pkg("diffusion")
    return D.SpacedDiffusion(D.space_timesteps(steps, spacing), **_kw(steps))


# ---- kernel level ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", ["plain50", "ddim10", "ddim50"])
def test_guided_update_kernel_matches_f64(schedule):
    d = pkg("diffusion").GaussianDiffusion(**_kw(50)) if schedule == "plain50" else _spaced(schedule)
    N = d.num_timesteps
    gen = torch.Generator().manual_seed(1)
    shape = (3, 10, 263)  # n = 7890: not a multiple of 4, the last quad takes the element-wise tail
    x, ec, eu, xp, nz = (torch.randn(shape, generator=gen) for _ in range(5))
    tab = d._device_table("cuda")
    cases = [("ddim", 0.0, 2), ("ddim", 0.5, 2), ("dpmpp", 0.0, 2), ("dpmpp", 0.0, 1)]
    for kind, eta, order in cases:
        coef = d._device_coef(kind, eta, order, "cuda")
        coef64 = d.solver_coefficients(kind, eta, order)
        for t in (N - 1, N // 2, 0):
            for clip in (0, 1):
                for guided in (True, False):
                    eu_ = eu if guided else None
                    xo, x0o = torch.empty(shape, device="cuda"), torch.empty(shape, device="cuda")
                    S.guided_update(x.cuda(), ec.cuda(), eu_.cuda() if guided else None, xp.cuda(), nz.cuda(), None, None, tab,
                                    coef, N, t, 2.5, clip, xo, x0o)
                    ref, ref0 = S.update_kernel_ref(d, coef64, t, x, ec, eu_, xp, nz, None, None, 2.5, clip)
                    e = rel_inf(xo.cpu(), ref)
                    # a clamped x0 is at most 1 while a*x - b*eps cancels terms of ~a*|x| (a = 359 at t = 49 of 50): its f32
                    # error is measured against the size of those terms (unclamped, that IS the size of x0)
                    den = max(float(ref0.abs().max()), float(d.sqrt_recip_alphas_cumprod[t] * x.abs().max()) if clip else 0.0)
                    e0 = float((x0o.cpu().double() - ref0).abs().max()) / den
                    assert e < 1e-5 and e0 < 1e-5, (kind, eta, order, t, clip, guided, e, e0)
    # in place (x_out = x, x0_out = x0_prev) on buffers that are not 16-byte aligned (the element-wise form)
    coef, coef64 = d._device_coef("dpmpp", 0.0, 2, "cuda"), d.solver_coefficients("dpmpp", 0.0, 2)
    t = N // 2
    xb, pb = torch.zeros(x.numel() + 1, device="cuda"), torch.zeros(x.numel() + 1, device="cuda")
    xi, pi = xb[1:].view(shape), pb[1:].view(shape)
    xi.copy_(x.cuda()), pi.copy_(xp.cuda())
    S.guided_update(xi, ec.cuda(), eu.cuda(), pi, None, None, None, tab, coef, N, t, 2.5, 0, xi, pi)
    ref, ref0 = S.update_kernel_ref(d, coef64, t, x, ec, eu, xp, None, None, None, 2.5, False)
    assert rel_inf(xi.cpu(), ref) < 1e-5 and rel_inf(pi.cpu(), ref0) < 1e-5
    # the same in place on aligned buffers
    xa, pa = x.cuda(), xp.cuda()
    S.guided_update(xa, ec.cuda(), eu.cuda(), pa, None, None, None, tab, coef, N, t, 2.5, 0, xa, pa)
    assert rel_inf(xa.cpu(), ref) < 1e-5 and rel_inf(pa.cpu(), ref0) < 1e-5


def test_fill_timesteps_mapped_reads_the_device_counter():
    L = pkg("_lib")
    d = _spaced([4, 3, 3])
    tmap = d._device_map("cuda")
    N = d.num_timesteps
    dst = torch.full((37,), -7, dtype=torch.int64, device="cuda")
    t_dev = torch.zeros(1, dtype=torch.int32, device="cuda")
    for t in list(range(N)) + [-3, N + 5]:  # a stale counter is clamped into the map
        t_dev.fill_(t)
        L.check(L.lib().mdm_fill_timesteps_mapped(_vp(dst), C.c_int64(dst.numel()), _vp(t_dev), _vp(tmap), C.c_int32(N),
                                                  C.c_void_p(L.stream_ptr())), "mdm_fill_timesteps_mapped")
        want = int(d.timestep_map[min(max(t, 0), N - 1)])
        assert bool((dst.cpu() == want).all()), (t, want)


# ---- loops against the oracle --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("spacing", ["ddim10", [4, 3, 3]])
@pytest.mark.parametrize("solver", ["ddim0", "ddim0.5", "dpmpp2m"])
def test_spaced_guided_loops_match_the_oracle(solver, spacing, use_graph):
    """1000-step schedule sampled in 10 steps.  The graph run uses the stem cache, whose gather clamps t into the length it
    was built over: a cache over the spaced length would hand the time embedding of step 9 to timesteps 100..999."""
    g, meta, m, noises, kw = _setup()
    d = _spaced(spacing)
    N, scale = d.num_timesteps, meta["cfg_scale"]
    shape = tuple(g["x_T"].shape)
    got = {}
    cb = lambda i, t, x: got.__setitem__(i, x.clone().cpu())  # noqa: E731
    if solver == "dpmpp2m":
        d.dpm_solver_sample_loop_with_cfg(m, shape, noise=g["x_T"].cuda(), clip_denoised=False, model_kwargs=kw,
                                          cfg_scale=scale, use_graph=use_graph, callback=cb)
        want = S.loop_ref(d, "cfg_dpmpp", scale, S.oracle_eps(g, meta), x_T=g["x_T"], **S.golden_text(g))
    else:
        eta = float(solver[4:])
        ns = noises(f"spaced.{eta}", N)
        d.ddim_sample_loop_with_cfg(m, shape, noise=g["x_T"].cuda(), clip_denoised=False, model_kwargs=kw, cfg_scale=scale,
                                    eta=eta, step_noise=ns, use_graph=use_graph, callback=cb)
        want = S.loop_ref(d, "cfg_ddim", scale, S.oracle_eps(g, meta), x_T=g["x_T"], eta=eta, step_noise=ns,
                          **S.golden_text(g))
    for i in (0, N // 2, N - 2, N - 1):
        e = rel_inf(got[i], want[i])
        assert e < 1e-3, (i, e)


def test_every_step_kept_equals_the_plain_schedule():
    """SpacedDiffusion over all 50 steps: guided DDPM (the existing loop, through the timestep map) == the plain loop."""
    g, meta, m, noises, kw = _setup()
    D = pkg("diffusion")
    plain, sp = D.GaussianDiffusion(**_kw(50)), D.SpacedDiffusion(range(50), **_kw(50))
    ns = noises("kept", 50)
    outs = [d.p_sample_loop_with_cfg(m, tuple(g["x_T"].shape), noise=g["x_T"].cuda(), clip_denoised=False, model_kwargs=kw,
                                     cfg_scale=meta["cfg_scale"], step_noise=ns).cpu() for d in (plain, sp)]
    assert rel_inf(outs[1], outs[0]) <= 1e-5


def test_first_order_dpm_solver_equals_guided_ddim_at_eta_zero():
    g, meta, m, noises, kw = _setup()
    d = _spaced("ddim10")
    shape, x_T = tuple(g["x_T"].shape), g["x_T"].cuda()
    a = d.dpm_solver_sample_loop_with_cfg(m, shape, noise=x_T, clip_denoised=False, model_kwargs=kw,
                                          cfg_scale=meta["cfg_scale"], order=1).cpu()
    b = d.ddim_sample_loop_with_cfg(m, shape, noise=x_T, clip_denoised=False, model_kwargs=kw, cfg_scale=meta["cfg_scale"],
                                    eta=0.0).cpu()
    c = d.dpm_solver_sample_loop_with_cfg(m, shape, noise=x_T, clip_denoised=False, model_kwargs=kw,
                                          cfg_scale=meta["cfg_scale"], order=2).cpu()
    assert rel_inf(a, b) <= 1e-4
    assert rel_inf(c, b) > 1e-4  # the second-order steps do change the result


def test_single_guided_ddim_step_is_the_first_loop_step():
    g, meta, m, noises, kw = _setup()
    d = _spaced("ddim10")
    shape, x_T = tuple(g["x_T"].shape), g["x_T"].cuda()
    ns = noises("single", 1)
    first = {}
    d.ddim_sample_loop_with_cfg(m, shape, noise=x_T, clip_denoised=False, model_kwargs=kw, cfg_scale=meta["cfg_scale"],
                                eta=0.5, step_noise=ns * d.num_timesteps, use_graph=False,
                                callback=lambda i, t, x: first.setdefault(i, x.clone().cpu()))
    t = torch.full((shape[0],), d.num_timesteps - 1, dtype=torch.int64, device="cuda")
    out = d.ddim_sample_with_cfg(m, x_T, t, clip_denoised=False, model_kwargs=kw, cfg_scale=meta["cfg_scale"], eta=0.5,
                                 noise=ns[0].cuda())
    assert torch.equal(out["sample"].cpu(), first[0])


@pytest.mark.parametrize("mode,eta", [("cfg_ddim", 0.5), ("cfg_dpmpp", 0.0)])
def test_graph_equals_eager_and_two_streams_equal_one_bitwise(mode, eta):
    g, meta, m, noises, kw = _setup()
    d = _spaced([4, 3, 3])
    shape = tuple(g["x_T"].shape)
    outs = {}
    for use_graph, streams in ((True, 1), (False, 1), (True, 2)):
        r = d._runner(m, shape, kw, "cuda", mode, meta["cfg_scale"], eta, False, use_graph, streams)
        outs[(use_graph, streams)] = r.run(g["x_T"].cuda(), None, False, None, seed=11).cpu()
    assert torch.isfinite(outs[(True, 1)]).all()
    assert torch.equal(outs[(True, 1)], outs[(False, 1)])
    assert torch.equal(outs[(True, 1)], outs[(True, 2)])


# ---- trainer -----------------------------------------------------------------------------------------------------------
def test_trainer_generate_few_step_is_independent_of_the_batch_split():
    g, meta, m, noises, kw = _setup()
    tr = _trainer(m, meta)
    caps = ["a", "b", "c", "d"]
    opts = dict(seed=3, sampler="ddim", sample_steps=10, eta=0.5)
    same = torch.tensor([16, 16, 16, 16])
    two = torch.stack(tr.generate(caps, same, 263, batch_size=2, **opts)).cpu()
    four = torch.stack(tr.generate(caps, same, 263, batch_size=4, **opts)).cpu()
    assert torch.isfinite(two).all()
    assert torch.equal(two, four)
    lens = torch.tensor([8, 16, 12, 4])
    serial = tr.generate(caps, lens, 263, batch_size=2, **opts)
    bucket = tr.generate_bucketed(caps, lens, 263, batch_size=2, unit_length=4, **opts)
    for i, n in enumerate(lens.tolist()):
        e = rel_inf(bucket[i][:n].cpu(), serial[i][:n].cpu())
        assert e < 1e-4, (i, e)
    # the defaults are the full guided DDPM loop; the few-step samplers give other (finite) results
    ddpm = torch.stack(tr.generate(caps, same, 263, batch_size=4, seed=3)).cpu()
    xp, xo = m.encode_text(caps, "cuda")
    want = tr.diffusion.p_sample_loop_with_cfg(m, (4, 16, 263), clip_denoised=False, cfg_scale=2.5, seed=3,
                                               model_kwargs={"xf_proj": xp, "xf_out": xo, "length": same, "text": caps}).cpu()
    assert torch.equal(ddpm, want)
    dpm = torch.stack(tr.generate(caps, same, 263, batch_size=4, seed=3, sampler="dpmpp2m", sample_steps=10)).cpu()
    assert torch.isfinite(dpm).all() and not torch.equal(dpm, four)
    with pytest.raises(ValueError):
        tr.generate(caps, same, 263, sampler="dpmpp2m", sample_steps=10, eta=0.5)


def test_configs1_shape_bf16_few_step_generation():
    """configs[1] shape (small, 8 experts, B=32, T=196, guided, 1000-step schedule) in bf16: DDIM-50 and DPM-Solver++(2M)-20
    through DDPMTrainer.generate (graph) against the same loops run eagerly.  Distances to a 1000-step DDIM run are printed
    as information only: the weights are synthetic, so they say nothing about sample quality."""
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
    kw = {"xf_proj": xf_proj.cuda(), "xf_out": xf_out.cuda(), "length": length, "text": caps}
    res = {}
    for sampler, steps in (("ddim", 50), ("dpmpp2m", 20), ("ddim", 20)):
        res[(sampler, steps)] = torch.stack(tr.generate(caps, length, 263, batch_size=B, seed=5, sampler=sampler,
                                                        sample_steps=steps)).cpu()
        assert torch.isfinite(res[(sampler, steps)]).all(), (sampler, steps)
        d = tr.sampling_diffusion(sampler, steps)
        loop = d.ddim_sample_loop_with_cfg if sampler == "ddim" else d.dpm_solver_sample_loop_with_cfg
        eager = loop(m, (B, T, 263), clip_denoised=False, model_kwargs=kw, cfg_scale=7.5, use_graph=False, seed=5).cpu()
        assert torch.equal(res[(sampler, steps)], eager), (sampler, steps)
    full = torch.stack(tr.generate(caps, length, 263, batch_size=B, seed=5, sampler="ddim")).cpu()
    assert torch.isfinite(full).all()
    print(f"[configs[1] bf16] rel_inf to guided DDIM-1000 (eta 0): DPM-Solver++(2M)-20 {rel_inf(res[('dpmpp2m', 20)], full):.3e}, "
          f"DDIM-20 {rel_inf(res[('ddim', 20)], full):.3e}, DDIM-50 {rel_inf(res[('ddim', 50)], full):.3e}")

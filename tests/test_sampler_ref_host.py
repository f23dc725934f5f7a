"""CPU: tests/sampler_ref.py, the f64 restatement the sampler GPU tests are judged against.

* pinned to the reference: ``loop_ref`` free-running with the oracle's denoiser against the loops_tiny goldens the reference
  recorded (guided DDPM trajectory and final, clipped DDIM finals), at the bound tests/test_oracle_golden.py puts on
  oracle/diffusion_ref.py against the same goldens;
* pinned to the product's host table: ``update_ref`` against cx x + c0 x0 + c1 x0_prev + cn z with the f64 rows of
  ``GaussianDiffusion.solver_coefficients``, at every row, at the tolerance tests/test_respacing_host.py uses for the same
  identity on the coefficients;
* each option of ``loop_ref`` does what its doc line says.
"""
import pytest
import torch

from conftest import load_golden, pkg, rel_inf

import sampler_ref as S


def _golden():
    g, meta = load_golden("loops_tiny")
    B, T, F_ = g["x_T"].shape
    synth = pkg("synth")

    def noises(tag, n):
        return [synth.uniform_pm1((B, T, F_), f"noise.{tag}.{i}", meta["iseed"]) * (3.0 ** 0.5) for i in range(n)]

    return g, meta, noises


# ---- pinned to the reference -------------------------------------------------------------------------------------------
def test_guided_ddpm_loop_matches_the_reference_goldens():
    g, meta, noises = _golden()
    assert meta["steps_cfg"] == 25
    d = S.make_diffusion("plain25")
    out = S.loop_ref(d, "cfg", meta["cfg_scale"], S.oracle_eps(g, meta), x_T=g["x_T"], step_noise=noises("cfg", 25),
                     **S.golden_text(g))
    for j, i in enumerate(g["cfg/traj_idx"].tolist()):
        e = rel_inf(out[i], g["cfg/traj"][j])
        print(f"[sampler_ref] guided DDPM-25 step {i}: rel_inf {e:.2e}")
        assert e < 2e-4, (i, e)
    e = rel_inf(out[24], g["cfg/final"])
    print(f"[sampler_ref] guided DDPM-25 final: rel_inf {e:.2e}")
    assert e < 2e-4, e


@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_clipped_ddim_loop_matches_the_reference_goldens(eta):
    """The reference records its DDIM loop with its default clip_denoised=True: x0 clamped before eps is re-derived."""
    g, meta, noises = _golden()
    assert meta["steps_ddim"] == 25
    d = S.make_diffusion("plain25")
    out = S.loop_ref(d, "ddim", 1.0, S.oracle_eps(g, meta), x_T=g["x_T"], eta=eta, step_noise=noises(f"ddim.{eta}", 25),
                     clip=True, **S.golden_text(g))
    e = rel_inf(out[24], g[f"ddim{eta}/final"])
    print(f"[sampler_ref] clipped DDIM-25 eta {eta} final: rel_inf {e:.2e}")
    assert e < 2e-4, e


# ---- pinned to the product's host table --------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", ["plain25", "ddim10", [4, 3, 3]])
def test_update_ref_is_the_products_coefficient_row(schedule):
    d = S.make_diffusion(schedule)
    acp, N = d.alphas_cumprod, d.num_timesteps
    gen = torch.Generator().manual_seed(N)
    x, x0, xp, z = (torch.randn(64, generator=gen, dtype=torch.float64) for _ in range(4))
    # (kind, eta, order, start): the rows walked and, per row, whether the step above it gave an x0
    cases = [("ddpm", 0.0, 2, None), ("ddim", 0.0, 2, None), ("ddim", 0.5, 2, None), ("dpmpp", 0.0, 1, None),
             ("dpmpp", 0.0, 2, None), ("dpmpp", 0.0, 2, N // 2), ("dpmpp", 0.0, 2, 1), ("ddim_inverse", 0.0, 2, None)]
    for kind, eta, order, start in cases:
        coef = d.solver_coefficients(kind, eta, order, start)
        top = N - 1 if start is None else start
        for t in (range(N - 1) if kind == "ddim_inverse" else range(top, -1, -1)):
            second = kind == "dpmpp" and order == 2 and t < top
            got = S.update_ref(kind, acp, t, x, x0, xp if second else None, eta, z)
            cx, c0, c1, cn = coef[t]
            terms = [cx * x, c0 * x0, c1 * xp, cn * z]
            assert second or c1 == 0.0, (kind, start, t)
            err = float((got - sum(terms)).abs().max())
            assert err <= 1e-9 * max(float(v.abs().max()) for v in terms), (kind, eta, order, start, t, err)


# ---- options -----------------------------------------------------------------------------------------------------------
def _stub_eps(x, t_orig, xf_proj, xf_out):
    """A cheap stand-in for the denoiser: depends on x, the timestep and the text, so a mixed-up argument shows."""
    return torch.tanh(0.3 * x + 1e-3 * t_orig) + xf_proj.double().mean(1)[:, None, None] + 0.1 * xf_out.double().mean()


def _inputs(n, shape, seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(shape, generator=gen) for _ in range(n)]


MODES = [("cfg", 0.0), ("ddim", 0.5), ("cfg_ddim", 0.5), ("cfg_dpmpp", 0.0)]


@pytest.mark.parametrize("mode,eta", MODES)
def test_check_gives_the_full_teacher_forced_run_at_those_steps(mode, eta):
    g, meta, noises = _golden()
    d = S.make_diffusion("ddim10")
    N = d.num_timesteps
    inp, ns = _inputs(N, g["x_T"].shape, 1), noises("opt", N)
    kw = dict(inputs=inp, eta=eta, step_noise=ns, **S.golden_text(g))
    full = S.loop_ref(d, mode, 2.5, _stub_eps, **kw)
    check = sorted({0, 1, N // 2, N - 2, N - 1})
    part = S.loop_ref(d, mode, 2.5, _stub_eps, check=check, **kw)
    assert sorted(full) == list(range(N)) and sorted(part) == check
    for i in check:
        assert torch.equal(part[i], full[i]), i
    free = S.loop_ref(d, mode, 2.5, _stub_eps, x_T=inp[0], eta=eta, step_noise=ns, **S.golden_text(g))
    assert torch.equal(free[0], full[0]) and not torch.equal(free[1], full[1])  # free-running carries its own x


@pytest.mark.parametrize("mode,eta", MODES)
def test_start_is_the_tail_of_a_run_with_shifted_inputs(mode, eta):
    g, meta, noises = _golden()
    d = S.make_diffusion([4, 3, 3])
    N, s = d.num_timesteps, 6
    inp, ns = _inputs(N, g["x_T"].shape, 2), noises("opt", N)
    off = N - 1 - s
    full = S.loop_ref(d, mode, 2.5, _stub_eps, inputs=inp, eta=eta, step_noise=ns, **S.golden_text(g))
    tail = S.loop_ref(d, mode, 2.5, _stub_eps, inputs=inp[off:], start=s, eta=eta, step_noise=ns[off:], **S.golden_text(g))
    assert sorted(tail) == list(range(s + 1))
    for i in range(s + 1):
        if mode == "cfg_dpmpp" and i == 0:  # the start step is first order although a row above it exists
            first = S.loop_ref(d, mode, 2.5, _stub_eps, inputs=inp, eta=eta, order=1, check=[off], **S.golden_text(g))
            assert torch.equal(tail[0], first[off]) and not torch.equal(tail[0], full[off])
        else:
            assert torch.equal(tail[i], full[i + off]), i


def test_inversion_walks_upwards_and_the_ddim_step_undoes_it():
    g, meta, _ = _golden()
    d = S.make_diffusion("ddim10")
    N = d.num_timesteps
    seen = []

    def const_eps(x, t_orig, xf_proj, xf_out):  # a constant eps: the deterministic DDIM step down is then the exact inverse
        seen.append(t_orig)
        return torch.full_like(x, 0.25)

    up = S.loop_ref(d, "ddim", 1.0, const_eps, x_T=g["x_T"], direction=+1, **S.golden_text(g))
    assert sorted(up) == list(range(N - 1)) and seen == [int(t) for t in d.timestep_map[:N - 1]]
    down = S.update_ref("ddim", d.alphas_cumprod, 1, up[0], S.x0_ref(d.alphas_cumprod[1], up[0], torch.full_like(up[0], 0.25)))
    # exact but for x0's a and b, which are f32 table entries (2^-24 relative each, in two x0's), seen through the eps
    # re-derived at level 0, which divides by sigma_0
    assert rel_inf(down, g["x_T"]) < 2 * 2.0 ** -24 / (1 - d.alphas_cumprod[0]) ** 0.5


def test_edit_mask_zero_is_no_edit_and_one_is_the_known_motion():
    g, meta, noises = _golden()
    d = S.make_diffusion("ddim10")
    N = d.num_timesteps
    inp = _inputs(N, g["x_T"].shape, 3)
    known = torch.randn(g["x_T"].shape, generator=torch.Generator().manual_seed(4)) * 1.5
    kw = dict(inputs=inp, **S.golden_text(g))
    plain = S.loop_ref(d, "cfg_dpmpp", 2.5, _stub_eps, **kw)
    zero = S.loop_ref(d, "cfg_dpmpp", 2.5, _stub_eps, known=known, mask=torch.zeros_like(known), **kw)
    one = S.loop_ref(d, "cfg_dpmpp", 2.5, _stub_eps, known=known, mask=torch.ones_like(known), **kw)
    assert all(torch.equal(zero[i], plain[i]) for i in range(N))
    assert torch.equal(one[N - 1], known.double())  # the last DPM-Solver++ step returns x0: the known motion, bit for bit
    x = inp[0].double()
    for clip in (False, True):
        x0 = S.x0_ref(d.alphas_cumprod[5], x, x * 0.5, x * 0.25, 2.5, clip=clip, known=known, mask=torch.ones_like(known))
        assert torch.equal(x0, known.double())


@pytest.mark.parametrize("clip", [False, True])
def test_one_prompt_of_unit_weight_is_cfg(clip):
    g, meta, noises = _golden()
    d = S.make_diffusion("plain25")
    N = d.num_timesteps
    inp, ns = _inputs(N, g["x_T"].shape, 5), noises("opt", N)
    text = S.golden_text(g)
    kw = dict(inputs=inp, step_noise=ns, clip=clip, check=[0, N // 2, N - 1])
    cfg = S.loop_ref(d, "cfg", 2.5, _stub_eps, **text, **kw)
    one = S.loop_ref(d, "cfg", 2.5, _stub_eps, weights=torch.ones(g["x_T"].shape[0], 1, *g["x_T"].shape[1:]), **text, **kw)
    assert all(torch.equal(one[i], cfg[i]) for i in cfg)
    if clip:  # the clamp sits on every x0 before the combination, not on the combined one
        x = inp[0].double() * 3
        x0 = S.x0_ref(d.alphas_cumprod[3], x, -x, x * 0.5, 2.5, clip=True)
        assert float(x0.abs().max()) > 1.0


def test_hooks_are_applied_where_their_doc_line_says():
    g, meta, noises = _golden()
    d = S.make_diffusion("plain25")
    N = d.num_timesteps
    inp, ns = _inputs(N, g["x_T"].shape, 6), noises("opt", N)
    kw = dict(inputs=inp, step_noise=ns, check=[3], **S.golden_text(g))
    calls = {"eps": 0, "noise": 0, "x0": 0}

    def count(name, f):
        def hook(v):
            calls[name] += 1
            return f(v)
        return hook

    plain = S.loop_ref(d, "cfg", 2.5, _stub_eps, **kw)
    same = S.loop_ref(d, "cfg", 2.5, _stub_eps, eps_hook=count("eps", lambda e: e), noise_hook=count("noise", lambda z: z),
                      x0_hook=count("x0", lambda v: v), **kw)
    assert calls == {"eps": 2, "noise": 1, "x0": 1} and torch.equal(same[3], plain[3])  # cond and uncond eps, one z, one x0
    zeroed = S.loop_ref(d, "cfg", 2.5, _stub_eps, noise_hook=lambda z: 0 * z, x0_hook=lambda v: 0 * v, **kw)
    ab, abp = d.alphas_cumprod[N - 4], d.alphas_cumprod[N - 5]
    want = (1 - abp) * (ab / abp) ** 0.5 / (1 - ab) * inp[3].double()  # x0 = 0, z = 0: the posterior's x_t term alone
    assert float((zeroed[3] - want).abs().max()) <= 1e-12 * float(want.abs().max())

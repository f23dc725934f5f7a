"""GPU: motion-to-motion generation: a given motion as the start of a partial loop, and DDIM inversion.

* mdm_diffuse_start against a * x + s * n in f64 with n from oracle/philox_ref.py (consecutive samples and explicit ids,
  per_sample % 4 != 0, pointers one float off 16-byte alignment, out aliasing x_start, given noise), under a derived gate;
  rows [0, 2) and [2, 4) with sample0 equal the 4-row call bit for bit;
* a partial loop is the tail of the full loop, bit for bit (x at level s from the full seeded loop's callback, given as
  ``noise=`` with ``start_step=s``), graph and eager, s at both ends and in the middle;
* every sampler from a noised motion against the loop restated in tests/sampler_ref.py from abar with the oracle's denoiser,
  teacher-forced on the device's trajectory; DPM-Solver++'s start step against the first-order formula;
* inversion: every step against the oracle's denoiser and the f64 update, the device clock at ``to_step`` afterwards, graph ==
  eager and two half batches == the whole, bitwise, unguided and guided;
* the trainer: strength 1 is the plain call and strength 0 the given motion, bitwise; the result does not depend on the batch
  split and equals generate_bucketed's; a binary edit mask's kept entries; init_joints; generate_long from a canvas.

Everything runs on the loops_tiny golden model (at B = 4, T = 16), the 25-step plain schedule and "ddim10" of 1000.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, pkg, rel_inf

import motion_features_ref as MR
import sampler_ref as S
from sampler_ref import caption_trainer as _trainer, make_diffusion as _diffusion, vp as _vp

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import philox_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu

XT = 0x7FFFFFFF  # MDM_NOISE_STREAM_XT


# ---- kernel level ------------------------------------------------------------------------------------------------------
def _start(x, noise, out, per, n, sample0, ids, seed, a, s):
    L = pkg("_lib")
    L.check(L.lib().mdm_diffuse_start(_vp(x), _vp(noise), _vp(out), per, n, sample0, _vp(ids), seed, a, s,
                                      C.c_void_p(L.stream_ptr())), "mdm_diffuse_start")


def _gate(got, x, nz, a, s, drawn):
    """|err| < s * 2e-6 + 4 * 2^-24 (|a x| + |s n|), elementwise: the first term is the gate tests/test_round2_gpu.py puts on
    the generator against the same oracle (it drops when the noise is given), the second the rounding of two products and a
    sum.  Returns the worst error as a fraction of its bound."""
    x, nz = x.double(), nz.double()
    want = a * x + s * nz
    bound = (abs(s) * 2e-6 if drawn else 0.0) + 4 * 2.0 ** -24 * ((a * x).abs() + (s * nz).abs())
    err = (got.double() - want).abs()
    assert bool(torch.isfinite(got).all())
    return float((err / bound.clamp_min(1e-300)).max())


@pytest.mark.parametrize("shape", [(3, 10, 263), (2, 16, 263)])
def test_start_kernel_matches_f64(shape):
    d = _diffusion("ddim10")
    n, per = shape[0], shape[1] * shape[2]
    seed, first = 0x1234_5678_9ABC, 7
    ids = [41, 3, 1 << 33][:n]
    gen = torch.Generator().manual_seed(per)
    x = torch.randn(shape, generator=gen) * 1.5
    given = torch.randn(shape, generator=gen)
    drawn = {"first": torch.from_numpy(P.normal(per, n, first, seed, XT)).view(shape),
             "ids": torch.from_numpy(np.concatenate([P.normal(per, 1, i, seed, XT) for i in ids])).view(shape)}
    ids_dev = torch.tensor(ids, dtype=torch.int64, device="cuda")
    for t in (0, 4, 9):  # sigma 0.01 ... ~1: the low level is where forming 1 - abar in f32 would cost digits
        a, s = float(np.float32(d.sqrt_alphas_cumprod[t])), float(np.float32(d.sqrt_one_minus_alphas_cumprod[t]))
        for off in (0, 1):  # 16-byte aligned (dwordx4 on the aligned rows) and one float off (element by element)
            bufs = [torch.zeros(x.numel() + off, device="cuda") for _ in range(3)]
            xi, ni, oi = (b[off:].view(shape) for b in bufs)
            xi.copy_(x), ni.copy_(given)
            for case in ("first", "ids", "given"):
                nz = given if case == "given" else drawn[case]
                oi.fill_(float("nan"))
                _start(xi, ni if case == "given" else None, oi, per, n, first if case == "first" else 0,
                       ids_dev if case == "ids" else None, seed, a, s)
                worst = _gate(oi.cpu(), x, nz, a, s, case != "given")
                assert worst < 1.0, (t, off, case, worst)
                assert torch.equal(xi.cpu(), x)  # the input is left alone
                alias = xi.clone() if off == 0 else torch.zeros(x.numel() + 1, device="cuda")[1:].view(shape).copy_(xi)
                _start(alias, ni if case == "given" else None, alias, per, n, first if case == "first" else 0,
                       ids_dev if case == "ids" else None, seed, a, s)
                assert torch.equal(alias, oi), (t, off, case)  # in place: the same bits
    # a = 0, s = 1 is the generator itself (fma(0, x, 1 * n) = n): what mdm_noise_normal writes, bit for bit
    L = pkg("_lib")
    out, ref = torch.empty(shape, device="cuda"), torch.empty(shape, device="cuda")
    _start(x.cuda(), None, out, per, n, first, None, seed, 0.0, 1.0)
    L.check(L.lib().mdm_noise_normal(_vp(ref), per, n, first, seed, None, XT, C.c_void_p(L.stream_ptr())))
    assert torch.equal(out, ref)


@pytest.mark.parametrize("shape", [(4, 10, 263), (4, 16, 263)])
def test_start_kernel_rows_do_not_depend_on_the_split(shape):
    per, seed, first = shape[1] * shape[2], 99, 5
    x = torch.randn(shape, generator=torch.Generator().manual_seed(1)).cuda()
    whole, parts = torch.empty_like(x), torch.empty_like(x)
    _start(x, None, whole, per, 4, first, None, seed, 0.8, 0.6)
    for lo in (0, 2):
        _start(x[lo:lo + 2], None, parts[lo:lo + 2], per, 2, first + lo, None, seed, 0.8, 0.6)
    assert torch.equal(whole, parts)
    ids = torch.tensor([first + 1, first], dtype=torch.int64, device="cuda")  # explicit ids: the same samples, reordered
    two = torch.empty_like(x[:2])
    _start(x[[1, 0]].contiguous(), None, two, per, 2, 0, ids, seed, 0.8, 0.6)
    assert torch.equal(two, whole[[1, 0]])


# ---- loops -------------------------------------------------------------------------------------------------------------
def _setup():
    g, meta, m, _, _ = S.loops_setup()
    synth = pkg("synth")
    B, T, F_ = 4, 16, g["x_T"].shape[2]  # the golden's model at four rows, so that a batch splits into halves
    _, _, length, xf_proj, xf_out = synth.synth_inputs(B, T, F_, 6, meta["text_latent_dim"], 9, min_len=4)
    g = dict(g, length=length, xf_proj=xf_proj, xf_out=xf_out)
    kw = {"xf_proj": g["xf_proj"].cuda(), "xf_out": g["xf_out"].cuda(), "length": g["length"].cuda(),
          "text": ["a person walks"] * B}
    init = synth.uniform_pm1((B, T, F_), "start.init", meta["iseed"]) * 1.5
    return g, meta, m, kw, init


def _loop(d, mode, m, kw, scale, eta, use_graph, cb=None, **more):
    return S.run_loop(d, mode, m, kw, scale, eta, use_graph, cb=cb, shape=(kw["xf_out"].shape[0], 16, 263), **more)


@pytest.mark.parametrize("mode,eta,schedule", [("cfg", 0.0, "plain25"), ("cfg_ddim", 0.0, "ddim10"), ("cfg_ddim", 0.5, "ddim10")])
def test_a_partial_loop_is_the_tail_of_the_full_loop(mode, eta, schedule):
    """x at level s of the full seeded loop, given as ``noise=`` with ``start_step=s``, ends where the full loop ends, bit for
    bit: the step noise is keyed on the timestep, not on the count of steps run."""
    g, meta, m, kw, _ = _setup()
    d = _diffusion(schedule)
    N, scale = d.num_timesteps, meta["cfg_scale"]
    level = {}  # x at level t - 1 after step t
    full = _loop(d, mode, m, kw, scale, eta, True, cb=lambda i, t, x: level.__setitem__(t - 1, x.clone()), seed=11)
    assert sorted(level) == list(range(-1, N - 1)) and torch.equal(level[-1], full)
    for use_graph in (True, False):
        for s in (0, N // 2, N - 2):
            seen = []
            out = _loop(d, mode, m, kw, scale, eta, use_graph, cb=lambda i, t, x: seen.append((i, t)), seed=11,
                        noise=level[s], start_step=s)
            assert seen == [(i, s - i) for i in range(s + 1)], (use_graph, s)
            assert torch.equal(out, full), (use_graph, s)
    with pytest.raises(NotImplementedError):
        _loop(d, mode, m, kw, scale, eta, True, seed=11, noise=level[0], start_step=torch.tensor([0, 1, 0, 0]))
    with pytest.raises(ValueError):
        _loop(d, mode, m, kw, scale, eta, True, seed=11, start_step=3)


@pytest.mark.parametrize("mode,eta,schedule", [("cfg", 0.0, "plain25"), ("cfg_ddim", 0.5, "ddim10"), ("cfg_dpmpp", 0.0, "ddim10"),
                                               ("cfg_dpmpp", 0.0, "plain25")])
def test_samplers_from_a_noised_motion_match_the_oracle(mode, eta, schedule):
    """From ``init_motion`` at ``start_step`` N // 2: the start is a x + s n with the oracle's generator, and every step
    agrees with the loop restated from abar (teacher-forced: each step from the device's x).  DPM-Solver++'s first step is
    first order, D = x0, although a step above it exists in the schedule."""
    g, meta, m, kw, init = _setup()
    d = _diffusion(schedule)
    N, scale, seed = d.num_timesteps, meta["cfg_scale"], 23
    B, T, F_ = init.shape
    s = N // 2
    acp = d.alphas_cumprod
    nz = torch.from_numpy(P.normal(T * F_, B, 0, seed, XT)).view(B, T, F_).double()
    x_s = acp[s] ** 0.5 * init.double() + (1 - acp[s]) ** 0.5 * nz
    got = []
    out = _loop(d, mode, m, kw, scale, eta, True, cb=lambda i, t, x: got.append(x.clone().cpu()), seed=seed,
                init_motion=init.cuda(), start_step=s).cpu()
    assert len(got) == s + 1 and torch.equal(out, got[-1])
    eager = _loop(d, mode, m, kw, scale, eta, False, seed=seed, init_motion=init.cuda(), start_step=s).cpu()
    assert torch.equal(eager, out)
    # second order needs the x0 of the step before: ``check`` recomputes it from that step's input; the step noise is keyed on t
    steps = sorted({0, 1, s // 2, s - 1, s})
    zs = {i: torch.from_numpy(P.normal(T * F_, B, 0, seed, s - i)).view(B, T, F_) for i in steps}
    want = S.loop_ref(d, mode, scale, S.oracle_eps(g, meta), inputs=[x_s.float()] + got[:-1], check=steps, start=s, eta=eta,
                      step_noise=zs, **S.golden_text(g))
    for i in steps:
        e = rel_inf(got[i], want[i])
        print(f"[start] {mode} eta {eta} {schedule}: step {i} (t = {s - i}) rel_inf {e:.2e}")
        assert e < 1e-3, (i, e)
    if mode == "cfg_dpmpp":  # and the second-order formula at the start step is NOT what ran
        assert s < N - 1 and d.solver_coefficients("dpmpp")[s, 2] != 0.0
    # the noise may be given instead of drawn, and without either it comes from the torch generator
    first = []
    _loop(d, mode, m, kw, scale, eta, True, cb=lambda i, t, x: first.append(x.clone().cpu()), seed=seed, init_motion=init.cuda(),
          start_step=s, noise=nz.float().cuda())
    assert rel_inf(first[0], got[0]) < 1e-3  # the oracle's draw given as noise: the same first step
    torch.manual_seed(5)
    a = _loop(d, mode, m, kw, scale, eta, True, init_motion=init.cuda(), start_step=s)
    torch.manual_seed(5)
    b = _loop(d, mode, m, kw, scale, eta, True, init_motion=init.cuda(), start_step=s)
    assert torch.equal(a, b) and not torch.equal(a.cpu(), out)


# ---- inversion -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 2.5])
def test_inversion(scale):
    g, meta, m, kw, init = _setup()
    d = _diffusion("ddim10")
    N = d.num_timesteps
    B, T, F_ = init.shape
    mode = "ddim" if scale == 1.0 else "cfg_ddim"
    runs = {}
    for use_graph in (True, False):
        got = []
        r = d._runner(m, (B, T, F_), kw, "cuda", mode, scale, 0.0, False, use_graph, start_step=N - 1, direction=+1)
        assert r.R == (B if scale == 1.0 else 2 * B)  # the caption alone, or the guided 2B form
        out = r.run(init.cuda(), None, False, lambda i, t, x: got.append((i, t, x.clone().cpu()))).cpu()
        assert int(r.t_dev) == N - 1  # the device clock ends at to_step
        assert [(i, t) for i, t, _ in got] == [(i, i) for i in range(N - 1)] and torch.equal(out, got[-1][2])
        runs[use_graph] = [x for _, _, x in got]
    assert all(torch.equal(a, b) for a, b in zip(runs[True], runs[False]))  # graph == eager
    want = S.loop_ref(d, mode, scale, S.oracle_eps(g, meta), inputs=[init] + runs[True][:-1], direction=+1, **S.golden_text(g))
    for t in range(N - 1):  # every step: row t takes level t to level t + 1
        e = rel_inf(runs[True][t], want[t])
        print(f"[invert] scale {scale}: row {t} rel_inf {e:.2e}")
        assert e < 1e-3, (t, e)
    # the public loop, to the last step and to a step on the way
    pub = d.ddim_invert_loop(m, init.cuda(), kw, cfg_scale=scale).cpu()
    assert torch.equal(pub, runs[True][-1])
    mid = d.ddim_invert_loop(m, init.cuda(), kw, to_step=4, cfg_scale=scale).cpu()
    assert torch.equal(mid, runs[True][3])
    assert torch.equal(d.ddim_invert_loop(m, init.cuda(), kw, to_step=0, cfg_scale=scale).cpu(), init)
    # two half batches equal the whole
    halves = []
    for lo in (0, 2):
        hkw = {k: v[lo:lo + 2] for k, v in kw.items()}
        halves.append(d.ddim_invert_loop(m, init[lo:lo + 2].cuda(), hkw, cfg_scale=scale).cpu())
    assert torch.equal(torch.cat(halves), pub)
    # the latents regenerate through the DDIM loop from their level (the figure is a record: random weights have no smooth ODE)
    back = d.ddim_sample_loop_with_cfg(m, (B, T, F_), noise=pub.cuda(), start_step=N - 1, clip_denoised=False, model_kwargs=kw,
                                       cfg_scale=scale).cpu()
    print(f"[invert] scale {scale}: round trip rel_inf {rel_inf(back, init):.3e}")
    assert torch.isfinite(back).all()


# ---- trainer -----------------------------------------------------------------------------------------------------------
CAPS = ["a", "b", "c", "d"]


def test_the_ends_of_the_strength():
    g, meta, m, kw, init = _setup()
    tr = _trainer(m, meta)
    lens = torch.tensor([16, 12, 16, 8])
    for sampler in ("ddim", "dpmpp2m", "ddpm"):
        opts = dict(batch_size=2, seed=3, sampler=sampler, sample_steps=10)
        plain = tr.generate(CAPS, lens, 263, **opts)
        one = tr.generate(CAPS, lens, 263, init_motion=init, strength=1.0, **opts)
        assert all(torch.equal(a, b) for a, b in zip(plain, one)), sampler
        zero = tr.generate(CAPS, lens, 263, init_motion=init, strength=0.0, **opts)
        assert all(torch.equal(z.cpu(), init[i]) for i, z in enumerate(zero)), sampler
        assert all(z.is_cuda for z in zero)
        half = tr.generate(CAPS, lens, 263, init_motion=init, strength=0.5, **opts)
        assert not any(torch.equal(a, b) for a, b in zip(plain, half)) and all(torch.isfinite(h).all() for h in half)
    with pytest.raises(ValueError):
        tr.generate(CAPS, lens, 263, init_motion=init[:, :12], strength=0.5, batch_size=2, seed=3, sampler="ddim", sample_steps=10)


def test_trainer_start_is_independent_of_the_batch_split():
    g, meta, m, kw, init = _setup()
    tr = _trainer(m, meta)
    lens = torch.tensor([16, 12, 16, 8])
    for sampler, extra in (("dpmpp2m", {}), ("ddim", dict(eta=0.5)), ("ddpm", {})):
        opts = dict(seed=3, sampler=sampler, sample_steps=10, init_motion=init, strength=0.5, **extra)
        by = {bs: tr.generate(CAPS, lens, 263, batch_size=bs, **opts) for bs in (2, 4)}
        bucket = tr.generate_bucketed(CAPS, lens, 263, batch_size=2, unit_length=4, **opts)
        for i, n in enumerate(lens.tolist()):
            for name, other in (("batch 4", by[4][i]), ("bucketed", bucket[i])):
                e = rel_inf(other[:n].cpu(), by[2][i][:n].cpu())
                print(f"[start] {sampler} sample {i} ({n} frames) {name} vs batch 2: rel_inf {e:.2e}")
                assert torch.equal(other[:n], by[2][i][:n]), (sampler, i, name, e)
    other = tr.generate(CAPS, lens, 263, batch_size=2, **dict(opts, seed=4))
    assert not torch.equal(other[1], by[2][1])


def test_start_composes_with_a_binary_edit_mask():
    g, meta, m, kw, init = _setup()
    E = pkg("motion_edit")
    synth = pkg("synth")
    tr = _trainer(m, meta)
    same = torch.tensor([16, 16, 16, 16])
    k = synth.uniform_pm1((4, 16, 263), "start.edit", 3).cuda()
    for sampler in ("ddim", "dpmpp2m", "ddpm"):
        for mask in (E.prefix_mask(16, 4), E.joint_feature_mask(E.UPPER_BODY)):
            out = torch.stack(tr.generate(CAPS, same, 263, batch_size=2, seed=3, sampler=sampler, sample_steps=10,
                                          init_motion=init, strength=0.5, edit_motion=k, edit_mask=mask))
            keep = torch.broadcast_to(mask.cuda(), k.shape) == 1
            assert torch.equal(out[keep], k[keep]), sampler
            assert not torch.equal(out[~keep], k[~keep]) and bool(torch.isfinite(out).all())


def test_init_joints_are_the_rows_joints_to_motion_makes_of_them():
    g, meta, m, kw, _ = _setup()
    MF = pkg("motion_features")
    tr = _trainer(m, meta)
    sk = MF.SKELETONS["t2m"]
    ref = MR.skeleton_from_tables(sk.chains, sk.raw_offsets, sk.face, sk.feet, sk.legs)
    lens = torch.tensor([16, 12, 16, 8])
    clips = [torch.from_numpy(MR.synth_clip(ref, n, 700 + i)).float() for i, n in enumerate((17, 13, 20, 9))]
    gen = torch.Generator().manual_seed(2)
    mean, std = (torch.randn(263, generator=gen) * 0.1).numpy(), (0.5 + torch.rand(263, generator=gen)).numpy()
    rows = MF.joints_to_motion([c.cuda() for c in clips], None, mean, std)
    assert tuple(rows.shape) == (4, 19, 263)
    opts = dict(batch_size=2, seed=3, sampler="dpmpp2m", sample_steps=10, strength=0.5)
    a = tr.generate(CAPS, lens, 263, init_joints=clips, mean=mean, std=std, **opts)
    b = tr.generate(CAPS, lens, 263, init_motion=rows, **opts)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    short = clips[:3] + [clips[3][:8]]  # 7 rows for a sample of 8 frames
    with pytest.raises(ValueError, match="shorter"):
        tr.generate(CAPS, lens, 263, init_joints=short, mean=mean, std=std, **opts)
    with pytest.raises(ValueError, match="mean and std"):
        tr.generate(CAPS, lens, 263, init_joints=clips, **opts)


def test_invert_then_generate_from_the_latents():
    g, meta, m, kw, init = _setup()
    tr = _trainer(m, meta)
    tr.cfg_scale = 1.0
    lens = torch.tensor([16, 12, 16, 8])
    lat, step = tr.invert(CAPS, init, lens, 263, sample_steps=10, batch_size=2)
    assert int(step) == 9 and step.sample_steps == 10 and [tuple(v.shape) for v in lat] == [(16, 263)] * 4
    whole, step4 = tr.invert(CAPS, init, lens, 263, sample_steps=10, batch_size=4, to_strength=0.5)
    assert int(step4) == 4
    d = tr.sampling_diffusion("ddim", 10)
    for cur in (0, 2):  # what the loop gives for the batch's rows, bit for bit
        want = d.ddim_invert_loop(m, init[cur:cur + 2].cuda(), {"text": CAPS[cur:cur + 2], "length": lens[cur:cur + 2]})
        assert torch.equal(torch.stack(lat[cur:cur + 2]), want)
    back = tr.generate(CAPS, lens, 263, batch_size=2, sampler="ddim", sample_steps=10, latents=lat, latent_step=step)
    want = d.ddim_sample_loop_with_cfg(m, (2, 16, 263), noise=torch.stack(lat[:2]), start_step=9, clip_denoised=False,
                                       model_kwargs={"text": CAPS[:2], "length": lens[:2]}, cfg_scale=1.0)
    assert torch.equal(torch.stack(back[:2]), want)
    for i, n in enumerate(lens.tolist()):
        print(f"[invert] trainer round trip sample {i}: rel_inf {rel_inf(back[i][:n].cpu(), init[i, :n]):.3e}")
    with pytest.raises(ValueError, match="ddim"):
        tr.generate(CAPS, lens, 263, batch_size=2, sampler="dpmpp2m", sample_steps=10, latents=lat, latent_step=step)
    with pytest.raises(ValueError, match="sample_steps"):
        tr.generate(CAPS, lens, 263, batch_size=2, sampler="ddim", sample_steps=20, latents=lat, latent_step=step)
    with pytest.raises(ValueError):
        tr.invert(CAPS, init, lens, 263, sample_steps=10, to_strength=0.0)


LENS, H = [16, 12, 16], 4


def test_generate_long_from_a_canvas():
    """Three windows of 16 / 12 / 16 frames at h = 4 over a 36-frame canvas: each window starts from its frames of the
    noised canvas, the overlaps from their owner window's, and neighbouring windows agree bit for bit on their shared frames
    after every step."""
    g, meta, m, kw, _ = _setup()
    ML = pkg("motion_long")
    synth = pkg("synth")
    starts, Cn = ML.plan_windows(LENS, H)
    assert Cn == 36
    t = ML.handshake_tables(starts, LENS, 16, H, "linear")
    hk = {"handshake_offsets": torch.from_numpy(t["offsets"]), "handshake_rows": torch.from_numpy(t["rows"]),
          "handshake_weights": torch.from_numpy(t["weights"]), "handshake_owner_rows": torch.from_numpy(t["owner_rows"])}
    canvas = synth.uniform_pm1((Cn, 263), "start.canvas", meta["iseed"]) * 1.5
    rows = ML.canvas_to_windows(canvas, starts, LENS, 16)
    sel = [0, 1, 0]
    lkw = dict({"xf_proj": g["xf_proj"][sel].cuda(), "xf_out": g["xf_out"][sel].cuda(), "length": torch.tensor(LENS).cuda(),
                "text": ["a", "b", "a"]}, **hk)

    def shared(x):
        return all(torch.equal(x[i, LENS[i] - H:LENS[i]], x[i + 1, :H]) for i in range(len(LENS) - 1))

    d = _diffusion("ddim10")
    for mode, eta in (("cfg", 0.0), ("cfg_ddim", 0.5), ("cfg_dpmpp", 0.0)):
        got = []
        out = _loop(d, mode, m, lkw, meta["cfg_scale"], eta, True, cb=lambda i, t, x: got.append(x.clone()), seed=9,
                    init_motion=rows.cuda(), start_step=4)
        assert len(got) == 5 and all(shared(x) for x in got) and shared(out), mode
        assert bool(torch.isfinite(out).all())
        free = _loop(d, mode, m, {k: v for k, v in lkw.items() if k not in hk}, meta["cfg_scale"], eta, True, seed=9,
                     init_motion=rows.cuda(), start_step=4)
        assert not shared(free)  # without the handshakes the windows disagree: their noise differs
    tr = _trainer(m, meta)
    script = [[("walk", 16), ("turn", 12), ("sit", 16)]]
    opts = dict(overlap=H, seed=9, sampler="dpmpp2m", sample_steps=10)
    plain = tr.generate_long(script, 263, **opts)[0]
    assert torch.equal(tr.generate_long(script, 263, init_motion=[canvas], strength=1.0, **opts)[0], plain)
    assert torch.equal(tr.generate_long(script, 263, init_motion=[canvas], strength=0.0, **opts)[0].cpu(), canvas)
    half = tr.generate_long(script, 263, init_motion=[canvas], strength=0.5, **opts)[0]
    assert tuple(half.shape) == (36, 263) and bool(torch.isfinite(half).all()) and not torch.equal(half, plain)
    near = tr.generate_long(script, 263, init_motion=[canvas], strength=0.1, **opts)[0].cpu()
    assert (near - canvas).abs().mean() < (half.cpu() - canvas).abs().mean()  # fewer steps stay nearer the motion
    with pytest.raises(ValueError):
        tr.generate_long(script, 263, init_motion=[canvas], **opts)
    with pytest.raises(ValueError):
        tr.generate_long(script, 263, init_motion=[canvas[:30]], strength=0.5, **opts)

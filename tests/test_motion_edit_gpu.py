"""GPU: motion editing (x0 replaced by (1 - m) x0 + m k on every step of every sampler).

* mdm_guided_update_inpaint against an f64 restatement (masks 0 / 1 / fractional, guided or not, with and without noise,
  aligned and misaligned buffers, n % 4 != 0), and bitwise equal to mdm_guided_update under an all-zero mask;
* all-zero masks leave the loops unchanged (bitwise for the few-step loops, within rounding for DDPM, whose update is
  associated differently);
* every loop against the oracle's denoiser with the loop restated in tests/sampler_ref.py from abar (not from the product's
  tables), teacher-forced on the device's trajectory, on the loops_tiny golden, under prefix, in-between and body-part masks,
  graph and eager; a binary mask's kept entries come out bit for bit;
* graph == eager and two streams == one bitwise, progressive loops and single steps, the trainer's result independent of
  the batch split, the feature layout under recover_from_ric, and the configs[1] shape in bf16.
"""
import types

import pytest
import torch

from conftest import pkg, rel_inf

import sampler_ref as S
from sampler_ref import KIND, caption_trainer as _trainer, make_diffusion as _diffusion

pytestmark = pytest.mark.gpu


# ---- kernel level ------------------------------------------------------------------------------------------------------
def test_inpaint_update_kernel_matches_f64_and_the_plain_kernel():
    d = _diffusion("ddim10")
    N = d.num_timesteps
    gen = torch.Generator().manual_seed(2)
    shape = (3, 10, 263)  # n = 7890: not a multiple of 4, the last quad takes the element-wise tail
    x, ec, eu, xp, nz, kn = (torch.randn(shape, generator=gen).cuda() for _ in range(6))
    frac = torch.rand(shape, generator=gen)
    frac[0, :3] = 0.0
    frac[1, :3] = 1.0
    masks = {"zero": torch.zeros(shape).cuda(), "one": torch.ones(shape).cuda(), "frac": frac.cuda()}
    tab = d._device_table("cuda")
    for kind, eta in (("ddpm", 0.0), ("ddim", 0.5), ("dpmpp", 0.0)):
        coef, coef64 = d._device_coef(kind, eta, 2, "cuda"), d.solver_coefficients(kind, eta, 2)
        for t in (N - 1, N // 2, 0):
            for clip in (0, 1):
                for eu_ in (eu, None):
                    for nz_ in (nz, None):
                        xp_ = xp if kind == "dpmpp" else None
                        for name, mk in masks.items():
                            xo, x0o = torch.empty(shape, device="cuda"), torch.empty(shape, device="cuda")
                            S.guided_update(x, ec, eu_, xp_, nz_, kn, mk, tab, coef, N, t, 2.5, clip, xo, x0o)
                            ref, ref0 = S.update_kernel_ref(
                                d, coef64, t, x.cpu(), ec.cpu(), None if eu_ is None else eu_.cpu(),
                                None if xp_ is None else xp_.cpu(), None if nz_ is None else nz_.cpu(), kn.cpu(), mk.cpu(), 2.5,
                                clip)
                            case = (kind, t, clip, eu_ is None, nz_ is None, name)
                            e = rel_inf(xo.cpu(), ref)
                            # x0 = a*x - b*eps cancels terms of ~a*|x|: its f32 error is measured against their size
                            den = max(float(ref0.abs().max()), float(d.sqrt_recip_alphas_cumprod[t] * x.abs().max()))
                            e0 = float((x0o.cpu().double() - ref0).abs().max()) / den
                            assert e < 1e-5 and e0 < 1e-5, (case, e, e0)
                            if name == "one":
                                assert torch.equal(x0o, kn), case
                            if name == "frac":
                                assert torch.equal(x0o[1, :3], kn[1, :3]), case
                            if name == "zero":  # the masked entry point with nothing masked is the plain kernel, bit for bit
                                po, p0 = torch.empty(shape, device="cuda"), torch.empty(shape, device="cuda")
                                S.guided_update(x, ec, eu_, xp_, nz_, None, None, tab, coef, N, t, 2.5, clip, po, p0)
                                assert torch.equal(xo, po) and torch.equal(x0o, p0), case
    # in place (x_out = x, x0_out = x0_prev) on buffers that are not 16-byte aligned (the element-wise form), and aligned
    coef, coef64 = d._device_coef("dpmpp", 0.0, 2, "cuda"), d.solver_coefficients("dpmpp", 0.0, 2)
    t = N // 2
    ref, ref0 = S.update_kernel_ref(d, coef64, t, x.cpu(), ec.cpu(), eu.cpu(), xp.cpu(), None, kn.cpu(), frac, 2.5, False)
    for off in (1, 0):
        bufs = [torch.zeros(x.numel() + off, device="cuda") for _ in range(4)]
        xi, pi, ki, mi = (b[off:].view(shape) for b in bufs)
        xi.copy_(x), pi.copy_(xp), ki.copy_(kn), mi.copy_(frac.cuda())
        S.guided_update(xi, ec, eu, pi, None, ki, mi, tab, coef, N, t, 2.5, 0, xi, pi)
        assert rel_inf(xi.cpu(), ref) < 1e-5 and rel_inf(pi.cpu(), ref0) < 1e-5, off
        assert torch.equal(pi[1, :3], kn[1, :3]), off


# ---- loops -------------------------------------------------------------------------------------------------------------
def _setup():
    g, meta, m, noises, kw = S.loops_setup()
    # beyond [-1, 1]: k is never clamped
    known = pkg("synth").uniform_pm1(tuple(g["x_T"].shape), "edit.known", meta["iseed"]) * 1.5
    return g, meta, m, noises, kw, known


def _mask(kind, B, T, F_):
    E = pkg("motion_edit")
    m = {"prefix": E.prefix_mask(T, 5), "inbetween": E.inbetween_mask(T, 3, 4), "zero": torch.zeros(T, 1),
         "body": E.joint_feature_mask(E.LOWER_BODY)}[kind]
    return torch.broadcast_to(m, (B, T, F_))


SOLVERS = [("cfg", 0.0), ("ddpm", 0.0), ("cfg_ddim", 0.0), ("cfg_ddim", 0.5), ("ddim", 0.0), ("ddim", 0.5),
           ("cfg_dpmpp", 0.0)]


@pytest.mark.parametrize("mask_kind", ["prefix", "inbetween", "body"])
@pytest.mark.parametrize("schedule", ["plain25", "ddim10", "4,3,3"])
@pytest.mark.parametrize("mode,eta", SOLVERS)
def test_edited_loops_match_the_oracle(mode, eta, schedule, mask_kind):
    g, meta, m, noises, kw, known = _setup()
    d = _diffusion([4, 3, 3] if schedule == "4,3,3" else schedule)
    N, scale = d.num_timesteps, meta["cfg_scale"]
    B, T, F_ = g["x_T"].shape
    mask = _mask(mask_kind, B, T, F_)
    ns = noises(f"edit.{mode}.{eta}", N)
    ekw = dict(kw, inpaint_motion=known.cuda(), inpaint_mask=mask.cuda())
    finals = []
    for use_graph in (True, False):
        got = []
        out = S.run_loop(d, mode, m, ekw, scale, eta, use_graph, x_T=g["x_T"].cuda(), step_noise=ns,
                         cb=lambda i, t, x: got.append(x.clone().cpu())).cpu()
        assert len(got) == N and torch.equal(out, got[-1])
        if use_graph:  # the eager run must reproduce it bitwise (below), so the oracle runs once
            want = S.loop_ref(d, mode, scale, S.oracle_eps(g, meta), inputs=[g["x_T"]] + got[:-1], eta=eta, step_noise=ns,
                              known=known, mask=mask, **S.golden_text(g))
            for i in sorted({0, 1, N // 2, N - 2, N - 1}):
                e = rel_inf(got[i], want[i])
                assert e < 1e-3, (i, e)
        keep = mask == 1
        assert torch.equal(out[keep], known[keep]), use_graph  # the kept entries are the known motion, bit for bit
        assert not torch.equal(out[~keep], known[~keep])
        finals.append(out)
    assert torch.equal(finals[0], finals[1])


@pytest.mark.parametrize("mode,eta", SOLVERS)
def test_an_all_zero_mask_changes_nothing(mode, eta):
    g, meta, m, noises, kw, known = _setup()
    d = _diffusion("plain25" if KIND[mode] == "ddpm" else "ddim10")
    B, T, F_ = g["x_T"].shape
    ns = noises("zero", d.num_timesteps)
    ekw = dict(kw, inpaint_motion=known.cuda(), inpaint_mask=_mask("zero", B, T, F_).cuda())
    plain = S.run_loop(d, mode, m, kw, meta["cfg_scale"], eta, True, x_T=g["x_T"].cuda(), step_noise=ns).cpu()
    edited = S.run_loop(d, mode, m, ekw, meta["cfg_scale"], eta, True, x_T=g["x_T"].cuda(), step_noise=ns).cpu()
    e = rel_inf(edited, plain)
    print(f"[zero mask] {mode} eta {eta}: rel_inf {e:.3e}")
    if mode in ("cfg_ddim", "cfg_dpmpp"):  # the same fused kernel's plain and masked instantiations
        assert torch.equal(edited, plain)
        return
    # mdm_ddim_step derives its coefficients on the device in f32; the DDPM kernel takes its noise scale from expf, the
    # "ddpm" table from an f64 exp.  One step differs by rounding; over a loop it accumulates through the forwards.
    assert e <= 1e-5, e
    t = torch.full((B,), d.num_timesteps - 1, dtype=torch.int64, device="cuda")
    x_t, z = g["x_T"].cuda(), ns[0].cuda()

    def step(k):
        if mode == "cfg":
            return d.p_sample_with_cfg(m, x_t, t, clip_denoised=False, model_kwargs=k, cfg_scale=meta["cfg_scale"], noise=z)
        if mode == "ddpm":
            return d.p_sample(m, x_t, t, clip_denoised=False, model_kwargs=k, noise=z)
        return d.ddim_sample(m, x_t, t, clip_denoised=False, model_kwargs=k, eta=eta, noise=z)

    one, ref = step(ekw)["sample"].cpu(), step(kw)["sample"].cpu()
    e1 = rel_inf(one, ref)
    print(f"[zero mask] {mode} eta {eta}: one step rel_inf {e1:.3e}")
    assert e1 <= 1e-6, e1


@pytest.mark.parametrize("mode,eta", [("cfg", 0.0), ("cfg_ddim", 0.5), ("cfg_dpmpp", 0.0)])
def test_graph_equals_eager_and_two_streams_equal_one_bitwise(mode, eta):
    g, meta, m, noises, kw, known = _setup()
    d = _diffusion([4, 3, 3])
    B, T, F_ = g["x_T"].shape
    ekw = dict(kw, inpaint_motion=known.cuda(), inpaint_mask=_mask("inbetween", B, T, F_).cuda())
    outs = {}
    for use_graph, streams in ((True, 1), (False, 1), (True, 2)):
        r = d._runner(m, (B, T, F_), ekw, "cuda", mode, meta["cfg_scale"], eta, False, use_graph, streams)
        outs[(use_graph, streams)] = r.run(g["x_T"].cuda(), None, False, None, seed=11).cpu()
    assert torch.isfinite(outs[(True, 1)]).all()
    assert torch.equal(outs[(True, 1)], outs[(False, 1)])
    assert torch.equal(outs[(True, 1)], outs[(True, 2)])


def test_progressive_loops_and_single_steps_edit_x0():
    g, meta, m, noises, kw, known = _setup()
    d = _diffusion("ddim10")
    B, T, F_ = g["x_T"].shape
    mask = _mask("prefix", B, T, F_)
    keep = mask == 1
    ekw = dict(kw, inpaint_motion=known.cuda(), inpaint_mask=mask.cuda())
    ns = noises("prog", d.num_timesteps)
    for gen_fn, extra in ((d.p_sample_loop_progressive, {}), (d.ddim_sample_loop_progressive, {"eta": 0.5})):
        steps = list(gen_fn(m, (B, T, F_), noise=g["x_T"].cuda(), clip_denoised=False, model_kwargs=ekw, step_noise=ns,
                            **extra))
        loop = (d.p_sample_loop if not extra else d.ddim_sample_loop)(
            m, (B, T, F_), noise=g["x_T"].cuda(), clip_denoised=False, model_kwargs=ekw, step_noise=ns, use_graph=False,
            **extra).cpu()
        assert torch.equal(steps[-1]["sample"].cpu(), loop)
        for s in steps:  # pred_xstart is the edited x0 on every step
            assert torch.equal(s["pred_xstart"].cpu()[keep], known[keep])
        assert torch.equal(loop[keep], known[keep])
    x_t = g["x_T"].cuda()
    t = torch.full((B,), d.num_timesteps - 1, dtype=torch.int64, device="cuda")
    sc = meta["cfg_scale"]
    for step in (lambda: d.p_sample_with_cfg(m, x_t, t, clip_denoised=False, model_kwargs=ekw, cfg_scale=sc,
                                             noise=ns[0].cuda()),
                 lambda: d.ddim_sample_with_cfg(m, x_t, t, clip_denoised=False, model_kwargs=ekw, cfg_scale=sc, eta=0.5,
                                                noise=ns[0].cuda()),
                 lambda: d.ddim_sample(m, x_t, t, clip_denoised=False, model_kwargs=ekw, eta=0.0),
                 lambda: d.p_sample(m, x_t, t, clip_denoised=False, model_kwargs=ekw, noise=ns[0].cuda())):
        out = step()
        assert torch.equal(out["pred_xstart"].cpu()[keep], known[keep])
        assert not torch.equal(out["pred_xstart"].cpu()[~keep], known[~keep])
    with pytest.raises(ValueError):
        d.ddim_sample(m, x_t, t, clip_denoised=False, model_kwargs=dict(kw, inpaint_motion=known.cuda()))


# ---- trainer -----------------------------------------------------------------------------------------------------------
def test_trainer_edit_is_independent_of_the_batch_split():
    g, meta, m, noises, kw, known = _setup()
    E = pkg("motion_edit")
    tr = _trainer(m, meta)
    caps = ["a", "b", "c", "d"]
    synth = pkg("synth")
    k = synth.uniform_pm1((4, 16, 263), "edit.trainer", 3).cuda()
    mask = E.prefix_mask(16, 4)
    opts = dict(seed=3, sampler="ddim", sample_steps=10, eta=0.5, edit_motion=k, edit_mask=mask)
    same = torch.tensor([16, 16, 16, 16])
    one = torch.stack(tr.generate(caps, same, 263, batch_size=1, **opts)).cpu()
    two = torch.stack(tr.generate(caps, same, 263, batch_size=2, **opts)).cpu()
    assert torch.isfinite(one).all() and rel_inf(one, two) < 1e-5, rel_inf(one, two)
    assert torch.equal(one[:, :4], k[:, :4].cpu()) and torch.equal(two[:, :4], k[:, :4].cpu())
    plain = torch.stack(tr.generate(caps, same, 263, batch_size=2, seed=3, sampler="ddim", sample_steps=10,
                                    eta=0.5)).cpu()
    assert not torch.equal(plain[:, 4:], one[:, 4:])  # the kept frames steer the generated ones
    lens = torch.tensor([8, 16, 12, 4])
    for extra in (dict(opts), dict(opts, sampler="dpmpp2m", eta=0.0, edit_mask=E.joint_feature_mask(E.UPPER_BODY))):
        serial = tr.generate(caps, lens, 263, batch_size=2, **extra)
        bucket = tr.generate_bucketed(caps, lens, 263, batch_size=2, unit_length=4, **extra)
        full = torch.broadcast_to(extra["edit_mask"].cuda(), k.shape) == 1
        for i, n in enumerate(lens.tolist()):
            e = rel_inf(bucket[i][:n].cpu(), serial[i][:n].cpu())
            assert e < 1e-4, (i, e)
            for out in (serial[i], bucket[i]):
                Ti = out.shape[0]
                assert torch.equal(out[full[i, :Ti]], k[i, :Ti][full[i, :Ti]])
    joints = tr.generate_joints(caps, lens, 263, torch.zeros(263).numpy(), torch.ones(263).numpy(), batch_size=2,
                                **opts)
    assert [tuple(j.shape) for j in joints] == [(n, 22, 3) for n in lens.tolist()]
    with pytest.raises(ValueError):
        tr.generate(caps, same, 263, batch_size=2, seed=3, edit_motion=k)


def test_joint_feature_mask_matches_recover_from_ric():
    """recover_from_ric of a motion perturbed only on joint_feature_mask(S) moves no joint outside S (S without joint 0)."""
    E = pkg("motion_edit")
    P = pkg("postprocess")
    gen = torch.Generator().manual_seed(4)
    x = (torch.randn(2, 20, 263, generator=gen) * 0.3).cuda()
    base = P.recover_from_ric(x).cpu()
    for S in (E.UPPER_BODY, (1, 4, 7, 10), (20, 21)):
        y = x + E.joint_feature_mask(S).cuda() * torch.randn(x.shape, generator=gen).cuda()
        got = P.recover_from_ric(y).cpu()
        outside = [j for j in range(22) if j not in S]
        assert torch.equal(got[:, :, outside], base[:, :, outside]), S
        assert not torch.equal(got[:, :, list(S)], base[:, :, list(S)]), S


def test_configs1_shape_bf16_prefix_edit():
    """configs[1] shape (small, 8 experts, B=32, T=196, guided, 1000-step schedule) in bf16: DPM-Solver++(2M)-20 with a
    prefix mask through DDPMTrainer.generate gives finite motions whose first frames are the known ones."""
    T_ = pkg("transformer")
    synth = pkg("synth")
    E = pkg("motion_edit")
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
    k = synth.uniform_pm1((B, T, 263), "edit.configs1", 0).cuda()
    out = torch.stack(tr.generate(caps, length, 263, batch_size=B, seed=5, sampler="dpmpp2m", sample_steps=20,
                                  edit_motion=k, edit_mask=E.prefix_mask(T, 40))).cpu()
    assert torch.isfinite(out).all()
    assert torch.equal(out[:, :40], k[:, :40].cpu())
    plain = torch.stack(tr.generate(caps, length, 263, batch_size=B, seed=5, sampler="dpmpp2m", sample_steps=20)).cpu()
    print(f"[configs[1] bf16 prefix 40] rel_inf of the generated frames to the unedited run: "
          f"{rel_inf(out[:, 40:], plain[:, 40:]):.3e}")

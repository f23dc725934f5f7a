"""GPU: long motions from overlapping windows, tied together on every step.

* mdm_handshake_blend against an f64 restatement (2- and 3-entry frames, 1-4 groups, F = 263 and odd F, unaligned group
  strides and buffers), copy mode bit for bit, nshared = 0 a no-op, the argument errors;
* every sampler on a plain and a respaced schedule, graph and eager, with three windows of 16 / 12 / 16 frames and h = 4
  (a 36-frame canvas on the loops_tiny model, num_frames = 16): the overlap frames of neighbouring windows are equal bit for
  bit after every step and in x_T, and each step agrees with the loop restated in f64 (tests/sampler_ref.py) with the
  oracle's denoiser and a numpy blend before the update (teacher-forced on the device's trajectory);
* no overlap changes nothing (bitwise), graph == eager and two streams == one bitwise, a canvas prefix edit keeps its frames
  through the overlaps, and the trainer's generate_long / generate_long_joints (batch split, lengths, joints, the configs[1]
  shape in bf16).
"""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from conftest import pkg, rel_inf

import sampler_ref as S
from sampler_ref import caption_trainer as _trainer, make_diffusion as _diffusion, vp as _vp

pytestmark = pytest.mark.gpu

LENS, H, T = [16, 12, 16], 4, 16
SOLVERS = [("cfg", 0.0), ("ddpm", 0.0), ("cfg_ddim", 0.0), ("cfg_ddim", 0.5), ("ddim", 0.0), ("ddim", 0.5),
           ("cfg_dpmpp", 0.0)]


def _blend(x, groups, stride, F, ns, off, rows, w):
    L = pkg("_lib")
    return L.lib().mdm_handshake_blend(_vp(x), C.c_int32(groups), C.c_int64(stride), C.c_int32(F), C.c_int32(ns),
                                       _vp(off), _vp(rows), _vp(w), C.c_void_p(L.stream_ptr()))


# ---- kernel level ------------------------------------------------------------------------------------------------------
def _random_tables(gen, nshared, nrows, entries):
    """nshared frames of ``entries`` (int or list) distinct rows out of range(nrows), weights summing to 1."""
    cnt = [entries] * nshared if isinstance(entries, int) else list(entries)
    perm = torch.randperm(nrows, generator=gen)[:sum(cnt)]
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    w = torch.rand(sum(cnt), generator=gen, dtype=torch.float64) + 0.1
    for c in range(nshared):
        w[off[c]:off[c + 1]] /= w[off[c]:off[c + 1]].sum()
    return torch.from_numpy(off), perm.to(torch.int32), w.float()


@pytest.mark.parametrize("F", [263, 37])
@pytest.mark.parametrize("groups", [1, 2, 3, 4])
def test_blend_kernel_matches_f64(F, groups):
    gen = torch.Generator().manual_seed(groups * 1000 + F)
    nrows = 40
    for entries, nshared in ((2, 9), (3, 5), ([2, 3, 2, 3, 3, 2], 6)):
        off, rows, w = _random_tables(gen, nshared, nrows, entries)
        for pad in (0, 3):  # group stride nrows * F (+ 3: unaligned group starts)
            stride = nrows * F + pad
            base = torch.randn(groups * stride + 1, generator=gen)
            for shift in (0, 1):  # the buffer itself 4 bytes off 16-byte alignment
                buf = base.clone().cuda()
                x = buf[shift:shift + groups * stride]
                want = x.cpu().double().clone()
                for g in range(groups):
                    v = want[g * stride:g * stride + nrows * F].view(nrows, F)
                    for c in range(nshared):
                        es = range(int(off[c]), int(off[c + 1]))
                        s = sum(float(w[e]) * v[int(rows[e])] for e in es)
                        for e in es:
                            v[int(rows[e])] = s
                assert _blend(x, groups, stride, F, nshared, off.cuda(), rows.cuda(), w.cuda()) == 0
                got = x.cpu()
                touched = torch.zeros(groups * stride, dtype=torch.bool)
                for g in range(groups):
                    touched[g * stride:g * stride + nrows * F].view(nrows, F)[rows.long()] = True
                e = rel_inf(got[touched], want[touched])
                assert e <= 1e-6, (entries, pad, shift, e)
                assert torch.equal(got[~touched], base[shift:shift + groups * stride][~touched])  # nothing else moves
                # copy mode: every entry takes its frame's first entry, bit for bit
                buf = base.clone().cuda()
                x = buf[shift:shift + groups * stride]
                want = x.cpu().clone()
                for g in range(groups):
                    v = want[g * stride:g * stride + nrows * F].view(nrows, F)
                    for c in range(nshared):
                        for e in range(int(off[c]) + 1, int(off[c + 1])):
                            v[int(rows[e])] = v[int(rows[off[c]])]
                assert _blend(x, groups, stride, F, nshared, off.cuda(), rows.cuda(), None) == 0
                assert torch.equal(x.cpu(), want), (entries, pad, shift)


def test_blend_kernel_no_op_and_argument_errors():
    x = torch.randn(4 * 16 * 263, device="cuda")
    keep = x.clone()
    off = torch.tensor([0, 2], dtype=torch.int32, device="cuda")
    rows = torch.tensor([0, 5], dtype=torch.int32, device="cuda")
    assert _blend(x, 2, 2 * 16 * 263, 263, 0, None, None, None) == 0  # nshared == 0: no-op, tables unread
    assert _blend(None, 1, 0, 263, 0, None, None, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(x, keep)
    assert _blend(None, 1, 16 * 263, 263, 1, off, rows, None) == 1
    assert _blend(x, 1, 16 * 263, 263, 1, None, rows, None) == 1
    assert _blend(x, 1, 16 * 263, 263, 1, off, None, None) == 1
    assert _blend(x, 1, 16 * 263, 0, 1, off, rows, None) == 1
    assert _blend(x, 0, 16 * 263, 263, 1, off, rows, None) == 1
    assert _blend(x, 1, 16 * 263, 263, -1, off, rows, None) == 1
    assert _blend(x, 1, -1, 263, 1, off, rows, None) == 1
    assert _blend(x, 1, 16 * 263, 0, 0, None, None, None) == 1
    torch.cuda.synchronize()
    assert torch.equal(x, keep)


# ---- loops -------------------------------------------------------------------------------------------------------------
def _tables(lens=LENS, h=H, blend="linear"):
    ML = pkg("motion_long")
    starts, Cn = ML.plan_windows(lens, h)
    t = ML.handshake_tables(starts, lens, T, h, blend)
    kw = {"handshake_offsets": torch.from_numpy(t["offsets"]), "handshake_rows": torch.from_numpy(t["rows"]),
          "handshake_weights": torch.from_numpy(t["weights"]), "handshake_owner_rows": torch.from_numpy(t["owner_rows"])}
    return starts, Cn, t, kw


def _setup():
    g, meta, m, noises, _ = S.loops_setup(B=len(LENS))
    sel = [0, 1, 0]
    text = {"xf_proj": g["xf_proj"][sel], "xf_out": g["xf_out"][sel], "length": torch.tensor(LENS)}
    kw = {"xf_proj": text["xf_proj"].cuda(), "xf_out": text["xf_out"].cuda(), "length": text["length"].cuda(),
          "text": ["a", "b", "a"]}
    x_T = pkg("synth").uniform_pm1((len(LENS), T, g["x_T"].shape[2]), "long.x_T", meta["iseed"]) * (3.0 ** 0.5)
    return g, meta, m, noises, kw, text, x_T


def _overlaps_equal(x):
    """The overlap frames of neighbouring windows of (3, T, F) windows of LENS at H, bit for bit."""
    for i in range(len(LENS) - 1):
        if not torch.equal(x[i, LENS[i] - H:LENS[i]], x[i + 1, :H]):
            return False
    return True


def _owner(x, t):
    """x (B, T, F) with every overlap frame taken from its owner window (numpy restatement of the copy mode)."""
    y = x.clone().reshape(-1, x.shape[-1])
    off, rows = t["offsets"], t["owner_rows"]
    for c in range(len(off) - 1):
        for e in range(off[c] + 1, off[c + 1]):
            y[rows[e]] = y[rows[off[c]]]
    return y.view_as(x)


def _blend_np(eps, t):
    """f64 eps (B, T, F) with the weighted mean written to every entry of each shared frame."""
    y = eps.clone().reshape(-1, eps.shape[-1])
    off, rows, w = t["offsets"], t["rows"], t["weights"].astype(np.float64)
    for c in range(len(off) - 1):
        es = range(off[c], off[c + 1])
        v = sum(w[e] * y[rows[e]] for e in es)
        for e in es:
            y[rows[e]] = v
    return y.view_as(eps)


@pytest.mark.parametrize("schedule", ["plain25", "ddim10"])
@pytest.mark.parametrize("mode,eta", SOLVERS)
def test_overlaps_stay_bit_identical_and_match_the_oracle(mode, eta, schedule):
    g, meta, m, noises, kw, text, x_T = _setup()
    d = _diffusion(schedule)
    N, scale = d.num_timesteps, meta["cfg_scale"]
    starts, Cn, tab, hk = _tables()
    assert Cn == 36 and Cn > m.num_frames  # longer than the model can see
    ns = noises(f"long.{mode}.{eta}", N)
    lkw = dict(kw, **hk)
    finals = []
    for use_graph in (True, False):
        got = []
        out = S.run_loop(d, mode, m, lkw, scale, eta, use_graph, x_T=x_T.cuda(), step_noise=ns,
                         cb=lambda i, t, x: got.append(x.clone().cpu())).cpu()
        assert len(got) == N and torch.equal(out, got[-1])
        for i, x in enumerate(got):
            assert _overlaps_equal(x), (use_graph, i)
        # x_T: the owner's values are copied in, so an x_T that already has them gives the same loop bit for bit
        if use_graph:
            same = S.run_loop(d, mode, m, lkw, scale, eta, True, x_T=_owner(x_T, tab).cuda(), step_noise=ns).cpu()
            assert torch.equal(same, out)
            # the oracle's denoiser, a numpy blend of the cond and the uncond eps rows before x0, the step noise owner-copied
            want = S.loop_ref(d, mode, scale, S.oracle_eps(g, meta, text["length"]), prompts=[(text["xf_proj"], text["xf_out"])],
                              uncond=S.golden_text(g)["uncond"], inputs=[_owner(x_T, tab)] + got[:-1], eta=eta, step_noise=ns,
                              eps_hook=lambda e: _blend_np(e, tab), noise_hook=lambda z: _owner(z, tab))
            worst = max(rel_inf(got[i], want[i]) for i in range(N))
            print(f"[long] {mode} eta {eta} {schedule}: worst step rel_inf vs restated loop {worst:.2e}")
            assert worst <= 1e-4, worst
        finals.append(out)
    assert torch.equal(finals[0], finals[1])
    plain = S.run_loop(d, mode, m, kw, scale, eta, True, x_T=x_T.cuda(), step_noise=ns).cpu()
    assert not _overlaps_equal(plain)  # without handshakes the windows disagree


@pytest.mark.parametrize("mode,eta", [("cfg", 0.0), ("cfg_ddim", 0.5), ("ddim", 0.5), ("cfg_dpmpp", 0.0)])
def test_no_overlap_changes_nothing_and_graph_streams_are_bitwise(mode, eta):
    g, meta, m, noises, kw, text, x_T = _setup()
    d = _diffusion("ddim10")
    shape = (len(LENS), T, x_T.shape[2])
    _, _, _, h0 = _tables(h=0)
    plain = d._runner(m, shape, kw, "cuda", mode, meta["cfg_scale"], eta, False, True).run(
        x_T.cuda(), None, False, None, seed=5).cpu()
    none = d._runner(m, shape, dict(kw, **h0), "cuda", mode, meta["cfg_scale"], eta, False, True).run(
        x_T.cuda(), None, False, None, seed=5).cpu()
    assert torch.equal(plain, none)
    _, _, _, hk = _tables(blend="uniform")
    outs = {}
    for use_graph, streams in ((True, 1), (False, 1), (True, 2)):
        r = d._runner(m, shape, dict(kw, **hk), "cuda", mode, meta["cfg_scale"], eta, False, use_graph, streams)
        outs[(use_graph, streams)] = r.run(None, None, False, None, seed=11).cpu()
    assert torch.isfinite(outs[(True, 1)]).all() and _overlaps_equal(outs[(True, 1)])
    assert torch.equal(outs[(True, 1)], outs[(False, 1)])
    assert torch.equal(outs[(True, 1)], outs[(True, 2)])
    # progressive loop: the same arithmetic, x_T owner-copied as well
    prog = list(d.ddim_sample_loop_progressive(m, shape, noise=x_T.cuda(), clip_denoised=False, model_kwargs=dict(kw, **hk),
                                               eta=0.0))
    loop = d.ddim_sample_loop(m, shape, noise=x_T.cuda(), clip_denoised=False, model_kwargs=dict(kw, **hk),
                              use_graph=False).cpu()
    assert torch.equal(prog[-1]["sample"].cpu(), loop) and _overlaps_equal(loop)


# ---- trainer ------------------------------------------------------------------------------------------------------------
SCRIPTS = [[("walk", 16), ("turn", 12), ("sit", 16)], [("jump", 16)], [("run", 10), ("stop", 12)]]


def test_trainer_generate_long():
    ML = pkg("motion_long")
    g, meta, m, noises, kw, text, x_T = _setup()
    tr = _trainer(m, meta)
    opts = dict(overlap=4, seed=3, sampler="ddim", sample_steps=10, eta=0.5)
    canv = [ML.plan_windows([n for _, n in sc], 4)[1] for sc in SCRIPTS]
    outs = {bs: [o.cpu() for o in tr.generate_long(SCRIPTS, 263, batch_size=bs, **opts)] for bs in (3, 6)}
    assert [tuple(o.shape) for o in outs[3]] == [(c, 263) for c in canv] == [(36, 263), (16, 263), (18, 263)]
    for a, b in zip(outs[3], outs[6]):
        assert torch.isfinite(a).all() and rel_inf(a, b) < 1e-5, rel_inf(a, b)
    # a single-window script is generate() under the same seed (window k = global sample k), bit for bit
    one = tr.generate_long([[("jump", 16)]], 263, **opts)[0].cpu()
    ref = tr.generate(["jump"], torch.tensor([16]), 263, seed=3, sampler="ddim", sample_steps=10, eta=0.5)[0].cpu()
    assert torch.equal(one, ref)
    # h = 0: the windows are independent samples, each generate()'s sample of the same global index
    flat = [c for sc in SCRIPTS for c in sc]
    z = tr.generate_long(SCRIPTS, 263, batch_size=6, **dict(opts, overlap=0))
    ref = tr.generate([c for c, _ in flat], torch.tensor([n for _, n in flat]), 263, batch_size=6, seed=3, sampler="ddim",
                      sample_steps=10, eta=0.5)
    k = 0
    for mo, sc in zip(z, SCRIPTS):
        s = 0
        for _, n in sc:
            assert torch.equal(mo[s:s + n].cpu(), ref[k][:n].cpu()), k
            s, k = s + n, k + 1
    # canvas noise: the result is a function of it
    nz = [torch.randn(c, 263, generator=torch.Generator().manual_seed(i)) for i, c in enumerate(canv)]
    a = tr.generate_long(SCRIPTS, 263, noise=nz, **opts)
    b = tr.generate_long(SCRIPTS, 263, noise=nz, **opts)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    # joints over the whole canvas
    mean, std = np.zeros(263, np.float32), np.ones(263, np.float32)
    std[0] = 0.05
    post = pkg("postprocess")
    joints = tr.generate_long_joints(SCRIPTS, 263, mean, std, batch_size=6, sigma=1.0, **opts)
    for j, mo, c in zip(joints, outs[6], canv):
        assert tuple(j.shape) == (c, 22, 3)
        want = post.motion_to_joints(mo.cuda()[None], mean, std, torch.tensor([c]), 22, 1.0)[0]
        assert torch.equal(j, want)


def test_canvas_prefix_edit_keeps_its_frames_through_the_overlaps():
    E = pkg("motion_edit")
    synth = pkg("synth")
    g, meta, m, noises, kw, text, x_T = _setup()
    tr = _trainer(m, meta)
    script = SCRIPTS[0]
    Cn = 36
    known = synth.uniform_pm1((Cn, 263), "long.known", meta["iseed"]) * 1.5
    for n_keep in (14, 22):  # inside the first overlap (canvas 12-15), past the second (20-23)
        mask = E.prefix_mask(Cn, n_keep)
        for sampler, extra in (("ddim", dict(eta=0.5)), ("dpmpp2m", {}), ("ddpm", {})):
            out = tr.generate_long([script], 263, overlap=4, seed=9, sampler=sampler, sample_steps=10, edit_motion=[known],
                                   edit_mask=[mask], **extra)[0].cpu()
            assert torch.equal(out[:n_keep], known[:n_keep]), (n_keep, sampler)
            assert not torch.equal(out[n_keep:], known[n_keep:])


def test_configs1_shape_bf16_four_600_frame_motions():
    """configs[1] widths (small, 8 experts, num_frames 196, guided, 1000-step schedule) in bf16: four 600-frame motions of
    four 165-frame windows each (h = 20) through DPM-Solver++(2M)-20 are finite."""
    ML = pkg("motion_long")
    T_ = pkg("transformer")
    synth = pkg("synth")
    m = T_.MotionTransformer(263, num_frames=196, latent_dim=512, ff_size=1024, num_layers=4, num_heads=4,
                             text_latent_dim=256, moe_num_experts=8, model_size="small", precision=1)
    m.load_state_dict(synth.synth_state_dict(m._layout, 0), strict=True)
    m.set_ephemerals(synth.synth_ephemerals(512, 256, 4, 7)), m.set_projections(synth.synth_projections(128, 4, 7))
    xo_u = synth.uniform_pm1((1, 28, 256), "in.uncond", 0) * (3.0 ** 0.5)
    m = m.cuda().eval()
    m.set_uncond_embedding(xo_u.mean(1).cuda(), xo_u.cuda())

    def enc(text, device):
        xo = torch.stack([synth.uniform_pm1((28, 256), "cap." + t, 0) * (3.0 ** 0.5) for t in text])
        return xo.mean(1).to(device), xo.to(device)

    m.text_encoder_fn = enc
    Tr = pkg("trainer")
    tr = Tr.DDPMTrainer(types.SimpleNamespace(device=torch.device("cuda"), diffusion_steps=1000, is_train=False,
                                              cfg_scale=7.5), m)
    scripts = [ML.split_long(f"caption {i}", 600, 196, 20) for i in range(4)]
    assert [len(s) for s in scripts] == [4] * 4
    out = tr.generate_long(scripts, 263, overlap=20, batch_size=32, seed=5, sampler="dpmpp2m", sample_steps=20)
    assert [tuple(o.shape) for o in out] == [(600, 263)] * 4
    assert all(bool(torch.isfinite(o).all()) for o in out)

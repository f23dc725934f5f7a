"""GPU: tracks: moving obstacles and a second character, per-frame records next to the scene of §24.

* mdm_joint_tracks_loss_grad against the fp64 autograd restatement of tests/scene_tracks_ref.py: (B, T) = (1, 2) and (3, 40) at
  F = 263 and 251 with Km = 5 tracks, (2, 196) at F = 263 with 16 static primitives and Km = 24, ragged lengths with 0 and 1,
  tracks only / plus a static scene / plus fractional target weights / joint weights with zeros / non-zero radii; the records
  follow the reference's own positions and are shifted clear of their jump sets, and the test asserts that placement (every
  penalised joint >= 1e-3 m from a jump set, every track penalising >= 5 % of (t, j) in a sample) before it looks at the
  kernel; gates are §14's (loss rel <= 1e-5, gradient rel_inf <= 1e-4, exact zeros);
* bitwise: Km = 0 is mdm_joint_scene_loss_grad; the broad phase's balls against NULL bounds for loss, gradient and the
  guidance's x and x0 on every case and the canvas; padding tracks and tracks no joint touches leave x and x0 (-0.0
  included); masked entries keep their bits; a track active on some frames is the track with weight 0 on the others;
* the guidance kernel's single step, its update of x and k iterations = k chained steps; the argument errors;
* the canvas kernel: two motions of 70 and 300 frames through shuffled rows against the restatement, and a 40-frame canvas
  against the window kernel;
* loops: cfg_dpmpp and ddim eta = 0.5 with tracks, a static scene and a root path against the loop restated in
  tests/sampler_ref.py with the autograd guidance, teacher-forced, <= 1e-4 per step, one with an edit mask; graph == eager
  bitwise; a long motion of two windows at overlap 20 against the restated canvas loop;
* the trainer: generate(scene_tracks=) independent of the batch split and of bucketing, generate_long(scene_tracks=) of the
  batch split, generate_together with one character is generate_joints + to_world bit for bit, character 0 does not depend on
  character 1;
* behaviour: a sphere that crosses a pelvis path when the pelvis does, and two characters on crossing paths: the tracks cut
  L_tracks of the final sample and the second character's penetration of the first.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import pkg, rel_inf
from test_motion_control_host import ref_positions

import sampler_ref as S
import scene_ref as R
import scene_tracks_ref as TR
from sampler_ref import caption_trainer as _trainer, loops_setup as _setup, make_diffusion as _diffusion, vp as _vp
from test_motion_control_gpu import _stats
from test_motion_scene_gpu import CANVAS, H, LENS, TW, _case as _scene_case, _check_against_restated, _cuda, _long_setup, _loop_scene

pytestmark = pytest.mark.gpu

VARIANTS = ("tracks", "scene", "targets", "joint_weights", "radii")
SHAPES = [(1, 2, 263, 5), (1, 2, 251, 5), (3, 40, 263, 5), (3, 40, 251, 5), (2, 196, 263, 24)]
SEED = 2  # of place_tracks, per sample b: SEED + b.  With these draws the reference alone meets the placement conditions


@functools.lru_cache(maxsize=None)
def _case(B, T, F, Km, variant):
    """The draws of test_motion_scene_gpu._case (x0, mean, std, lengths with 0 and 1, joint parameters, the static scene placed
    from the reference's positions and, for "targets", fractional target weights) plus Km tracks per sample that follow the
    reference's positions, and the reference's loss and gradient.  "tracks": no static scene.  Shared by the tests, left
    unchanged."""
    K = 16 if Km == 24 else 5
    c = dict(_scene_case(B, T, F, K, "scene" if variant == "tracks" else variant))
    if variant == "tracks":
        c["scene"] = torch.zeros(B, 0, 12)
    c["tracks"] = torch.stack([TR.place_tracks(c["P"][b], c["jp"][b], Km, seed=SEED + b, T=T) for b in range(B)]).float()
    c["tstats"] = [TR.track_stats(c["P"][b], c["tracks"][b].double(), c["jp"][b]) for b in range(B)]
    c["ref"] = TR.ref_tracks_loss_grad(c["x0"], c["lens"], c["mean"], c["std"], c["tracks"], c["jp"],
                                       c["scene"] if c["scene"].shape[1] else None, c["tg"], c["w"])
    c["bounds"] = pkg("motion_scene").track_bounds(c["tracks"])
    return c


def _cu(v):
    return None if v is None else v.cuda().float().contiguous()


def _tracks_lg(x0, lens, mean, std, scene, jp, tracks, bounds=None, tg=None, w=None):
    """mdm_joint_tracks_loss_grad on packed records: scene (B, K, 12), tracks (B, T, Km, 12), bounds (B, T, 4) or None."""
    L = pkg("_lib")
    B, T, F = x0.shape
    dev = [_cu(v) for v in (x0, mean, std, tg, w, scene, jp, tracks, bounds)]
    ln = lens.cuda().to(torch.int32)
    loss, grad = torch.empty(B, device="cuda"), torch.empty(B, T, F, device="cuda")
    K, Km = scene.shape[1], tracks.shape[2]
    L.check(L.lib().mdm_joint_tracks_loss_grad(_vp(dev[0]), _vp(ln), _vp(dev[1]), _vp(dev[2]), _vp(dev[3]), _vp(dev[4]),
                                               _vp(dev[5] if K else None), C.c_int32(K), _vp(dev[6]), _vp(dev[7] if Km else None),
                                               C.c_int32(Km), _vp(dev[8]), C.c_int32(B), C.c_int32(T), C.c_int32(F), _vp(loss),
                                               _vp(grad), C.c_void_p(L.stream_ptr())))
    return loss.cpu(), grad.cpu()


def _bits(v):
    return v.contiguous().view(torch.int32)


# ---- mdm_joint_tracks_loss_grad -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("B,T,F,Km", SHAPES)
def test_tracks_loss_grad_matches_fp64_autograd(B, T, F, Km, variant):
    c = _case(B, T, F, Km, variant)
    D = 3 * ((F + 1) // 12) + 1
    # the placement, on the reference alone
    jump = torch.stack([s[0] for s in c["tstats"]])
    share = torch.stack([s[1] for s in c["tstats"]])
    print(f"[tracks B={B} T={T} F={F} Km={Km} {variant}] least jump distance {float(jump.min()):.2e} m, least share of (t, j) "
          f"penalised per track (best sample) {float(share.max(0).values.min()):.3f}")
    assert float(jump.min()) >= R.JUMP_CLEAR, jump
    assert bool((share.max(0).values >= 0.05).all()), share
    loss, grad = _tracks_lg(c["x0"], c["lens"], c["mean"], c["std"], c["scene"], c["jp"], c["tracks"], c["bounds"], c["tg"], c["w"])
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
    print(f"[tracks B={B} T={T} F={F} Km={Km} {variant}] worst loss rel {worst_l:.2e}, worst gradient rel_inf {worst_g:.2e}")
    # the broad phase changes no bit: the balls against NULL bounds
    l0, g0 = _tracks_lg(c["x0"], c["lens"], c["mean"], c["std"], c["scene"], c["jp"], c["tracks"], None, c["tg"], c["w"])
    assert torch.equal(_bits(loss), _bits(l0)) and torch.equal(_bits(grad), _bits(g0))


def test_python_entry_equals_the_packed_call():
    """motion_scene.scene_loss_grad(tracks=) on lists of track stacks: one shared list, one list per sample, with and without
    the broad phase; the tracks term is what the static scene of a frame's records gives for that frame."""
    MS = pkg("motion_scene")
    c = _case(3, 40, 263, 5, "scene")
    P = c["P"][0].float()
    trk = [MS.moving_sphere(P[:, 15] + torch.tensor([0.1, 0.0, 0.1]), 0.4, margin=0.05),
           # a bar beside the pelvis (through it, the pelvis would sit on the axis, where the gradient jumps)
           MS.moving_capsule(P[:, 0] + torch.tensor([0.3, -1.0, -0.3]), P[:, 0] + torch.tensor([0.3, 1.0, 0.3]), 0.25, weight=2.0),
           MS.moving_half_space((0.0, 1.0, 0.0), torch.linspace(0.0, 0.5, 40))]
    prims = [MS.sphere((0.3, 0.8, 0.2), 0.7, margin=0.05), MS.floor(0.1)]
    rec, jp = MS.pack_scene(prims), MS.joint_params(22, [0.05] * 22, None)
    args = (c["x0"].cuda(), c["lens"], c["mean"], c["std"])
    loss, grad = MS.scene_loss_grad(*args, prims, joint_radius=[0.05] * 22, tracks=trk)
    packed = MS.batch_tracks(trk, 3, 40)
    l2, g2 = _tracks_lg(c["x0"], c["lens"], c["mean"], c["std"], rec[None].expand(3, -1, -1), jp[None].expand(3, -1, -1), packed,
                        MS.track_bounds(packed))
    assert torch.equal(loss.cpu(), l2) and torch.equal(grad.cpu(), g2) and float(l2[0]) > 0
    l3, g3 = MS.scene_loss_grad(*args, prims, joint_radius=[0.05] * 22, tracks=trk, bounds=False)
    assert torch.equal(_bits(l3.cpu()), _bits(l2)) and torch.equal(_bits(g3.cpu()), _bits(g2))
    per = [trk, trk[:1], []]
    l4, g4 = MS.scene_loss_grad(*args, None, joint_radius=[0.05] * 22, tracks=per)
    rl, rg = TR.ref_tracks_loss_grad(c["x0"], c["lens"], c["mean"], c["std"], MS.batch_tracks(per, 3, 40), jp[None].expand(3, -1, -1))
    assert abs(float(l4[0]) - float(rl[0])) <= 1e-5 * float(rl[0]) and float(l4[1]) == 0.0 and float(l4[2]) == 0.0
    assert rel_inf(g4[0].cpu(), rg[0]) <= 1e-4
    # without tracks the call is the scene's
    l5, g5 = MS.scene_loss_grad(*args, prims, joint_radius=[0.05] * 22)
    l6, g6 = MS.scene_loss_grad(*args, prims, joint_radius=[0.05] * 22, tracks=[])
    assert torch.equal(_bits(l5), _bits(l6)) and torch.equal(_bits(g5), _bits(g6))


# ---- bitwise ------------------------------------------------------------------------------------------------------------
def test_no_tracks_is_the_scene_loss_grad_bitwise():
    from test_motion_scene_gpu import _scene_lg
    c = _case(3, 40, 263, 5, "targets")
    none = torch.zeros(3, 40, 0, 12)
    loss, grad = _tracks_lg(c["x0"], c["lens"], c["mean"], c["std"], c["scene"], c["jp"], none, None, c["tg"], c["w"])
    l0, g0 = _scene_lg(c["x0"], c["lens"], c["mean"], c["std"], c["scene"], c["jp"], c["tg"], c["w"])
    assert torch.equal(_bits(loss), _bits(l0)) and torch.equal(_bits(grad), _bits(g0)) and float(l0[0]) > 0
    # padding tracks only, through the tracks instantiation: the same values up to fp32 rounding (another instantiation may
    # contract its products differently)
    pad = torch.zeros(3, 40, 4, 12)
    loss, grad = _tracks_lg(c["x0"], c["lens"], c["mean"], c["std"], c["scene"], c["jp"], pad, None, c["tg"], c["w"])
    assert rel_inf(loss, l0) <= 1e-6 and rel_inf(grad, g0) <= 1e-6
    # neither tracks that bite nor a scene nor targets: zero
    loss, grad = _tracks_lg(c["x0"], c["lens"], c["mean"], c["std"], torch.zeros(3, 0, 12), c["jp"], pad)
    assert not loss.any() and not grad.any()


def test_a_track_active_on_some_frames_is_the_track_with_weight_zero_on_the_others():
    c = _case(3, 40, 263, 5, "scene")
    a, b = 7, 23
    gone, zero = c["tracks"].clone(), c["tracks"].clone()
    gone[:, :a, 1] = 0.0  # track 1 (the capsule) absent outside [a, b): padding records
    gone[:, b:, 1] = 0.0
    zero[:, :a, 1, 2] = 0.0  # the same track with weight 0 there
    zero[:, b:, 1, 2] = 0.0
    MS = pkg("motion_scene")
    out = {}
    for name, trk in (("gone", gone), ("zero", zero), ("all", c["tracks"])):
        for bounds in (None, MS.track_bounds(trk)):
            out[name, bounds is None] = _tracks_lg(c["x0"], c["lens"], c["mean"], c["std"], c["scene"], c["jp"], trk, bounds)
    for bounds in (True, False):
        assert torch.equal(_bits(out["gone", bounds][0]), _bits(out["zero", bounds][0]))
        assert torch.equal(_bits(out["gone", bounds][1]), _bits(out["zero", bounds][1]))
    assert torch.equal(_bits(out["gone", True][1]), _bits(out["gone", False][1]))
    assert not torch.equal(out["gone", True][1], out["all", True][1])


def _guide(x, x0, mask, lens, mean, std, tg, w, scene, jp, tracks, bounds, scale, iters, coef, steps, t, shape=None, K=None,
           Km=None):
    L = pkg("_lib")
    B, T, F = x0.shape if shape is None else shape
    K = (0 if scene is None else scene.shape[1]) if K is None else K
    Km = (0 if tracks is None else tracks.shape[2]) if Km is None else Km
    return L.lib().mdm_joint_tracks_guidance(_vp(x), _vp(x0), _vp(mask), _vp(lens), _vp(mean), _vp(std), _vp(tg), _vp(w), _vp(scene),
                                             C.c_int32(K), _vp(jp), _vp(tracks), C.c_int32(Km), _vp(bounds), C.c_int32(B),
                                             C.c_int32(T), C.c_int32(F), C.c_float(scale), C.c_int32(iters), _vp(coef),
                                             C.c_int32(steps), C.c_void_p(0), C.c_int32(t), C.c_void_p(L.stream_ptr()))


def _kernel_case(variant="targets", shape=(3, 40, 263, 5)):
    c = _case(*shape, variant)
    gen = torch.Generator().manual_seed(3)
    B, T, F, _ = shape
    return dict(x=torch.randn(B, T, F, generator=gen).cuda(), x0=_cu(c["x0"]), mean=_cu(c["mean"]), std=_cu(c["std"]),
                tg=_cu(c["tg"]), w=_cu(c["w"]), scene=_cu(c["scene"]) if c["scene"].shape[1] else None, jp=_cu(c["jp"]),
                tracks=_cu(c["tracks"]), bounds=_cu(c["bounds"]), lens=c["lens"].cuda().to(torch.int32))


def _kargs(k, bounds=True):
    return (k["lens"], k["mean"], k["std"], k["tg"], k["w"], k["scene"], k["jp"], k["tracks"], k["bounds"] if bounds else None)


def test_guidance_kernel_steps_and_update():
    L = pkg("_lib")
    d = _diffusion("ddim10")
    N = d.num_timesteps
    k = _kernel_case()
    c = _case(3, 40, 263, 5, "targets")
    x, x0, lens = k["x"], k["x0"], k["lens"]
    D = 67

    def grad_of(y):
        return _tracks_lg(y, lens.cpu(), c["mean"], c["std"], c["scene"], c["jp"], c["tracks"], c["bounds"], c["tg"], c["w"])[1].cuda()

    scale = 0.01
    for kind in ("ddim", "dpmpp", "ddpm"):
        coef = d._device_coef(kind, 0.0, 2, "cuda")
        for t in (N - 1, N // 2, 0):
            c0 = float(coef[t, 1])
            xo, x0o = x.clone(), x0.clone()
            L.check(_guide(xo, x0o, None, *_kargs(k), scale, 1, coef, N, t))
            # one fp32 step each way, a few ulp of the largest value involved (as §24's test: the gradients are large)
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
            x1, x01 = x.clone(), x0.clone()  # the broad phase changes no bit
            L.check(_guide(x1, x01, None, *_kargs(k, False), scale, 1, coef, N, t))
            assert torch.equal(_bits(x1), _bits(xo)) and torch.equal(_bits(x01), _bits(x0o))
    # k iterations = k chained loss-grad steps, at the step size §24's test derives for these weights (1e-5)
    coef = d._device_coef("ddim", 0.0, 2, "cuda")
    scale = 1e-5
    for it in (2, 5):
        xo, x0o = x.clone(), x0.clone()
        L.check(_guide(xo, x0o, None, *_kargs(k), scale, it, coef, N, 3))
        y = x0.clone()
        for _ in range(it):
            y = y - scale * grad_of(y)
        e = float((x0o - y).abs().max()) / float(x0.abs().max())
        print(f"[tracks guidance] {it} iterations vs chained loss-grad steps: {e:.2e}")
        assert e <= 1e-5, (it, e)
        x1, x01 = x.clone(), x0.clone()
        L.check(_guide(x1, x01, None, *_kargs(k, False), scale, it, coef, N, 3))
        assert torch.equal(_bits(x1), _bits(xo)) and torch.equal(_bits(x01), _bits(x0o))
    # tracks without a scene and without targets move x0 as well
    xo, x0o = x.clone(), x0.clone()
    L.check(_guide(xo, x0o, None, lens, k["mean"], k["std"], None, None, None, k["jp"], k["tracks"], k["bounds"], 0.01, 1, coef, N, 3))
    g = _tracks_lg(c["x0"], lens.cpu(), c["mean"], c["std"], torch.zeros(3, 0, 12), c["jp"], c["tracks"], c["bounds"])[1].cuda()
    want = x0 - 0.01 * g
    assert float((x0o - want).abs().max()) <= 1e-6 * float(torch.maximum(x0.abs(), want.abs()).max())
    assert not torch.equal(x0o, x0)


@pytest.mark.parametrize("shape", SHAPES)
def test_guidance_with_bounds_equals_null_bounds_bitwise(shape):
    """x and x0 after three guidance iterations, with the balls and with NULL bounds, with and without an edit mask."""
    L = pkg("_lib")
    d = _diffusion("ddim10")
    N = d.num_timesteps
    coef = d._device_coef("dpmpp", 0.0, 2, "cuda")
    k = _kernel_case("radii", shape)
    gen = torch.Generator().manual_seed(5)
    mask = (torch.rand(k["x0"].shape, generator=gen) < 0.5).float().cuda()
    for m in (None, mask):
        outs = []
        for bounds in (True, False):
            xo, x0o = k["x"].clone(), k["x0"].clone()
            L.check(_guide(xo, x0o, m, *_kargs(k, bounds), 1e-5, 3, coef, N, 4))
            outs.append((xo, x0o))
        assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0])) and torch.equal(_bits(outs[0][1]), _bits(outs[1][1]))
        assert not torch.equal(outs[0][1], k["x0"])


def test_untouched_tracks_and_masked_entries_are_bitwise_unchanged():
    L, MS = pkg("_lib"), pkg("motion_scene")
    d = _diffusion("ddim10")
    N = d.num_timesteps
    coef = d._device_coef("dpmpp", 0.0, 2, "cuda")
    k = _kernel_case("tracks")
    x, x0, lens = k["x"].clone(), k["x0"].clone(), k["lens"]
    x0[0, :5, :10] = -0.0
    x[0, :5, :10] = -0.0
    T = 40
    t = torch.arange(T, dtype=torch.float64)
    # far from every joint in every frame: a sphere and a bar circling 1 km away, a floor sinking 1 km below, a keep-in box
    # of 1 km half extents that turns
    ring = torch.stack([1000 * torch.cos(0.1 * t), torch.zeros(T, dtype=torch.float64), 1000 * torch.sin(0.1 * t)], 1)
    far = [MS.moving_sphere(ring, 1.0, margin=0.5), MS.moving_capsule(ring, ring + torch.tensor([0.0, 5.0, 0.0]), 0.5),
           MS.moving_half_space((0, 1, 0), -1000.0 - t), MS.moving_box(torch.zeros(T, 3), (1000, 1000, 1000), 0.01 * t, inside=True)]
    pad = torch.zeros(3, T, 3, 12)
    for trk in (MS.batch_tracks(far, 3, T), MS.batch_tracks(far[:2], 3, T), pad):
        for bounds in (MS.track_bounds(trk).cuda(), None):
            xo, x0o = x.clone(), x0.clone()
            L.check(_guide(xo, x0o, None, lens, k["mean"], k["std"], None, None, None, k["jp"], trk.cuda().contiguous(), bounds, 0.05,
                           3, coef, N, 4))
            assert torch.equal(_bits(xo), _bits(x)) and torch.equal(_bits(x0o), _bits(x0))
    gen = torch.Generator().manual_seed(8)
    mask = (torch.rand(x0.shape, generator=gen) < 0.5).float().cuda()
    xo, x0o = x.clone(), x0.clone()
    L.check(_guide(xo, x0o, mask, *_kargs(k)[:3], None, None, None, k["jp"], k["tracks"], k["bounds"], 1e-3, 3, coef, N, 4))
    keep = mask == 1
    assert torch.equal(_bits(x0o[keep]), _bits(x0[keep])) and torch.equal(_bits(xo[keep]), _bits(x[keep]))
    assert not torch.equal(x0o[~keep], x0[~keep])


def test_argument_errors():
    L = pkg("_lib")
    lib = L.lib()
    d = _diffusion("ddim10")
    N = d.num_timesteps
    coef = d._device_coef("ddim", 0.0, 2, "cuda")
    k = _kernel_case()
    a = [k["x"].clone(), k["x0"].clone(), None, k["lens"], k["mean"], k["std"], k["tg"], k["w"], k["scene"], k["jp"], k["tracks"],
         k["bounds"], 0.001, 1, coef, N, 0, (3, 40, 263)]
    assert _guide(*a) == 0
    for i in (0, 1, 3, 4, 5, 6, 7, 9, 14):  # a null pointer; targets without weights and the reverse
        bad = list(a)
        bad[i] = None
        assert _guide(*bad) == 1, i
    bad = list(a)
    bad[11] = None  # NULL bounds are allowed
    assert _guide(*bad) == 0
    assert _guide(*a, Km=5) == 0 and _guide(*a, Km=25) == 1 and _guide(*a, Km=-1) == 1
    assert _guide(*a, K=5) == 0 and _guide(*a, K=17) == 1 and _guide(*a, K=-1) == 1
    bad = list(a)
    bad[10] = None
    assert _guide(*bad, Km=5) == 1  # null tracks with Km > 0
    bad[10] = k["tracks"].flatten()[1:]  # records are read 16 bytes at a time
    assert _guide(*bad, Km=5) == 1
    for i, v in ((12, float("nan")), (12, float("inf")), (13, 0), (13, L.CONTROL_MAX_ITERS + 1), (15, 0), (16, N), (16, -1)):
        bad = list(a)
        bad[i] = v
        assert _guide(*bad) == 1, (i, v)
    for shape in ((3, 40, 262), (3, 0, 263), (-1, 40, 263), (3, 205, 263)):
        assert _guide(*a[:-1], shape) == 1, shape
    # the T limit is the scene's: 202 frames at F = 263 with 16 primitives, whatever the tracks
    big = torch.zeros(1, 203, 263, device="cuda")
    sc16, t24 = torch.zeros(1, 16, 12, device="cuda"), torch.zeros(1, 203, 24, 12, device="cuda")
    loss = torch.empty(1, device="cuda")

    def lg(T_, K_, Km_):
        return lib.mdm_joint_tracks_loss_grad(_vp(big), _vp(k["lens"]), _vp(k["mean"]), _vp(k["std"]), None, None, _vp(sc16),
                                              C.c_int32(K_), _vp(k["jp"]), _vp(t24), C.c_int32(Km_), None, C.c_int32(1),
                                              C.c_int32(T_), C.c_int32(263), _vp(loss), _vp(big), C.c_void_p(L.stream_ptr()))

    assert lg(203, 16, 24) == 1 and lg(202, 16, 24) == 0 and lg(203, 8, 24) == 0 and lg(202, 16, 25) == 1 and lg(203, 16, 0) == 1
    torch.cuda.synchronize()


# ---- the canvas kernel --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _canvas_case(canvases, F, with_targets):
    from test_long_control_gpu import _layout, _stats as _cstats, _weights as _cweights
    from test_motion_scene_gpu import _joint_params
    J, Tw = (F + 1) // 12, 200
    gen = torch.Generator().manual_seed(sum(canvases) * 7 + F)
    B, off, fr = _layout(canvases, Tw, sum(canvases) + F + 1)  # a seed that deals the windows out of order
    x = torch.randn(B, Tw, F, generator=gen) * 0.7
    mean, std = _cstats(F, len(canvases), F + len(canvases))
    total = int(off[-1])
    tg = torch.randn(total, J, 3, generator=gen) * 2.0
    w = torch.cat([_cweights("frac", n, J, n + F) for n in canvases])
    jp = _joint_params("radii", len(canvases), J, total)
    flat = x.reshape(-1, F)
    scene, tracks, stats, loss, grad = [], [], [], [], torch.zeros(total, F, dtype=torch.float64)
    for m in range(len(canvases)):
        a, b = int(off[m]), int(off[m + 1])
        rows = flat[fr[a:b]]
        P = ref_positions(rows, mean[m], std[m]).detach()
        scene.append(R.place_scene(P, jp[m], 5, seed=m).float())
        tracks.append(TR.place_tracks(P, jp[m], 5, seed=SEED + m).float())
        stats.append(TR.track_stats(P, tracks[-1].double(), jp[m]))
        l, g = TR.ref_tracks_loss_grad(rows[None], [b - a], mean[m], std[m], tracks[-1][None], jp[m][None], scene[-1][None],
                                       tg[a:b][None] if with_targets else None, w[a:b][None] if with_targets else None)
        loss.append(l[0])
        grad[a:b] = g[0]
    tracks = torch.cat(tracks)
    return dict(x=x, off=off, fr=fr, mean=mean, std=std, tg=tg if with_targets else None, w=w if with_targets else None, jp=jp,
                scene=torch.stack(scene), tracks=tracks, bounds=pkg("motion_scene").track_bounds(tracks), stats=stats,
                ref=(torch.stack(loss), grad))


def _canvas_lg(c, bounds=True):
    """mdm_canvas_tracks_loss_grad on packed records: scene (M, K, 12), tracks (total, Km, 12), bounds (total, 4)."""
    L = pkg("_lib")
    F = c["x"].shape[-1]
    M, total = c["off"].numel() - 1, c["fr"].numel()
    x, mean, std, tg, w, scene, jp, tracks, bnd = (_cu(c[k]) for k in ("x", "mean", "std", "tg", "w", "scene", "jp", "tracks", "bounds"))
    off, fr = c["off"].cuda().to(torch.int32), c["fr"].cuda().to(torch.int32)
    loss, grad = torch.zeros(M, device="cuda"), torch.zeros(total, F, device="cuda")
    ws = torch.empty(int(L.lib().mdm_canvas_control_workspace_floats(total, F)), device="cuda")
    L.check(L.lib().mdm_canvas_tracks_loss_grad(_vp(x), _vp(off), _vp(fr), _vp(mean), _vp(std), _vp(tg), _vp(w), _vp(scene),
                                                C.c_int32(scene.shape[1]), _vp(jp), _vp(tracks), C.c_int32(tracks.shape[1]),
                                                _vp(bnd if bounds else None), C.c_int32(M), C.c_int32(F), _vp(loss), _vp(grad),
                                                _vp(ws), C.c_void_p(L.stream_ptr())))
    return loss.cpu(), grad.cpu()


@pytest.mark.parametrize("with_targets", [False, True])
def test_canvas_tracks_loss_grad_matches_fp64_autograd(with_targets):
    canvases, F = (70, 300), 263  # tiles are 64 frames, blocks 256
    c = _canvas_case(canvases, F, with_targets)
    jump = torch.stack([s[0] for s in c["stats"]])
    share = torch.stack([s[1] for s in c["stats"]])
    print(f"[canvas tracks] least jump distance {float(jump.min()):.2e} m, share penalised {share.max(0).values.tolist()}")
    assert float(jump.min()) >= R.JUMP_CLEAR and bool((share.max(0).values >= 0.05).all())
    assert len(set((c["fr"] // 200).tolist())) > 1 and bool((c["fr"][1:] < c["fr"][:-1]).any())  # several rows, not in order
    loss, grad = _canvas_lg(c)
    rl, rg = c["ref"]
    assert torch.equal(grad[:, 67:], torch.zeros(sum(canvases), F - 67))
    for m, n in enumerate(canvases):
        a = int(c["off"][m])
        el = abs(float(loss[m]) - float(rl[m])) / float(rl[m])
        eg = rel_inf(grad[a:a + n], rg[a:a + n])
        print(f"[canvas tracks n={n} targets={with_targets}] loss rel {el:.2e} gradient rel_inf {eg:.2e}")
        assert el <= 1e-5, (m, el)
        assert eg <= 1e-4, (m, eg)
    l0, g0 = _canvas_lg(c, bounds=False)  # the broad phase changes no bit
    assert torch.equal(_bits(loss), _bits(l0)) and torch.equal(_bits(grad), _bits(g0))


def _canvas_guide(c, x, x0, mask, bounds, scale, iters, coef, steps, t):
    L = pkg("_lib")
    F = x0.shape[-1]
    M, total = c["off"].numel() - 1, c["fr"].numel()
    mean, std, tg, w, scene, jp, tracks, bnd = (_cu(c[k]) for k in ("mean", "std", "tg", "w", "scene", "jp", "tracks", "bounds"))
    off, fr = c["off"].cuda().to(torch.int32), c["fr"].cuda().to(torch.int32)
    ws = torch.empty(int(L.lib().mdm_canvas_control_workspace_floats(total, F)), device="cuda")
    L.check(L.lib().mdm_canvas_tracks_guidance(_vp(x), _vp(x0), _vp(mask), _vp(off), _vp(fr), _vp(mean), _vp(std), _vp(tg), _vp(w),
                                               _vp(scene), C.c_int32(scene.shape[1]), _vp(jp), _vp(tracks), C.c_int32(tracks.shape[1]),
                                               _vp(bnd if bounds else None), C.c_int32(M), C.c_int32(F), C.c_float(scale),
                                               C.c_int32(iters), _vp(coef), C.c_int32(steps), C.c_void_p(0), C.c_int32(t), _vp(ws),
                                               C.c_void_p(L.stream_ptr())))
    torch.cuda.synchronize()


def test_canvas_guidance_steps_and_bounds():
    """One canvas guidance iteration is x0 - scale grad on the canvas rows, x moves by c0 delta, other rows keep their bits;
    with the balls and with NULL bounds, with and without a mask, x and x0 agree bit for bit."""
    d = _diffusion("ddim10")
    N = d.num_timesteps
    coef = d._device_coef("dpmpp", 0.0, 2, "cuda")
    c = _canvas_case((70, 300), 263, True)
    gen = torch.Generator().manual_seed(11)
    x0, x = c["x"].cuda().contiguous(), torch.randn(c["x"].shape, generator=gen).cuda()
    _, grad = _canvas_lg(c)
    fr = c["fr"].cuda()
    xo, x0o = x.clone(), x0.clone()
    _canvas_guide(c, xo, x0o, None, True, 1e-5, 1, coef, N, 4)
    want = x0.reshape(-1, 263)[fr] - 1e-5 * grad.cuda()
    got = x0o.reshape(-1, 263)[fr]
    assert float((got - want).abs().max()) <= 1e-6 * float(torch.maximum(got.abs(), want.abs()).max())
    delta, c0 = (x0o - x0), float(coef[4, 1])
    big = max(1.0, float(x.abs().max()), abs(c0) * float(delta.abs().max()))
    assert float((xo - x - c0 * delta).abs().max()) <= 1e-6 * big
    other = torch.ones(x0.numel() // 263, dtype=torch.bool, device="cuda")
    other[fr] = False
    assert torch.equal(_bits(x0o.reshape(-1, 263)[other]), _bits(x0.reshape(-1, 263)[other])) and not torch.equal(x0o, x0)
    mask = (torch.rand(x0.shape, generator=gen) < 0.5).float().cuda()
    for m in (None, mask):
        outs = []
        for bounds in (True, False):
            xo, x0o = x.clone(), x0.clone()
            _canvas_guide(c, xo, x0o, m, bounds, 1e-5, 3, coef, N, 4)
            outs.append((xo, x0o))
        assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0])) and torch.equal(_bits(outs[0][1]), _bits(outs[1][1]))
        assert not torch.equal(outs[0][1], x0)
        if m is not None:
            assert torch.equal(_bits(outs[0][1][m == 1]), _bits(x0[m == 1]))


def test_canvas_kernel_equals_the_window_kernel_on_a_short_motion():
    """The (3, 40) case's first sample (40 frames) as a one-motion canvas, its rows in order: the two kernels' summation
    orders differ, so they agree to the gates, not bit for bit; and the Python entry on lists of track stacks."""
    c = _case(3, 40, 263, 5, "targets")
    one = dict(x=c["x0"][:1], off=torch.tensor([0, 40]), fr=torch.arange(40), mean=c["mean"][:1], std=c["std"][:1],
               tg=c["tg"][0], w=c["w"][0], jp=c["jp"][:1], scene=c["scene"][:1], tracks=c["tracks"][0], bounds=c["bounds"][0])
    loss, grad = _canvas_lg(one)
    wl, wg = _tracks_lg(c["x0"][:1], c["lens"][:1], c["mean"][:1], c["std"][:1], c["scene"][:1], c["jp"][:1], c["tracks"][:1],
                        c["bounds"][:1], c["tg"][:1], c["w"][:1])
    el, eg = abs(float(loss[0]) - float(wl[0])) / float(wl[0]), rel_inf(grad, wg[0])
    print(f"[canvas vs window, tracks] loss rel {el:.2e} gradient rel_inf {eg:.2e}")
    assert el <= 1e-5 and eg <= 1e-4
    MS = pkg("motion_scene")
    P = c["P"][0].float()
    trk = [MS.moving_sphere(P[:, 15] + torch.tensor([0.1, 0.0, 0.1]), 0.4), MS.moving_half_space((0, 1, 0), torch.linspace(0, 0.4, 40))]
    l1, g1 = MS.canvas_scene_loss_grad(c["x0"][:1].cuda(), [0, 40], torch.arange(40), c["mean"][0], c["std"][0], None, tracks=[trk])
    l2, g2 = MS.scene_loss_grad(c["x0"][:1].cuda(), [40], c["mean"][0], c["std"][0], None, tracks=trk)
    assert float(l2[0]) > 0 and abs(float(l1[0]) - float(l2[0])) <= 1e-5 * float(l2[0]) and rel_inf(g1.cpu(), g2[0].cpu()) <= 1e-4


# ---- loops --------------------------------------------------------------------------------------------------------------
def _loop_tracks(T):
    """Three obstacles that move through the space the loops_tiny samples live in: a ball that crosses it, a pillar that
    sweeps along X and a floor that rises."""
    MS = pkg("motion_scene")
    t = torch.linspace(0.0, 1.0, T, dtype=torch.float64)
    ball = torch.stack([1.5 - 1.5 * t, torch.full_like(t, 0.4), -0.5 + 2.0 * t], 1)
    foot = torch.stack([-1.0 + 2.0 * t, torch.full_like(t, -1.0), torch.full_like(t, 0.8)], 1)
    return [MS.moving_sphere(ball, 0.6, margin=0.05), MS.moving_capsule(foot, foot + torch.tensor([0.0, 3.0, 0.0]), 0.3, weight=2.0),
            MS.moving_half_space((0.0, 1.0, 0.0), -0.6 + 0.5 * t)]


def _control(B, T, scale=0.001, iters=2):
    """A root path, a static scene and tracks over the loops_tiny batch, as control_* kwargs (CPU tensors)."""
    M, MS = pkg("motion_control"), pkg("motion_scene")
    tg, w = M.root_path_targets(T, [[0.0, 0.0], [1.0, 0.5], [1.5, 2.0]], [0, T // 2, T - 1])
    mean, std = _stats(263, B, 21)
    jp = MS.joint_params(22, [0.03] * 22, [1.0] * 20 + [0.0, 2.0])
    return {"control_joints": tg.expand(B, -1, -1, -1).clone(), "control_weights": w.expand(B, -1, -1, -1).clone(),
            "control_mean": mean, "control_std": std, "control_scale": scale, "control_iters": iters,
            "control_scene": MS.batch_scene(_loop_scene(), B), "control_joint_params": jp[None].expand(B, -1, -1).clone(),
            "control_tracks": MS.batch_tracks(_loop_tracks(T), B, T)}


def _restated(d, mode, m, g, ctl, inputs, scale, eta=0.0, step_noise=None, known=None, mask=None):
    """tests/sampler_ref.py's loop, teacher-forced, with ``iters`` autograd guidance steps down L + L_scene + L_tracks hooked in
    after the edit blend."""
    one_minus_m = 1.0 if mask is None else 1.0 - mask.double()

    def guide(x0):
        for _ in range(ctl["control_iters"]):
            _, gr = TR.ref_tracks_loss_grad(x0, g["length"], ctl["control_mean"], ctl["control_std"], ctl["control_tracks"],
                                            ctl["control_joint_params"], ctl["control_scene"], ctl["control_joints"],
                                            ctl["control_weights"])
            x0 = x0 - ctl["control_scale"] * one_minus_m * gr
        return x0

    return S.loop_ref(d, mode, scale, S.device_eps(m, g["length"]), prompts=[(g["xf_proj"], g["xf_out"])],
                      uncond=m.uncond_embedding(g["x_T"].shape[0], "cuda"), inputs=inputs, eta=eta, step_noise=step_noise,
                      clip=True, known=known, mask=mask, x0_hook=guide)


@pytest.mark.parametrize("mode,eta,edit", [("cfg_dpmpp", 0.0, False), ("ddim", 0.5, False), ("cfg_dpmpp", 0.0, True)])
def test_tracks_loops_match_the_restated_loop(mode, eta, edit):
    g, meta, m, noises, kw = _setup()
    d = _diffusion("ddim10")
    N, sc = d.num_timesteps, meta["cfg_scale"]
    B, T, F_ = g["x_T"].shape
    ctl = _control(B, T)
    ns = noises(f"tracks.{mode}.{eta}", N)
    known = mask = None
    skw = dict(kw, **_cuda(ctl))
    if edit:
        known = pkg("synth").uniform_pm1((B, T, F_), "tracks.known", meta["iseed"])
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
            _check_against_restated(got, want, f"tracks {mode} eta {eta} edit {edit}")
    assert torch.equal(outs[0], outs[1])  # graph == eager
    if edit:
        assert torch.equal(outs[0][mask == 1], known[mask == 1])
    no_tracks = {k: v for k, v in skw.items() if k != "control_tracks"}
    plain = S.run_loop(d, mode, m, no_tracks, sc, eta, True, x_T=g["x_T"].cuda(), step_noise=ns, clip=True).cpu()
    assert not torch.equal(plain, outs[0])
    # the tracks alone: no static scene, no targets
    alone = {k: v for k, v in skw.items() if k not in ("control_joints", "control_weights", "control_scene")}
    out = S.run_loop(d, mode, m, alone, sc, eta, True, x_T=g["x_T"].cuda(), step_noise=ns, clip=True).cpu()
    assert torch.isfinite(out).all() and not torch.equal(out, outs[0])


# ---- the trainer --------------------------------------------------------------------------------------------------------
def _floors(MS, n, heights, **kw):
    """A horizontal floor that moves between ``heights`` over n frames: linear in x0, so a fixed step is stable whatever the
    size of the model's x0 (the trainer samples unclipped; as §24's trainer test)."""
    return MS.moving_half_space((0.0, 1.0, 0.0), torch.linspace(heights[0], heights[1], n), **kw)


def test_trainer_tracks_are_independent_of_the_batch_split():
    MS = pkg("motion_scene")
    g, meta, m, noises, kw = _setup()
    tr = _trainer(m, meta)
    caps = ["a", "b", "c", "d"]
    mean, std = (v[0].numpy() for v in _stats(263, 1, 21))
    ceiling = MS.moving_half_space((0.0, -1.0, 0.0), torch.linspace(-3.0, -2.0, 16))
    tracks = [[_floors(MS, 16, (0.5, 1.0))], [_floors(MS, 16, (1.0, 0.0)), ceiling], [_floors(MS, 12, (0.0, 1.0), margin=0.2)],
              [_floors(MS, 16, (0.2, 0.2))]]
    opts = dict(seed=3, sampler="ddim", sample_steps=10, eta=0.5, scene_tracks=tracks, scene_joint_radius=[0.05] * 22,
                control_scale=0.05, control_iters=2, mean=mean, std=std)
    same = torch.tensor([16, 16, 16, 16])
    one = torch.stack(tr.generate(caps, same, 263, batch_size=1, **opts)).cpu()
    two = torch.stack(tr.generate(caps, same, 263, batch_size=2, **opts)).cpu()
    assert torch.isfinite(one).all() and rel_inf(one, two) < 1e-5, rel_inf(one, two)
    plain = torch.stack(tr.generate(caps, same, 263, batch_size=2, seed=3, sampler="ddim", sample_steps=10, eta=0.5)).cpu()
    assert all(not torch.equal(plain[i], two[i]) for i in range(4))
    shared = torch.stack(tr.generate(caps, same, 263, batch_size=2, **dict(opts, scene_tracks=tracks[0]))).cpu()
    assert rel_inf(shared[0], two[0]) < 1e-5 and not torch.equal(shared[1], two[1])
    # next to a static scene the tracks still count (the trainer's unclipped samples reach heights of hundreds: a floor
    # far below them all)
    both = torch.stack(tr.generate(caps, same, 263, batch_size=2, **dict(opts, scene=[MS.floor(-1e6)]))).cpu()
    assert rel_inf(both, two) < 1e-5
    lens = torch.tensor([8, 16, 12, 4])
    serial = tr.generate(caps, lens, 263, batch_size=2, **opts)
    bucket = tr.generate_bucketed(caps, lens, 263, batch_size=2, unit_length=4, **opts)
    for i, n in enumerate(lens.tolist()):
        assert rel_inf(bucket[i][:n].cpu(), serial[i][:n].cpu()) < 1e-4, i
    ex = {k: v for k, v in opts.items() if k not in ("mean", "std")}
    joints = tr.generate_joints(caps, lens, 263, mean, std, batch_size=2, sigma=0.0, **ex)
    assert [tuple(j.shape) for j in joints] == [(n, 22, 3) for n in lens.tolist()]
    depth, share = MS.penetration(torch.stack([torch.nn.functional.pad(j, (0, 0, 0, 0, 0, 16 - j.shape[0])) for j in joints]),
                                  lens, None, [0.05] * 22, tracks=tracks)
    assert depth.shape == (4,) and share.shape == (4,) and bool(torch.isfinite(depth).all())
    with pytest.raises(ValueError):
        tr.generate(caps, same, 263, batch_size=2, seed=3, scene_tracks=tracks)  # no mean / std


# ---- a long motion ------------------------------------------------------------------------------------------------------
def test_long_motion_with_tracks_matches_the_restated_canvas_loop():
    from test_long_control_gpu import _blend_np, _owner, _run
    M, ML, MS = pkg("motion_control"), pkg("motion_long"), pkg("motion_scene")
    g, meta, m, text, x_T, plans = _long_setup()
    d = _diffusion("ddim10")
    N, scale = d.num_timesteps, meta["cfg_scale"]
    tg, w = M.root_path_targets(CANVAS, [[0.0, 0.0], [1.0, 0.5], [1.5, 2.0]], [0, CANVAS // 2, CANVAS - 1])
    mean, std = _stats(263, 1, 21)
    std[:, 0] = 0.05
    control = ML.canvas_control(plans, 263, [tg], [w], 2e-4, 2, mean[0], std[0], "cpu", [_loop_scene()], [0.03] * 22,
                                scene_tracks=[_loop_tracks(CANVAS)])
    ctl = control([0], TW)
    assert tuple(ctl["canvas_control_tracks"].shape) == (CANVAS, 3, 12) and tuple(ctl["canvas_control_scene"].shape) == (1, 4, 12)
    tab_kw = ML.batch_tables(plans, [0], TW, H, "linear")
    tab = {k[len("handshake_"):]: v.numpy() for k, v in tab_kw.items()}
    kw = {"xf_proj": text["xf_proj"].cuda(), "xf_out": text["xf_out"].cuda(), "length": text["length"].cuda(), **tab_kw}
    fr = ctl["canvas_control_rows"].long()

    def guide(x0):
        flat = x0.clone().reshape(-1, 263)
        c = flat[fr]
        for _ in range(2):
            _, gr = TR.ref_tracks_loss_grad(c[None], [CANVAS], mean[0], std[0], ctl["canvas_control_tracks"][None],
                                            ctl["canvas_control_joint_params"], ctl["canvas_control_scene"], tg[None], w[None])
            c = c - 2e-4 * gr[0]
        flat[fr] = c
        return _owner(flat.view_as(x0), tab)

    for mode, eta in (("cfg_dpmpp", 0.0), ("ddim", 0.5)):
        ns = [pkg("synth").uniform_pm1((2, TW, 263), f"longtracks.{mode}.{i}", meta["iseed"]) * (3.0 ** 0.5) for i in range(N)]
        out, got, got0 = _run(d, mode, m, dict(kw, **_cuda(ctl)), scale, eta, True, x_T, ns)
        assert torch.isfinite(out).all()
        for v in got + got0:
            assert torch.equal(v[0, LENS[0] - H:LENS[0]], v[1, :H])
        want = S.loop_ref(d, mode, scale, S.device_eps(m, text["length"]), prompts=[(text["xf_proj"], text["xf_out"])],
                          uncond=m.uncond_embedding(2, "cuda"), inputs=[_owner(x_T, tab)] + got[:-1], eta=eta, step_noise=ns,
                          clip=True, eps_hook=lambda e: _blend_np(e, tab), noise_hook=lambda z: _owner(z, tab), x0_hook=guide)
        worst = max(rel_inf(got[i], want[i]) for i in range(N))
        print(f"[long tracks] {mode} eta {eta}: worst step rel_inf vs restated canvas loop {worst:.2e}")
        assert worst <= 1e-4, worst
        eager, _, _ = _run(d, mode, m, dict(kw, **_cuda(ctl)), scale, eta, False, x_T, ns)
        assert torch.equal(eager, out)
        no_tracks = {k: v for k, v in ctl.items() if k != "canvas_control_tracks"}
        plain, _, _ = _run(d, mode, m, dict(kw, **_cuda(no_tracks)), scale, eta, True, x_T, ns)
        assert not torch.equal(plain, out)


def test_trainer_generate_long_with_tracks():
    """generate_long(scene_tracks=) on horizontal moving half-spaces (the trainer samples unclipped): independent of the batch
    split, through the joints front end."""
    MS = pkg("motion_scene")
    g, meta, m, text, x_T, plans = _long_setup()
    tr = _trainer(m, meta)
    scripts = [[("walk", 48), ("sit", 40)], [("jump", 44)], [("run", 44), ("stop", 48)]]
    mean, std = np.zeros(263, np.float32), np.ones(263, np.float32)
    std[0] = 0.05
    ceiling = MS.moving_half_space((0.0, -1.0, 0.0), torch.linspace(-3.0, -2.0, 44))
    tracks = [[_floors(MS, 68, (0.0, 1.0))], [_floors(MS, 44, (0.5, 0.0)), ceiling], [_floors(MS, 60, (0.3, 0.0), margin=0.3)]]
    opts = dict(overlap=20, seed=3, sampler="ddim", sample_steps=10, eta=0.5, scene_tracks=tracks, scene_joint_radius=[0.05] * 22,
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
        tr.generate_long(scripts, 263, mean=mean, std=std, **dict(opts, scene_tracks=tracks[0]))  # one list, not one per motion


# ---- several characters -------------------------------------------------------------------------------------------------
def _crossing(T, weight_free=False):
    """Two characters on straight pelvis paths that cross at (1, 0) in the middle of the clip, targets in the world."""
    M = pkg("motion_control")
    a, wa = M.root_path_targets(T, [[0.0, 0.0], [2.0, 0.0]], [0, T - 1])
    b, wb = M.root_path_targets(T, [[1.0, -1.0], [1.0, 1.0]], [0, T - 1])
    return [[dict(caption="walk east", length=T, control_joints=a, control_weights=wa),
             dict(caption="walk north", length=T, position=(1.0, -1.0), yaw=0.0, control_joints=b, control_weights=wb)]]


def _together_stats():
    """The trainer samples unclipped and the seeded loops_tiny weights give rows of size hundreds, so the de-normalisation
    brings them to a body's size: std 0.002 (root velocity, height: steps of a few decimetres a frame), 0.0005 for the joint
    columns (a body about 1.2 m across) and 0.05 x 0.002 for the heading velocity, as the window tests' 0.05 at std 1."""
    mean, std = np.zeros(263, np.float32), np.full(263, 0.002, np.float32)
    std[0], std[4:67] = 0.05 * 0.002, 0.0005
    return mean, std


def _together_opts():
    """§14's step for the window tests, 0.002 at std 1: the curvature goes with std^2, so 0.002 / 0.002^2 here."""
    return dict(sampler="ddim", sample_steps=20, control_scale=0.002 / 0.002 ** 2, control_iters=8, sigma=0.0, seed=7, batch_size=4)


def test_generate_together_one_character_and_independence():
    MS = pkg("motion_scene")
    g, meta, m, noises, kw = _setup()
    tr = _trainer(m, meta)
    mean, std = _together_stats()
    T = 16
    two = _crossing(T)
    solo = [[dict(two[0][0], position=(0.5, -0.25), yaw=0.3)]]
    out = tr.generate_together(solo, 263, mean, std, **_together_opts())
    tg = MS.to_local(two[0][0]["control_joints"], (0.5, -0.25), 0.3)
    ref = tr.generate_joints(["walk east"], torch.tensor([T]), 263, mean, std, control_joints=tg[None],
                             control_weights=two[0][0]["control_weights"][None], **_together_opts())
    want = MS.to_world(ref[0], (0.5, -0.25), 0.3)
    assert tuple(out[0][0].shape) == (T, 22, 3) and torch.equal(_bits(out[0][0].cpu()), _bits(want.cpu()))
    # character 0 does not depend on character 1, nor on the other scenes of the call
    pair = tr.generate_together(two + [[dict(caption="walk east", length=12)]], 263, mean, std, radius=0.3, **_together_opts())
    alone = tr.generate_together([two[0][:1]], 263, mean, std, **_together_opts())
    # (another batch: to rounding, as the trainer's batch splits)
    assert rel_inf(pair[0][0].cpu(), alone[0][0].cpu()) < 1e-4 and len(pair[0]) == 2 and len(pair[1]) == 1
    assert tuple(pair[0][1].shape) == (T, 22, 3) and bool(torch.isfinite(pair[0][1]).all()) and tuple(pair[1][0].shape) == (12, 22, 3)
    free = tr.generate_together(two, 263, mean, std, radius=0.3, weight=0.0, **_together_opts())
    assert torch.equal(_bits(free[0][0].cpu()), _bits(pair[0][0].cpu())) and not torch.equal(free[0][1], pair[0][1])


# ---- behaviour ----------------------------------------------------------------------------------------------------------
# L_tracks of the final sample with scene_tracks= over L_tracks without, the larger of the samples, measured on an MI355X
# (DESIGN.md §25), and its gate: 4 x the measurement (the project's margin for seed-to-seed spread), never above 0.5
MOVING_RATIO_MEASURED = 0.384
MOVING_RATIO_GATE = 0.5 if MOVING_RATIO_MEASURED is None else min(4 * MOVING_RATIO_MEASURED, 0.5)


def test_a_moving_obstacle_on_the_path_is_avoided():
    """The setting of test_an_obstacle_on_the_path_is_avoided (loops_tiny, guided DDIM-20, x0 clipped, a pelvis path (0, 0) ->
    (2, 0) -> (2, 2), mean 0, std 1 except the heading velocity's 0.05, control_scale 0.002, control_iters 8); in place of the
    pillar a sphere of radius 0.3 rolls across the path along Z at 0.3 m a frame and is at (1, 0), at the height the pelvis of
    the run without it has there, in the frame in which the path's pelvis is: L_tracks of the final sample with
    scene_tracks= against the run without (the path alone).  The weight follows §14's rule scale x curvature < 2 for a
    primitive that moves: the ball is in reach of a joint for about n_c = 3 frames around frame t = 4 and
    of about J_c = 3 joints, and its force reaches the root velocities of the t frames before, a curvature of about
    2 a J_c n_c t = 72 a, so a < 2 / (0.002 x 72) = 14: a = 10."""
    M, MS = pkg("motion_control"), pkg("motion_scene")
    g, meta, m, noises, kw = _setup()
    d = _diffusion("ddim20")
    B, T, F_ = g["x_T"].shape
    tg, w = M.root_path_targets(T, [[0.0, 0.0], [2.0, 0.0], [2.0, 2.0]], [0, T // 2, T - 1])
    mean, std = torch.zeros(B, F_), torch.ones(B, F_)
    std[:, 0] = 0.05
    meet = int((tg[:, 0, 0] - 1.0).abs().argmin())  # the frame in which the path's pelvis is at (1, 0)
    assert float(tg[meet, 0, 0]) == pytest.approx(1.0, abs=0.13) and float(tg[meet, 0, 2]) == 0.0
    t = torch.arange(T, dtype=torch.float64)
    ctl = {"control_joints": tg.expand(B, -1, -1, -1).clone(), "control_weights": w.expand(B, -1, -1, -1).clone(),
           "control_mean": mean, "control_std": std, "control_scale": 0.002, "control_iters": 8}
    outs = {"path": d.ddim_sample_loop_with_cfg(m, (B, T, F_), clip_denoised=True, model_kwargs=dict(kw, **_cuda(ctl)),
                                                cfg_scale=2.5, seed=7)}
    tracks = []
    for b in range(B):  # one ball per sample, at its own pelvis' height
        height = float(ref_positions(outs["path"][b].cpu().double(), mean[b].double(), std[b].double())[meet, 0, 1])
        ball = torch.stack([torch.ones(T, dtype=torch.float64), torch.full((T,), height, dtype=torch.float64), 0.3 * (t - meet)], 1)
        tracks.append([MS.moving_sphere(ball, 0.3, margin=0.05, weight=10.0)])
    trk = {"control_tracks": MS.batch_tracks(tracks, B, T)}
    outs["tracks"] = d.ddim_sample_loop_with_cfg(m, (B, T, F_), clip_denoised=True, model_kwargs=dict(kw, **_cuda(ctl), **_cuda(trk)),
                                                 cfg_scale=2.5, seed=7)
    ls = {k: MS.scene_loss_grad(v, g["length"], mean, std, None, tracks=tracks)[0].cpu() for k, v in outs.items()}
    lp = {k: M.joint_loss_grad(v, g["length"], mean, std, ctl["control_joints"], ctl["control_weights"])[0].cpu()
          for k, v in outs.items()}
    ratio = ls["tracks"] / ls["path"]
    print(f"[moving] L_tracks without scene_tracks= {ls['path'].tolist()} with {ls['tracks'].tolist()} ratio {ratio.tolist()}; "
          f"path loss without {lp['path'].tolist()} with {lp['tracks'].tolist()}")
    assert bool((ls["path"] > 0).all())
    assert bool((ratio <= MOVING_RATIO_GATE).all()), ratio


# the second character's deepest penetration of the first with avoidance over that with weight = 0, measured the same way
TOGETHER_RATIO_MEASURED = 0.198
TOGETHER_RATIO_GATE = 0.5 if TOGETHER_RATIO_MEASURED is None else min(4 * TOGETHER_RATIO_MEASURED, 0.5)


def test_two_characters_on_crossing_paths_keep_apart():
    """generate_together with two characters whose straight pelvis paths cross at (1, 0) in the middle of the clip (guided
    DDIM-20, the de-normalisation and step of _together_stats / _together_opts, control_iters 8, capsules of radius 0.3 around
    the first character's bones, margin 0.05, weight 5: the pillar's of §24, by its reasoning, the force reaching the root
    path): ``penetration`` of character 1 into character 0's tracks with avoidance against the same call with weight = 0.
    Character 0 is the same in both."""
    MS = pkg("motion_scene")
    g, meta, m, noises, kw = _setup()
    tr = _trainer(m, meta)
    mean, std = _together_stats()
    T = 16
    res = {wt: tr.generate_together(_crossing(T), 263, mean, std, radius=0.3, margin=0.05, weight=wt, **_together_opts())
           for wt in (5.0, 0.0)}
    assert torch.equal(res[5.0][0][0], res[0.0][0][0])
    body = MS.character_tracks(res[5.0][0][0], 0.3, margin=0.05)
    depth = {wt: float(MS.penetration(r[0][1][None], [T], None, tracks=body)[0][0]) for wt, r in res.items()}
    share = {wt: float(MS.penetration(r[0][1][None], [T], None, tracks=body)[1][0]) for wt, r in res.items()}
    ratio = depth[5.0] / depth[0.0] if depth[0.0] > 0 else float("inf")
    print(f"[together] deepest penetration of character 1 into character 0: weight 0 {depth[0.0]:.4f} m (share of frames "
          f"{share[0.0]:.3f}), weight 5 {depth[5.0]:.4f} m (share {share[5.0]:.3f}), ratio {ratio:.3e}")
    assert depth[0.0] > 0
    assert ratio <= TOGETHER_RATIO_GATE, ratio

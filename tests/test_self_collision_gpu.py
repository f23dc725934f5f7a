"""GPU: self-collision avoidance against the fp64 restatement of tests/self_collision_ref.py.

* mdm_self_push: push vectors and depths against fp64 on poses that really penetrate (placement asserted in
  tests/test_self_collision_host.py); zeros past a length and under an empty mask; two runs bit-equal.
* mdm_self_targets: the joints are postprocess.recover_from_ric's bits, the targets joints + push bit for bit, the weights
  weight * u_j or 0, the static pair wins bit for bit, weight 0 gives zero weights.
* one mdm_joint_guidance step on the produced targets against one fp64 autograd step of L_self plus a root-path term.
* loops on loops_tiny: graph == eager bitwise, per-step rel_inf against the teacher-forced restated loop.
* the bitwise no-ops, the effect on final samples, and every argument error of the two entries.

Gates.  PUSH_GATE is four times the largest error measured on an MI355X (DESIGN.md §33 records it, as §31 records its record
ends'); the step and loop gates are the project's per-step 1e-4 rel_inf; the effect gate is min(4 x the measured ratio, 0.5),
the convention of §24, §25 and §31."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import sampler_ref as S
import self_collision_ref as SR
from conftest import pkg, rel_inf
from sampler_ref import caption_trainer as _trainer, loops_setup as _setup, make_diffusion as _diffusion, vp as _vp
from test_motion_control_host import ref_positions

pytestmark = pytest.mark.gpu

# the largest |push - fp64| and |depth - fp64| over the cases below, in metres, measured on an MI355X
PUSH_ERR_MEASURED = 8.46e-7  # the push at (2, 196), F = 263; the depth stays under 1.12e-7
PUSH_GATE = 4 * PUSH_ERR_MEASURED


def _bits(v):
    return v.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a.cpu().float()), _bits(b.cpu().float()))


# ---- mdm_self_push ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,F", SR.CASES)
def test_push_and_depth_match_fp64(B, T, F):
    MS = pkg("motion_scene")
    c = SR.case(B, T, F)
    P32 = c["P"].float()
    want_push, want_depth = SR.push_depth(P32, c["lens"], c["body"])  # fp64 on the fp32 joints the kernel is given
    push, depth = MS.self_push(P32.cuda(), c["lens"], c["body"])
    ep, ed = float((push.cpu().double() - want_push).abs().max()), float((depth.cpu().double() - want_depth).abs().max())
    print(f"[self push B={B} T={T} F={F}] push against fp64 {ep:.3e} m, depth {ed:.3e} m (largest push {float(want_push.abs().max()):.3f} m, "
          f"depth {float(want_depth.max()):.3f} m)")
    assert float(want_depth.max()) > 0.01
    assert ep <= PUSH_GATE and ed <= PUSH_GATE, (ep, ed)
    assert torch.equal((depth.cpu() > 0), (want_depth > 0))  # the placement keeps every pair 1e-3 m from pen = 0
    for b in range(B):
        n = int(c["lens"][b])
        assert float(push[b, n:].abs().sum()) == 0.0 and float(depth[b, n:].abs().sum()) == 0.0
    again = MS.self_push(P32.cuda(), c["lens"], c["body"])
    assert _same(again[0], push) and _same(again[1], depth)
    none = MS.self_body(MS.default_offsets(SR.SKELETON[F]), SR.SKELETON[F], pairs=np.zeros((c["J"], c["J"] - 1), dtype=bool))
    z = MS.self_push(P32.cuda(), c["lens"], none)
    assert float(z[0].abs().sum()) == 0.0 and float(z[1].abs().sum()) == 0.0


# ---- mdm_self_targets ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,F", SR.CASES)
def test_targets_are_joints_plus_push_and_the_static_pair_wins(B, T, F):
    MS, PP = pkg("motion_scene"), pkg("postprocess")
    c = SR.case(B, T, F)
    body, lens, J = c["body"], c["lens"], c["J"]
    x0 = c["x0"].cuda()
    tg, w, joints = MS.self_targets(x0, lens, c["mean"], c["std"], body, SR.WEIGHT, return_joints=True)
    rows = x0 * c["std"].cuda()[:, None] + c["mean"].cuda()[:, None]
    want = torch.zeros_like(joints)
    for b in range(B):
        n = int(lens[b])
        want[b, :n] = PP.recover_from_ric(rows[b, :n], J)
    assert _same(joints, want)  # postprocess.recover_from_ric of the de-normalised x0, bit for bit
    push, depth = MS.self_push(joints, lens, body)
    assert _same(tg, joints + push)
    u = body.joint_params[:, 1].cuda()
    wj = torch.where(depth > 0, (torch.tensor(SR.WEIGHT) * u)[None, None].expand_as(depth), torch.zeros_like(depth))
    assert _same(w, wj[..., None].expand(-1, -1, -1, 3))
    assert float((w > 0).float().mean()) > 0.02
    e = float((tg.cpu().double() - c["targets"]).abs().max())
    print(f"[self targets B={B} T={T} F={F}] targets against fp64 {e:.3e} m")
    # P itself carries the recovery's fp32 prefix sums: up to T = 196 roundings of 2^-24 of a root position of a few metres,
    # 196 x 6e-8 x 3 = 3.5e-5 m at the most; measured 3.8e-6 m
    assert e <= 4e-5 and torch.equal(w.cpu().double(), c["weights"])
    # the static pair: bit for bit wherever it carries a weight and past the lengths, the produced pair elsewhere
    sg, sw = (v.cuda() for v in c["static"])
    tgs, ws = MS.self_targets(x0, lens, c["mean"], c["std"], body, SR.WEIGHT, sg, sw)
    live = (torch.arange(T)[None] < lens[:, None]).cuda()[..., None]
    user = ((sw != 0).any(-1) | ~live)[..., None].expand_as(sg)
    assert bool((user & live[..., None] & (depth > 0)[..., None]).any())  # one of them sits on a penetrating joint
    assert torch.equal(_bits(tgs)[user], _bits(sg)[user]) and torch.equal(_bits(ws)[user], _bits(sw)[user])
    assert torch.equal(_bits(tgs)[~user], _bits(tg)[~user]) and torch.equal(_bits(ws)[~user], _bits(w)[~user])
    assert torch.equal(ws.cpu().double(), c["weights_static"])
    # weight 0 and no static pair: no weight anywhere
    tg0, w0 = MS.self_targets(x0, lens, c["mean"], c["std"], body, 0.0)
    assert float(w0.abs().sum()) == 0.0 and _same(tg0, tg)


# ---- one guidance step -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [263, 251])
def test_one_guidance_step_is_one_step_down_l_self_and_the_root_path(F):
    L, MS, M = pkg("_lib"), pkg("motion_scene"), pkg("motion_control")
    B, T = 3, 40
    c = SR.case(B, T, F)
    body, lens, J = c["body"], c["lens"], c["J"]
    d = _diffusion("ddim10")
    coef = d._device_coef("ddim", 0.0, 2, "cuda")
    t, scale = 4, 0.002
    path, pw = M.root_path_targets(T, [[0.0, 0.0], [1.0, 0.5], [1.5, 2.0]], [0, T // 2, T - 1], joints_num=J)
    sg, sw = path.expand(B, -1, -1, -1).clone(), pw.expand(B, -1, -1, -1).clone()
    x0 = c["x0"].cuda()
    x = torch.randn(B, T, F, generator=torch.Generator().manual_seed(F)).cuda()
    mean, std = c["mean"].cuda().contiguous(), c["std"].cuda().contiguous()
    tg, w = MS.self_targets(x0, lens, mean, std, body, SR.WEIGHT, sg.cuda(), sw.cuda())
    xo, x0o = x.clone(), x0.clone()
    L.check(L.lib().mdm_joint_guidance(_vp(xo), _vp(x0o), None, _vp(lens.to(torch.int32).cuda()), _vp(mean), _vp(std), _vp(tg), _vp(w),
                                       B, T, F, scale, 1, _vp(coef), d.num_timesteps, None, t, L.stream_ptr()), "mdm_joint_guidance")
    worst = of_step = 0.0
    for b in range(B):
        n = int(lens[b])
        xb = c["x0"][b, :n].double().clone().requires_grad_(True)
        P = ref_positions(xb, c["mean"][b], c["std"][b])
        own = (sw[b, :n] != 0).any(-1)  # the user's target wins on its joints: L_self counts the others
        pen = SR.pens(P, body)[0]
        loss = SR.WEIGHT * (body.joint_params[:, 1].double()[None, :, None] * pen * pen)[~own].sum()
        loss = loss + (sw[b, :n].double() * (P - sg[b, :n].double()) ** 2).sum()
        loss.backward()
        want = c["x0"][b].double().clone()
        want[:n] -= scale * xb.grad
        e = rel_inf(x0o[b].cpu(), want)
        worst = max(worst, e)
        of_step = max(of_step, float((x0o[b].cpu().double() - want).abs().max()) / float((want - c["x0"][b].double()).abs().max()))
        assert float((want - c["x0"][b].double()).abs().max()) > 1e-3  # the step moves the row
        delta = (x0o[b] - x0[b]).double()
        assert float((xo[b].double() - x[b].double() - float(coef[t, 1]) * delta).abs().max()) <= 1e-6 * max(1.0, float(x.abs().max()))
    print(f"[self step F={F}] one guidance step on the produced targets against one fp64 step of L_self + root path: rel_inf {worst:.2e} "
          f"({of_step:.2e} of the largest move)")
    assert worst <= 1e-4


# ---- loops -----------------------------------------------------------------------------------------------------------------
from test_motion_scene_gpu import _check_against_restated, _control, _cuda  # noqa: E402

LOOP_RADIUS_SCALE, LOOP_WEIGHT = 2.0, 2.0


def _loop_control(B, T, extra):
    """The control kwargs of a loop over loops_tiny (CPU tensors) and the body: self-collision alone, or on top of
    test_motion_scene_gpu._control's root path and static scene."""
    ctl = _control(B, T)
    if extra == "alone":
        ctl = {k: ctl[k] for k in ("control_mean", "control_std", "control_scale", "control_iters")}
    return ctl, SR.body_of(263, LOOP_RADIUS_SCALE)


@pytest.mark.parametrize("extra", ["alone", "path_scene"])
@pytest.mark.parametrize("mode,eta,edit", [("cfg_dpmpp", 0.0, False), ("ddim", 0.5, False), ("cfg_dpmpp", 0.0, True)])
def test_self_loops_match_the_restated_loop(mode, eta, edit, extra):
    g, meta, m, noises, kw = _setup()
    d = _diffusion("ddim10")
    N, sc = d.num_timesteps, meta["cfg_scale"]
    B, T, F_ = g["x_T"].shape
    ctl, body = _loop_control(B, T, extra)
    ns = noises(f"self.{mode}.{eta}", N)
    known = mask = None
    skw = dict(kw, **_cuda(ctl), control_self={"body": body, "weight": LOOP_WEIGHT})
    if edit:
        known = pkg("synth").uniform_pm1((B, T, F_), "self.known", meta["iseed"])
        mask = torch.broadcast_to(pkg("motion_edit").inbetween_mask(T, 3, 4), (B, T, F_))
        skw.update(inpaint_motion=known.cuda(), inpaint_mask=mask.cuda())
    outs, seen = [], []
    for use_graph in (True, False):
        got = []
        out = S.run_loop(d, mode, m, skw, sc, eta, use_graph, x_T=g["x_T"].cuda(), step_noise=ns, clip=True,
                         cb=lambda i, t, x: got.append(x.clone().cpu())).cpu()
        assert len(got) == N and torch.equal(out, got[-1]) and torch.isfinite(out).all()
        outs.append(out)
        if use_graph:
            hook = SR.guidance_hook(g["length"], ctl, body, LOOP_WEIGHT, mask, seen)
            want = S.loop_ref(d, mode, sc, S.device_eps(m, g["length"]), prompts=[(g["xf_proj"], g["xf_out"])],
                              uncond=m.uncond_embedding(B, "cuda"), inputs=[g["x_T"]] + got[:-1], eta=eta, step_noise=ns, clip=True,
                              known=known, mask=mask, x0_hook=hook)
            share, axis = max(s for s, _ in seen), min(a for _, a in seen)
            print(f"[self loop {mode} eta {eta} edit {edit} {extra}] largest share of a row's (t, j) penalised in a step {share:.3f}, "
                  f"least distance of a penalised pair to its bone's axis {axis:.2e} m")
            assert share >= 0.10, share  # on the restated states alone: the body bites
            _check_against_restated(got, want, f"self {mode} eta {eta} edit {edit} {extra}")
    assert torch.equal(outs[0], outs[1])  # graph == eager
    if edit:
        assert torch.equal(outs[0][mask == 1], known[mask == 1])
    if extra == "path_scene":
        plain = S.run_loop(d, mode, m, {k: v for k, v in skw.items() if k != "control_self"}, sc, eta, True, x_T=g["x_T"].cuda(),
                           step_noise=ns, clip=True).cpu()
        assert not torch.equal(plain, outs[0])


# ---- bitwise no-ops --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tr():
    g, meta, m, noises, kw = _setup()
    return _trainer(m, meta)


def test_no_ops_are_bitwise():
    MS = pkg("motion_scene")
    g, meta, m, noises, kw = _setup()
    d = _diffusion("ddim10")
    B, T, F_ = g["x_T"].shape
    ctl = _control(B, T)
    run = lambda k: S.run_loop(d, "cfg_dpmpp", m, k, meta["cfg_scale"], 0.0, True, x_T=g["x_T"].cuda(), clip=True).cpu()  # noqa: E731
    base = run(dict(kw, **_cuda(ctl)))
    body = SR.body_of(263, LOOP_RADIUS_SCALE)
    assert torch.equal(run(dict(kw, **_cuda(ctl), control_self={"body": body, "weight": 0.0})), base)
    assert torch.equal(run(dict(kw, **_cuda(ctl), control_self=None)), base)
    # a body nothing can enter: the producer runs, every produced weight is 0, and the guidance sees the user's pair alone
    thin = MS.self_body(MS.default_offsets("t2m"), "t2m", radii=np.full(22, 1e-6), margin=-100.0)
    assert bool(thin.allowed.any())
    assert torch.equal(run(dict(kw, **_cuda(ctl), control_self={"body": thin, "weight": 5.0})), base)
    assert not torch.equal(run(dict(kw, **_cuda(ctl), control_self={"body": body, "weight": LOOP_WEIGHT})), base)
    # without any control the key at weight 0 is the plain call, whatever mean / std say
    plain = run(kw)
    stats = {k: ctl[k].cuda() for k in ("control_mean", "control_std")}
    assert torch.equal(run(dict(kw, **stats, control_self={"body": body, "weight": 0.0})), plain)
    # through the trainer
    tr = _tr()
    mean, std = _effect_stats()
    args = (["a person walks", "a person sits"], torch.tensor([16, 12]), 263)
    opts = dict(sampler="ddim", sample_steps=10, seed=3, batch_size=4)
    ref = tr.generate(*args, **opts)
    for off in (None, dict(weight=0.0)):
        out = tr.generate(*args, mean=mean, std=std, self_collision=off, **opts)
        assert all(_same(a, b) for a, b in zip(out, ref))
    assert MS.self_max_frames() == MS.SELF_MAX_FRAMES


# ---- effect ----------------------------------------------------------------------------------------------------------------
# L_self of the final joints with self_collision over L_self without it (what the parent commit produces), measured on an
# MI355X, and its gate: 4 x the measurement, never above 0.5
EFFECT_RATIO_MEASURED = 0.01436
EFFECT_RATIO_GATE = 0.5 if EFFECT_RATIO_MEASURED is None else min(4 * EFFECT_RATIO_MEASURED, 0.5)
EFFECT_SCALE, EFFECT_WEIGHT = 2e5, 5.0


def _effect_stats():
    """The trainer samples unclipped and the seeded loops_tiny weights give rows of size hundreds: std 0.0005 on the joint
    columns and the height brings them to a body about 1.2 m across (tests/test_scene_tracks_gpu.py), and a root that all but
    stands (1e-5 a frame, heading 1e-6) keeps the curvature of the root path, which every pushed joint of every later frame
    feeds, under that of a joint's own columns: by §14's rule the step is then set by 2 a std^2 = 2.5e-6 at a = 5,
    2e5 x 2.5e-6 = 0.5 < 2."""
    mean, std = np.zeros(263, np.float32), np.full(263, 0.0005, np.float32)
    std[0], std[1:3] = 1e-6, 1e-5
    return mean, std


def test_wrists_and_knees_leave_the_body():
    """A wrist folded across the trunk: a keyframe path pulls the left *elbow* to the spine, so that the forearm and the wrist,
    which carry no target, are free to be pushed.  L_self of the final joints with self_collision over that without."""
    MS = pkg("motion_scene")
    tr = _tr()
    mean, std = _effect_stats()
    T, elbow = 16, 18
    tg, w = torch.zeros(1, T, 22, 3), torch.zeros(1, T, 22, 3)
    tg[0, 4:12, elbow], w[0, 4:12, elbow] = torch.tensor([0.0, 0.2, 0.05]), 1.0
    opts = dict(sampler="ddim", sample_steps=20, control_scale=EFFECT_SCALE, control_iters=8, sigma=0.0, seed=7, batch_size=4,
                control_joints=tg, control_weights=w)
    body = MS.self_body(MS.default_offsets("t2m"), "t2m")
    res = {}
    for name, own in (("without", None), ("with", dict(weight=EFFECT_WEIGHT))):
        j = tr.generate_joints(["a person folds the arms"], torch.tensor([T]), 263, mean, std, self_collision=own, **opts)[0]
        assert tuple(j.shape) == (T, 22, 3) and torch.isfinite(j).all()
        depth, share = MS.self_penetration(j[None], [T], body)
        res[name] = (float(SR.l_self(j.cpu().double(), body, 1.0)), float(depth[0]), float(share[0]),
                     float((j[4:12, elbow].cpu() - tg[0, 4:12, elbow]).norm(dim=-1).mean()))
    ratio = res["with"][0] / res["without"][0] if res["without"][0] > 0 else float("inf")
    print(f"[self effect] L_self / a of the final joints: without {res['without'][0]:.4f}, with {res['with'][0]:.4f}, ratio {ratio:.3e}; "
          f"deepest single-pair penetration {res['without'][1]:.4f} -> {res['with'][1]:.4f} m; share of (t, j) inside a margin "
          f"{res['without'][2]:.3f} -> {res['with'][2]:.3f}; mean elbow distance to its target {res['without'][3]:.4f} -> {res['with'][3]:.4f} m")
    assert res["without"][0] > 0 and res["without"][1] > 0
    assert ratio <= EFFECT_RATIO_GATE, ratio


# ---- arguments -------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    L, MS = pkg("_lib"), pkg("motion_scene")
    lib = L.lib()
    c = SR.case(1, 2, 263)
    body = c["body"]
    B, T, F, J = 1, 2, 263, 22
    x0, mean, std = c["x0"].cuda(), c["mean"].cuda(), c["std"].cuda()
    lens = c["lens"].to(torch.int32).cuda()
    rho, jp, mask = body.on("cuda")
    joints, tg, w = (torch.full((B, T, J, 3), 7.0).cuda() for _ in range(3))
    scratch = torch.empty(MS.self_scratch_floats(B, T, F)).cuda()
    depth = torch.full((B, T, J), 7.0).cuda()
    inf, nan = float("inf"), float("nan")

    def push(**o):
        a = dict(joints=joints, length=lens, bones=body.bones, nb=body.nb, rho=rho, jp=jp, mask=mask, margin=0.02, B=B, T=T, J=J,
                 out=tg, depth=depth)
        a.update(o)
        return lib.mdm_self_push(_vp(a["joints"]), _vp(a["length"]), _vp(a["bones"]), a["nb"], _vp(a["rho"]), _vp(a["jp"]), _vp(a["mask"]),
                                 a["margin"], a["B"], a["T"], a["J"], _vp(a["out"]), _vp(a["depth"]), L.stream_ptr())

    def targets(**o):
        a = dict(x0=x0, length=lens, mean=mean, std=std, bones=body.bones, nb=body.nb, rho=rho, jp=jp, mask=mask, margin=0.02, weight=5.0,
                 sg=None, sw=None, B=B, T=T, F=F, joints=joints, scratch=scratch, tg=tg, w=w)
        a.update(o)
        return lib.mdm_self_targets(_vp(a["x0"]), _vp(a["length"]), _vp(a["mean"]), _vp(a["std"]), _vp(a["bones"]), a["nb"], _vp(a["rho"]),
                                    _vp(a["jp"]), _vp(a["mask"]), a["margin"], a["weight"], _vp(a["sg"]), _vp(a["sw"]), a["B"], a["T"],
                                    a["F"], _vp(a["joints"]), _vp(a["scratch"]), _vp(a["tg"]), _vp(a["w"]), L.stream_ptr())

    bad_bone = body.bones.clone()
    bad_bone[3, 1] = J
    neg_bone = body.bones.clone()
    neg_bone[0, 0] = -1
    for o in (dict(joints=None), dict(length=None), dict(bones=None), dict(rho=None), dict(jp=None), dict(mask=None), dict(out=None),
              dict(J=1), dict(J=33), dict(nb=0), dict(nb=32), dict(bones=bad_bone), dict(bones=neg_bone), dict(margin=nan),
              dict(margin=inf), dict(B=-1), dict(T=-1)):
        assert push(**o) == 1, o
    for o in (dict(x0=None), dict(length=None), dict(mean=None), dict(std=None), dict(bones=None), dict(rho=None), dict(jp=None),
              dict(mask=None), dict(joints=None), dict(scratch=None), dict(tg=None), dict(w=None), dict(nb=0), dict(nb=32),
              dict(bones=bad_bone), dict(bones=neg_bone), dict(F=262), dict(F=12 * 33 - 1), dict(F=11), dict(sg=tg), dict(sw=w),
              dict(margin=nan), dict(weight=nan), dict(weight=inf), dict(weight=-1.0), dict(B=-1)):
        assert targets(**o) == 1, o
    assert targets(T=MS.self_max_frames() + 1) == 3  # MDM_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    for v in (joints, tg, w, depth):  # every refusal came before a launch
        assert bool((v == 7.0).all())
    assert push(B=0) == 0 and push(T=0) == 0 and targets(B=0) == 0 and targets(T=0) == 0
    torch.cuda.synchronize()
    assert bool((tg == 7.0).all()) and bool((w == 7.0).all())
    assert push(depth=None) == 0  # the depth is optional
    assert MS.self_scratch_floats(3, 40, 263) == 3 * 40 * (67 + 66) + 2 * 67 and MS.self_scratch_floats(3, 40, 262) == 0
    with pytest.raises(ValueError):
        MS.self_targets(x0, c["lens"], mean, std, body, 5.0, static_targets=tg)
    with pytest.raises(ValueError):
        MS.self_targets(x0, c["lens"], mean, std, body, -1.0)
    with pytest.raises(ValueError):
        MS.self_targets(c["x0"][..., :251].cuda(), c["lens"], mean[:, :251], std[:, :251], body, 1.0)

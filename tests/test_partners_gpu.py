"""GPU: characters sampled together: mdm_partner_tracks, the launch that turns a step's x0 of a whole batch into
the capsule tracks every row's partners avoid and the contact targets they reach for.

* records and contact targets against the fp64 restatement of tests/partners_ref.py: (B, T) = (3, 2) and (4, 40) with lengths
  (40, 28, 40, 17) at F = 263 and 251, two scenes of two and one scene of three with a bone subset (Km = 24), behind Ks = 0 and
  Ks = 3 static tracks (one a half-space), and (2, 196) with Km = 24; end points and targets in metres, header floats and the
  all-zero records of empty slots and of frames past either length bit for bit; the placement is asserted on the reference
  alone in tests/test_partners_host.py;
* the world-joint scratch is `to_world` in fp32 of `postprocess.recover_from_ric`, bit for bit at placement (0, 0, 0);
* the balls contain every live keep-out record in fp64, +-inf as specified, and mdm_joint_tracks_guidance with them equals
  NULL bounds bit for bit, with and without an edit mask; two runs give the same bits;
* the argument errors of the C entry and of the Python layers.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import partners_ref as PR
from conftest import pkg
from sampler_ref import make_diffusion as _diffusion, vp as _vp

pytestmark = pytest.mark.gpu

# the largest absolute error of a record end point or a contact target against fp64, in metres, measured on an MI355X
# (DESIGN.md §31), and its gate: 4 x the measurement, never above a tenth of a millimetre
RECORD_ERR_MEASURED = 1.24e-6
RECORD_ERR_GATE = 1e-4 if RECORD_ERR_MEASURED is None else min(4 * RECORD_ERR_MEASURED, 1e-4)


def _bits(v):
    return v.contiguous().view(torch.int32)


def _run(c, **kw):
    MS = pkg("motion_scene")
    return MS.partner_tracks(c["x0"].cuda(), c["lens"], c["mean"], c["std"], c["tables"], c["static"], **kw)


@pytest.mark.parametrize("B,T,F,layout,Ks", PR.CASES)
def test_records_and_targets_match_fp64(B, T, F, layout, Ks):
    c = PR.case(B, T, F, layout, Ks)
    t = c["tables"]
    tracks, bounds, targets = (v.cpu() for v in _run(c))
    ref = c["rec"]
    live = ref[..., 0] != 0
    part = torch.zeros_like(live)
    part[:, :, Ks:] = True
    # end points of the partner capsules, in metres
    e_rec = float((tracks.double() - ref)[live & part][:, 4:10].abs().max())
    # every other float of a live partner record, all of an absent one and all of a static one: bit for bit
    head = [0, 1, 2, 3, 10, 11]
    assert torch.equal(_bits(tracks[live & part][:, head]), _bits(ref.float()[live & part][:, head]))
    assert torch.equal(_bits(tracks[~live]), torch.zeros_like(_bits(tracks[~live])))
    assert int((~live & part).sum()) > 0  # frames past a length and empty slots are among them
    if Ks:
        assert torch.equal(_bits(tracks[:, :, :Ks]), _bits(c["static"]))
    # contact targets where a contact lands, exact zeros everywhere else (the call writes nothing there)
    hit = c["hit"]
    assert bool(hit.any())
    e_tg = float((targets.double() - c["tg"])[hit].abs().max())
    assert torch.equal(_bits(targets[~hit]), torch.zeros_like(_bits(targets[~hit])))
    print(f"[partners B={B} T={T} F={F} {layout} Ks={Ks} Km={t.Km}] record end points {e_rec:.2e} m, contact targets {e_tg:.2e} m")
    assert e_rec <= RECORD_ERR_GATE and e_tg <= RECORD_ERR_GATE, (e_rec, e_tg)
    # the same bits run after run
    again = _run(c)
    for v, w in zip((tracks, bounds, targets), again):
        assert torch.equal(_bits(v), _bits(w.cpu()))


@pytest.mark.parametrize("B,T,F,layout,Ks", [s for s in PR.CASES if s[3] == "pairs" and s[4] == 0] + [(2, 196, 263, "pairs", 3)])
def test_world_joints_are_the_postprocessing_s(B, T, F, layout, Ks):
    MS, PP = pkg("motion_scene"), pkg("postprocess")
    c = PR.case(B, T, F, layout, Ks)
    J = c["J"]
    x = c["x0"].cuda()
    world = _run(c, return_world=True)[3]
    P = PP.recover_from_ric(x * c["std"].cuda()[:, None] + c["mean"].cuda()[:, None], J)  # fp32, (B, T, J, 3)
    worst = 0.0
    for b in range(B):
        n = int(c["lens"][b])
        want = MS.to_world(P[b, :n], c["pose"][b, :2].tolist(), float(c["pose"][b, 2]))
        worst = max(worst, float((world[b, :n] - want).abs().max()), float((world[b, :n].cpu().double() - c["W"][b]).abs().max()))
        assert not world[b, n:].any()
    print(f"[partners world B={B} T={T} F={F}] against to_world(recover_from_ric) in fp32 and against fp64: {worst:.2e} m")
    assert worst <= RECORD_ERR_GATE
    # at placement (0, 0, 0) the scratch is recover_from_ric bit for bit
    t0 = MS.partner_tables(c["scenes"], np.zeros((B, 3)), c["lens"], c["bones"], T=T, J=J)
    w0 = MS.partner_tracks(x, c["lens"], c["mean"], c["std"], t0, return_world=True)[3]
    for b in range(B):
        n = int(c["lens"][b])
        assert torch.equal(_bits(w0[b, :n]), _bits(P[b, :n])), b


def _contains(tracks, bounds, lens):
    """fp64: every live keep-out record of a frame, inflated by max(margin, 0), lies inside the frame's ball; +inf for a frame
    with a live half-space or keep-in record, -inf for one without a live record."""
    q, bd = tracks.double(), bounds.double()
    kind, live = q[..., 0], (q[..., 0] != 0) & (q[..., 2] > 0)
    open_ = (live & ((kind == 4) | (q[..., 1] < 0))).any(-1)
    none = ~live.any(-1)
    assert torch.equal(bd[..., 3][open_], torch.full_like(bd[..., 3][open_], math.inf))
    assert torch.equal(bd[..., 3][none], torch.full_like(bd[..., 3][none], -math.inf))
    finite = ~open_ & ~none
    assert bool(torch.isfinite(bd[..., 3][finite]).all()) and bool(torch.isfinite(bd[..., :3]).all())
    m = q[..., 3].clamp(min=0)
    c = bd[..., None, :3]
    far_sphere = (q[..., 4:7] - c).norm(dim=-1) + q[..., 7]
    far_caps = torch.maximum((q[..., 4:7] - c).norm(dim=-1), (q[..., 7:10] - c).norm(dim=-1)) + q[..., 10]
    far_box = (q[..., 4:7] - c).norm(dim=-1) + q[..., 7:10].norm(dim=-1)
    far = torch.where(kind == 1, far_sphere, torch.where(kind == 2, far_caps, far_box)) + m
    inside = far <= bd[..., 3:4]
    assert bool(inside[live & finite[..., None]].all())
    return int(open_.sum()), int(none.sum()), int(finite.sum())


@pytest.mark.parametrize("B,T,F,layout,Ks", PR.CASES)
def test_bounds_contain_the_records_and_change_no_bit_of_the_guidance(B, T, F, layout, Ks):
    L = pkg("_lib")
    c = PR.case(B, T, F, layout, Ks)
    t = c["tables"]
    tracks, bounds, targets = _run(c)
    n_open, n_none, n_finite = _contains(tracks.cpu(), bounds.cpu(), c["lens"])
    print(f"[partners bounds B={B} T={T} F={F} {layout} Ks={Ks}] frames with a +inf ball {n_open}, -inf {n_none}, finite {n_finite}")
    assert n_open > 0 if Ks else n_open == 0  # the half-space of the static tracks, live in all frames but the last
    assert n_finite > 0 and (n_none > 0 or Ks)
    # mdm_joint_tracks_guidance on the produced tracks: the produced balls against NULL bounds
    d = _diffusion("ddim10")
    N = d.num_timesteps
    coef = d._device_coef("dpmpp", 0.0, 2, "cuda")
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(B, T, F, generator=gen).cuda()
    x0 = c["x0"].cuda()
    mask = (torch.rand(B, T, F, generator=gen) < 0.5).float().cuda()
    jp = pkg("motion_scene").joint_params(c["J"])[None].expand(B, -1, -1).cuda().contiguous()
    lens, mean, std = c["lens"].cuda().to(torch.int32), c["mean"].cuda().contiguous(), c["std"].cuda().contiguous()
    w = t.weights.cuda()
    for m in (None, mask):
        outs = []
        for bd in (bounds, None):
            xo, x0o = x.clone(), x0.clone()
            L.check(L.lib().mdm_joint_tracks_guidance(
                _vp(xo), _vp(x0o), _vp(m), _vp(lens), _vp(mean), _vp(std), _vp(targets), _vp(w), _vp(None), C.c_int32(0), _vp(jp),
                _vp(tracks), C.c_int32(t.Km), _vp(bd), C.c_int32(B), C.c_int32(T), C.c_int32(F), C.c_float(1e-5), C.c_int32(3),
                _vp(coef), C.c_int32(N), C.c_void_p(0), C.c_int32(4), C.c_void_p(L.stream_ptr())))
            outs.append((xo, x0o))
        assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0])) and torch.equal(_bits(outs[0][1]), _bits(outs[1][1]))
        assert not torch.equal(outs[0][1], x0)


def test_weight_zero_partners_have_no_ball_and_one_character_has_no_tracks():
    MS = pkg("motion_scene")
    c = PR.case(4, 40, 263, "pairs", 0)
    t0 = MS.partner_tables(c["scenes"], c["pose"], c["lens"], c["bones"], T=40, J=22, weight=0.0)
    tracks, bounds, _ = MS.partner_tracks(c["x0"].cuda(), c["lens"], c["mean"], c["std"], t0)
    assert bool((tracks[..., 2] == 0).all()) and bool((tracks[0, :28, :, 0] == 2).all())
    assert bool((bounds[..., 3] == -math.inf).all()) and not bounds[..., :3].any()
    t1 = MS.partner_tables([[0], [1], [2, 3]], c["pose"], c["lens"], c["bones"], T=40, J=22)
    tracks, bounds, targets = MS.partner_tracks(c["x0"].cuda(), c["lens"], c["mean"], c["std"], t1)
    assert not tracks[:2].any() and bool((bounds[:2, :, 3] == -math.inf).all()) and bool(tracks[2, :17].any()) and not targets.any()
    t2 = MS.partner_tables([[0], [1]], c["pose"], c["lens"], c["bones"], T=40, J=22)
    tracks, bounds, targets = MS.partner_tracks(c["x0"].cuda(), c["lens"], c["mean"], c["std"], t2)
    assert tracks.shape == (4, 40, 0, 12) and bool((bounds[..., 3] == -math.inf).all())


def test_argument_errors():
    L, MS = pkg("_lib"), pkg("motion_scene")
    lib = L.lib()
    c = PR.case(4, 40, 263, "pairs", 3)
    t = c["tables"]
    B, T, F = 4, 40, 263
    dev = dict(x0=c["x0"].cuda().contiguous(), ln=c["lens"].cuda().to(torch.int32), mean=c["mean"].cuda().contiguous(),
               std=c["std"].cuda().contiguous(), place=t.placements.cuda(), prow=t.partner_rows.cuda(), cont=t.contacts.cuda(),
               world=torch.empty(B, T, 22, 3, device="cuda"),
               scratch=torch.empty(int(lib.mdm_partner_tracks_scratch_floats(B, T, F)), device="cuda"), tracks=torch.zeros(B, T, 24, 12, device="cuda"),
               bounds=torch.empty(B, T, 4, device="cuda"), targets=torch.zeros(B, T, 22, 3, device="cuda"))
    host = dict(prow=t.partner_rows.clone(), bones=t.bones.clone(), cont=t.contacts.clone())

    def call(over=None, **sizes):
        a = dict(dev)
        h = dict(host)
        for k, v in (over or {}).items():
            (h if k.startswith("h_") else a)[k[2:] if k.startswith("h_") else k] = v
        s = dict(Pm=1, nb=21, radius=0.3, margin=0.05, weight=5.0, Ks=3, Km=24, Nc=2, B=B, T=T, F=F)
        s.update(sizes)
        return lib.mdm_partner_tracks(_vp(a["x0"]), _vp(a["ln"]), _vp(a["mean"]), _vp(a["std"]), _vp(a["place"]), _vp(a["prow"]),
                                      _vp(h["prow"]), s["Pm"], _vp(h["bones"]), s["nb"], s["radius"], s["margin"], s["weight"],
                                      s["Ks"], s["Km"], _vp(a["cont"]), _vp(h["cont"]), s["Nc"], s["B"], s["T"], s["F"],
                                      _vp(a["world"]), _vp(a["scratch"]), _vp(a["tracks"]), _vp(a["bounds"]), _vp(a["targets"]),
                                      C.c_void_p(L.stream_ptr()))

    assert call() == 0
    for k in ("x0", "ln", "mean", "std", "place", "prow", "h_prow", "h_bones", "cont", "h_cont", "world", "scratch", "tracks", "bounds",
              "targets"):
        assert call({k: None}) == 1, k
    assert call(Km=25, Ks=4) == 1 and call(Km=-1) == 1 and call(Km=23) == 1 and call(Ks=2) == 1 and call(nb=20) == 1
    assert call(F=262) == 1 and call(F=10) == 1
    for i, v in ((0, 22), (1, -1)):
        bones = host["bones"].clone()
        bones[4, i] = v
        assert call({"h_bones": bones}) == 1
    for b, v in ((0, 4), (1, -2), (2, 2)):  # outside [-1, B), and a row that is its own partner
        prow = host["prow"].clone()
        prow[b, 0] = v
        assert call({"h_prow": prow}) == 1
    for col, v in ((0, 4), (2, -1), (1, 22), (3, -1), (4, 41), (6, int(np.float32(1.5).view(np.int32))),
                   (6, int(np.float32(-0.25).view(np.int32))), (6, int(np.float32(np.nan).view(np.int32))),
                   (6, int(np.float32(np.inf).view(np.int32)))):
        cont = host["cont"].clone()
        if col == 4:
            cont[1, 4], cont[1, 5] = 9, 8  # first > last
        else:
            cont[1, col] = v
        assert call({"h_cont": cont}) == 1, (col, v)
    assert call({"tracks": dev["tracks"].flatten()[1:]}) == 1 and call({"bounds": dev["bounds"].flatten()[1:]}) == 1
    assert call({"place": torch.zeros(17, device="cuda")[1:]}) == 1
    assert call(radius=0.0) == 1 and call(weight=-1.0) == 1 and call(margin=math.nan) == 1
    assert lib.mdm_partner_tracks_scratch_floats(4, 40, 263) == 4 * 40 * (67 + 66) + 134
    assert lib.mdm_partner_tracks_scratch_floats(4, 40, 262) == 0 and lib.mdm_partner_tracks_max_frames() == 3276
    assert call(B=0) == 0 and call(T=0) == 0 and call(B=-1) == 1
    # without partner slots, contacts or tracks their pointers may be NULL
    assert call({"prow": None, "h_prow": None, "h_bones": None, "cont": None, "h_cont": None, "targets": None, "tracks": None,
                 "bounds": None}, Pm=0, nb=0, Ks=0, Km=0, Nc=0) == 0
    torch.cuda.synchronize()
    # the Python layers
    with pytest.raises(L.MdmError):
        MS.partner_tracks(c["x0"], c["lens"], c["mean"], c["std"], t, c["static"])  # not on a GPU
    with pytest.raises(ValueError):
        MS.partner_tracks(c["x0"].cuda(), c["lens"], c["mean"], c["std"], t)  # the tables reserve three static tracks
    with pytest.raises(ValueError):
        MS.partner_tracks(c["x0"].cuda(), c["lens"], c["mean"], c["std"], t, c["static"][:, :, :2])
    with pytest.raises(ValueError):
        MS.partner_tracks(c["x0"].cuda()[:, :30], c["lens"], c["mean"], c["std"], t, c["static"])
    with pytest.raises(ValueError):
        MS.partner_tracks(c["x0"].cuda(), [40, 28, 40, 16], c["mean"], c["std"], t, c["static"])
    with pytest.raises(ValueError):
        MS.partner_tracks(c["x0"].cuda(), c["lens"], c["mean"], c["std"], PR.case(4, 40, 263, "pairs", 0)["tables"], c["static"])


# ---- loops ---------------------------------------------------------------------------------------------------------------
import functools  # noqa: E402

import sampler_ref as S  # noqa: E402
from conftest import rel_inf  # noqa: E402
from sampler_ref import caption_trainer as _trainer, loops_setup as _setup  # noqa: E402
from test_motion_scene_gpu import _check_against_restated, _control, _cuda  # noqa: E402
from test_scene_tracks_gpu import _crossing, _together_opts, _together_stats  # noqa: E402


def _loop_partners(B, T, lens):
    """The loops_tiny batch as one scene of all its rows, placed on top of each other, with a bone subset that fits the 24
    tracks of a frame and one wrist-to-wrist contact; on top of test_motion_scene_gpu._control's root path and static scene."""
    MS = pkg("motion_scene")
    ctl = _control(B, T)
    nb = min(24 // (B - 1), 21)
    bones = MS.skeleton_bones(22)[:nb]
    pose = torch.tensor([[0.15 * b, -0.1 * b, 0.4 * b] for b in range(B)], dtype=torch.float64)
    contacts = [MS.contact(0, 20, 1, 21, range(2, T - 2), weight=1.0, meet=0.5)]
    extra = dict(control_partner_scenes=[list(range(B))], control_partner_placements=pose, control_partner_bones=bones,
                 control_partner_radius=0.3, control_partner_margin=0.05, control_partner_weight=2.0, control_contact_list=contacts)
    tables = MS.partner_tables([list(range(B))], pose, lens, bones, T=T, J=22, contacts=contacts, radius=0.3, margin=0.05, weight=2.0,
                               control_weights=ctl["control_weights"])
    return ctl, extra, tables, contacts


@pytest.mark.parametrize("mode,eta,edit", [("cfg_dpmpp", 0.0, False), ("ddim", 0.5, False), ("cfg_dpmpp", 0.0, True)])
def test_partner_loops_match_the_restated_loop(mode, eta, edit):
    g, meta, m, noises, kw = _setup()
    d = _diffusion("ddim10")
    N, sc = d.num_timesteps, meta["cfg_scale"]
    B, T, F_ = g["x_T"].shape
    ctl, extra, tables, contacts = _loop_partners(B, T, g["length"])
    ns = noises(f"partners.{mode}.{eta}", N)
    known = mask = None
    skw = dict(kw, **_cuda(ctl), **extra)
    if edit:
        known = pkg("synth").uniform_pm1((B, T, F_), "partners.known", meta["iseed"])
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
            hook = PR.guidance_hook(g["length"], ctl, tables, contacts, mask, seen)
            want = S.loop_ref(d, mode, sc, S.device_eps(m, g["length"]), prompts=[(g["xf_proj"], g["xf_out"])],
                              uncond=m.uncond_embedding(B, "cuda"), inputs=[g["x_T"]] + got[:-1], eta=eta, step_noise=ns, clip=True,
                              known=known, mask=mask, x0_hook=hook)
            # on the restated states alone: the partner records bite, away from where their gradient jumps
            share, jump = max(s for s, _ in seen), min(j for _, j in seen)
            print(f"[partners loop {mode} eta {eta} edit {edit}] largest share of a row's (t, j) penalised by partner records in a "
                  f"step {share:.3f}, least distance of a penalised joint to a capsule axis {jump:.2e} m")
            assert share >= 0.05 and jump >= 1e-3, (share, jump)
            _check_against_restated(got, want, f"partners {mode} eta {eta} edit {edit}")
    assert torch.equal(outs[0], outs[1])  # graph == eager
    if edit:
        assert torch.equal(outs[0][mask == 1], known[mask == 1])
    plain = S.run_loop(d, mode, m, dict(kw, **_cuda(ctl)), sc, eta, True, x_T=g["x_T"].cuda(), step_noise=ns, clip=True).cpu()
    assert not torch.equal(plain, outs[0])


def test_runner_refusals():
    D = pkg("dist")
    g, meta, m, noises, kw = _setup()
    d = _diffusion("ddim10")
    B, T, F_ = g["x_T"].shape
    ctl, extra, tables, contacts = _loop_partners(B, T, g["length"])
    skw = dict(kw, **_cuda(ctl), **extra)

    def run(**over):
        return S.run_loop(d, "cfg_dpmpp", m, dict(skw, **over), meta["cfg_scale"], 0.0, False, x_T=g["x_T"].cuda(), clip=True)

    with pytest.raises(ValueError, match="bones="):  # Km over the limit: four static tracks in front of 21 bones
        run(control_tracks=torch.zeros(B, T, 4, 12).cuda())
    with pytest.raises(ValueError):  # handshake tables: long motions are out of scope
        run(handshake_offsets=torch.tensor([0, 2], dtype=torch.int32), handshake_rows=torch.tensor([3, T + 1], dtype=torch.int32),
            handshake_weights=torch.tensor([0.5, 0.5]), handshake_owner_rows=torch.tensor([3, 3], dtype=torch.int32))
    with pytest.raises(ValueError):  # canvas control
        run(canvas_control_offsets=torch.tensor([0, T], dtype=torch.int32))
    with pytest.raises(ValueError):
        run(control_partner_placements=None)
    with pytest.raises(ValueError):
        run(control_partner_scenes=[[0, B]])
    with pytest.raises(ValueError):  # two contacts on one (row, frame, joint)
        run(control_contact_list=contacts * 2)
    w = ctl["control_weights"].clone()
    w[0, 5, 20] = 1.0
    with pytest.raises(ValueError):  # a contact on a static control weight
        run(control_weights=w.cuda())
    with pytest.raises(ValueError):
        D.shard_kwargs(skw, 0, 1)
    with pytest.raises(ValueError):
        D.shard_kwargs({"control_contact_list": contacts}, 0, 1)
    assert "length" in D.shard_kwargs(kw, 0, 1)


# ---- through the trainer -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tr():
    g, meta, m, noises, kw = _setup()
    return _trainer(m, meta)


def _same(a, b):
    return torch.equal(_bits(a.cpu()), _bits(b.cpu()))


def test_mutual_bitwise_equivalences():
    MS = pkg("motion_scene")
    tr = _tr()
    mean, std = _together_stats()
    T = 16
    two = _crossing(T)
    opts = _together_opts()
    # one-character scenes: mutual is the sequential call
    solo = [[dict(two[0][0], position=(0.5, -0.25), yaw=0.3)], [dict(two[0][1], length=12, control_joints=two[0][1]["control_joints"][:12],
                                                                   control_weights=two[0][1]["control_weights"][:12])]]
    seq = tr.generate_together(solo, 263, mean, std, **opts)
    mut = tr.generate_together(solo, 263, mean, std, mutual=True, **opts)
    assert all(_same(a[0], b[0]) for a, b in zip(seq, mut)) and tuple(mut[1][0].shape) == (12, 22, 3)
    # weight = 0 without contacts: generate_joints of the flattened rows, then to_world
    free = tr.generate_together(two, 263, mean, std, radius=0.3, weight=0.0, mutual=True, **opts)
    place = [((0.0, 0.0), 0.0), ((1.0, -1.0), 0.0)]
    tg = torch.stack([MS.to_local(c["control_joints"], *pl) for c, pl in zip(two[0], place)])
    wt = torch.stack([c["control_weights"] for c in two[0]])
    ref = tr.generate_joints(["walk east", "walk north"], torch.tensor([T, T]), 263, mean, std, control_joints=tg, control_weights=wt,
                             **opts)
    assert all(_same(free[0][i], MS.to_world(ref[i], *place[i])) for i in range(2))
    # a contact in which b does all the reaching leaves a as it is without the contact
    reach = tr.generate_together(two, 263, mean, std, radius=0.3, weight=0.0, mutual=True,
                                 contacts=[[MS.contact(0, 21, 1, 20, range(6, 11), weight=5.0, meet=0.0)]], **opts)
    assert _same(reach[0][0], free[0][0]) and not _same(reach[0][1], free[0][1])
    # two scenes in one call: the first as it is alone, to the batch split's rounding
    both = tr.generate_together(two + [[dict(caption="walk east", length=12)]], 263, mean, std, radius=0.3, mutual=True, **opts)
    alone = tr.generate_together(two, 263, mean, std, radius=0.3, mutual=True, **opts)
    e = max(rel_inf(both[0][i].cpu(), alone[0][i].cpu()) for i in range(2))
    print(f"[partners trainer] a scene with another scene in its batch against the scene alone: {e:.2e}")
    assert e <= 1e-4 and len(both[1]) == 1 and tuple(both[1][0].shape) == (12, 22, 3)
    # the order of the characters does not matter beyond the noise they draw: the same call twice gives the same bits
    again = tr.generate_together(two, 263, mean, std, radius=0.3, mutual=True, **opts)
    assert all(_same(alone[0][i], again[0][i]) for i in range(2))


def test_mutual_errors():
    MS = pkg("motion_scene")
    tr = _tr()
    mean, std = _together_stats()
    two = _crossing(16)
    opts = _together_opts()
    c = MS.contact(0, 21, 1, 20, range(6, 11))
    with pytest.raises(ValueError, match="mutual"):
        tr.generate_together(two, 263, mean, std, contacts=[[c]], **opts)
    with pytest.raises(ValueError, match="bones="):  # two partners of 21 bones
        tr.generate_together([two[0] + two[0][:1]], 263, mean, std, mutual=True, **opts)
    with pytest.raises(ValueError, match="bones="):  # five characters, batches of four
        tr.generate_together([two[0] * 2 + two[0][:1]], 263, mean, std, mutual=True, bones=[(0, 1)], **opts)
    with pytest.raises(ValueError):
        tr.generate_together(two, 263, mean, std, mutual=True, contacts=[[c], []], **opts)
    with pytest.raises(ValueError):
        tr.generate_together(two, 263, mean, std, mutual=True, contacts=[[MS.contact(0, 21, 2, 20, range(6, 11))]], **opts)
    with pytest.raises(ValueError):  # on the root path's own weights
        tr.generate_together(two, 263, mean, std, mutual=True, contacts=[[MS.contact(0, 0, 1, 20, range(6, 11))]], **opts)


# the deepest penetration of either final body into the other's capsules with avoidance over that with weight = 0, measured
# on an MI355X, and its gate: 4 x the measurement, never above 0.5
MUTUAL_RATIO_MEASURED = 0.0  # no joint of either body is left inside the other's capsules
MUTUAL_RATIO_GATE = 0.5 if MUTUAL_RATIO_MEASURED is None else min(4 * MUTUAL_RATIO_MEASURED, 0.5)


def test_both_characters_move_out_of_each_other_s_way():
    """§25's crossing (straight pelvis paths that cross at (1, 0) in the middle of a 16-frame clip, capsules of radius 0.3,
    margin 0.05, weight 5) with mutual=True: the deeper of the two bodies' penetrations of the other, against weight = 0; and
    character 0 reacts, which in the sequential mode it never does."""
    MS = pkg("motion_scene")
    tr = _tr()
    mean, std = _together_stats()
    T = 16
    res = {wt: tr.generate_together(_crossing(T), 263, mean, std, radius=0.3, margin=0.05, weight=wt, mutual=True, **_together_opts())
           for wt in (5.0, 0.0)}
    depth = {}
    for wt, r in res.items():
        a, b = r[0]
        depth[wt] = max(float(MS.penetration(b[None], [T], None, tracks=MS.character_tracks(a, 0.3, margin=0.05))[0][0]),
                        float(MS.penetration(a[None], [T], None, tracks=MS.character_tracks(b, 0.3, margin=0.05))[0][0]))
    ratio = depth[5.0] / depth[0.0] if depth[0.0] > 0 else float("inf")
    moved = float((res[5.0][0][0] - res[0.0][0][0]).abs().max())
    print(f"[partners together] deepest penetration of either body into the other: weight 0 {depth[0.0]:.4f} m, weight 5 "
          f"{depth[5.0]:.4f} m, ratio {ratio:.3e}; character 0 moved by up to {moved:.4f} m")
    assert depth[0.0] > 0
    assert not _same(res[5.0][0][0], res[0.0][0][0])
    assert ratio <= MUTUAL_RATIO_GATE, ratio


# the mean wrist distance over the contact frames with the contact over that without, measured the same way
CONTACT_RATIO_MEASURED = 0.0616
CONTACT_RATIO_GATE = 0.5 if CONTACT_RATIO_MEASURED is None else min(4 * CONTACT_RATIO_MEASURED, 0.5)


def _standing(T):
    return [[dict(caption="stand", length=T), dict(caption="stand still", length=T, position=(0.8, 0.0), yaw=0.0)]]


def test_a_contact_brings_two_wrists_together():
    """Two characters standing 0.8 m apart, a wrist-to-wrist contact on frames 6 - 10 that meets halfway.  Its weight follows
    §14's rule, scale x curvature < 2, with §25's curvature 2 a J_c n_c t std^2: one joint, n_c = 5 contact frames, the force
    reaching the root velocities (std 0.002) of the t = 10 frames before them: 4e-4 a, so at scale 0.002 / 0.002^2 = 500
    a < 10; a = 2 keeps the factor 5 of the other behaviour tests."""
    import limb_pin_ref as LP
    import test_motion_features_gpu as TF
    MS, P = pkg("motion_scene"), pkg("postprocess")
    tr = _tr()
    mean, std = _together_stats()
    T, fr = 16, list(range(6, 11))
    c = MS.contact(0, 20, 1, 21, range(6, 11), weight=2.0, meet=0.5)
    opts = dict(_together_opts(), weight=0.0, mutual=True)
    res = {"with": tr.generate_together(_standing(T), 263, mean, std, contacts=[[c]], **opts),
           "without": tr.generate_together(_standing(T), 263, mean, std, **opts)}
    dist = {k: float((r[0][0][fr, 20] - r[0][1][fr, 21]).norm(dim=-1).mean()) for k, r in res.items()}
    ratio = dist["with"] / dist["without"]
    print(f"[partners contact] mean wrist distance over the contact frames: without {dist['without']:.4f} m, with {dist['with']:.4f} m, "
          f"ratio {ratio:.3e}")
    assert dist["without"] > 0
    assert ratio <= CONTACT_RATIO_GATE, ratio
    # pin_targets: the meeting point of the final joints joins both characters' pins
    pinned = tr.generate_together(_standing(T), 263, mean, std, contacts=[[c]], pin_targets=True, pin_blend=3, **opts)
    plain = res["with"][0]
    place = [((0.0, 0.0), 0.0), ((0.8, 0.0), 0.0)]
    m = plain[0][fr, 20] + 0.5 * (plain[1][fr, 21] - plain[0][fr, 20])
    g, w = torch.zeros(2, T, 22, 3), torch.zeros(2, T, 22, 3)
    g[0, fr, 20], g[1, fr, 21] = MS.to_local(m, *place[0]).cpu(), MS.to_local(m, *place[1]).cpu()
    w[0, fr, 20] = w[1, fr, 21] = 2.0
    local = torch.stack([MS.to_local(p, *pl) for p, pl in zip(plain, place)])
    want, (err, counts) = P.pin_limbs(local, torch.tensor([T, T]), g, w, blend=3, return_error=True)
    # the unpinned result went through to_world and back, so the comparison with the trainer's own pass is to rounding
    for i in range(2):
        assert float((pinned[0][i] - MS.to_world(want[i], *place[i])).abs().max()) <= 1e-5
    # where both limbs reach (pin_limbs' report: no pin frame out of reach) the wrists coincide, within 4 x the fp32 form's own
    # error of the restated pin on the same inputs, per wrist
    sk = TF.ref_skel("t2m")
    limbs = LP.limbs_of(sk)
    j, G, W = local.cpu().numpy(), g.numpy(), w.numpy()
    w64 = LP.pin_limbs(limbs, j, [T, T], G, W, blend=3, ft=np.float64)
    w32 = LP.pin_limbs(limbs, j, [T, T], G, W, blend=3, ft=np.float32)
    yard = float(np.abs(w32[0].astype(np.float64) - w64[0]).max())
    gap = (pinned[0][0][fr, 20] - pinned[0][1][fr, 21]).norm(dim=-1)
    out_of_reach = int(counts[:, :, 1].sum())
    print(f"[partners contact] pinned: wrist gaps {gap.tolist()}, pin frames out of reach {out_of_reach}, fp32 yardstick {yard:.2e}")
    assert int(counts[:, :, 0].sum()) == 2 * len(fr)
    if out_of_reach == 0:
        assert float(gap.max()) <= 2 * 4.0 * max(yard, 1e-7), (float(gap.max()), yard)
    else:
        reach = (torch.stack([(MS.to_world(want[i], *place[i])[fr, jn] - m.to(want)).norm(dim=-1) for i, jn in ((0, 20), (1, 21))])
                 <= 4.0 * max(yard, 1e-7)).all(0)
        assert bool(reach.any()) and float(gap[reach].max()) <= 2 * 4.0 * max(yard, 1e-7)

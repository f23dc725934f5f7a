"""CPU: scene constraints host logic.

* the primitive constructors and pack_scene: records, signs, the normalised normal, padding of per-sample lists;
* every ValueError of the helpers, of check_control_kwargs / check_canvas_control_kwargs and of the trainer's scene arguments;
  dist.shard_kwargs of the scene kwargs;
* the fp64 restatement tests/scene_ref.py (the reference tests/test_motion_scene_gpu.py holds the kernels against) checked
  against central finite differences, one case per kind plus keep-in, and against motion_scene's own torch distances;
* penetration against hand-placed joints;
* mdm_joint_scene_max_frames and the scene calls' argument checks without a GPU, where the library loads.
"""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

from conftest import pkg

import scene_ref as R
from test_motion_control_host import ref_positions


def _prims(MS):
    return [MS.sphere((0.3, 0.8, 0.2), 0.7, margin=0.05), MS.capsule((1, -1, 0), (1, 2, 0), 0.3, weight=2.0),
            MS.box((0, 0.5, 1), (0.5, 0.4, 0.6), 0.7, margin=0.1), MS.half_space((0, 2, 0), 0.1),
            MS.box((0, 1, 0), (2, 2, 2), -0.3, inside=True)]


# ---- constructors -------------------------------------------------------------------------------------------------------
def test_constructors_and_pack_scene():
    MS = pkg("motion_scene")
    rec = MS.pack_scene(_prims(MS))
    assert rec.shape == (5, 12) and rec.dtype == torch.float32
    assert rec[:, 0].tolist() == [1, 2, 3, 4, 3] and rec[:, 1].tolist() == [1, 1, 1, 1, -1]
    assert rec[0, 2:].tolist() == pytest.approx([1.0, 0.05, 0.3, 0.8, 0.2, 0.7, 0, 0, 0, 0])
    assert rec[1, 2:].tolist() == pytest.approx([2.0, 0.0, 1, -1, 0, 1, 2, 0, 0.3, 0])
    assert rec[2, 3:].tolist() == pytest.approx([0.1, 0, 0.5, 1, 0.5, 0.4, 0.6, math.cos(0.7), math.sin(0.7)])
    assert rec[3, 4:8].tolist() == pytest.approx([0, 1, 0, 0.1])  # the normal normalised on the host
    fl = MS.pack_scene([MS.floor(), MS.floor(0.25, margin=0.1)])
    assert fl[0].tolist() == [4, 1, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0] and fl[1, 3] == pytest.approx(0.1) and fl[1, 7] == 0.25
    assert MS.pack_scene([]).shape == (0, 12)
    assert MS.pack_scene([MS.floor()] * 16).shape == (16, 12)
    b = MS.batch_scene(_prims(MS), 3)
    assert b.shape == (3, 5, 12) and torch.equal(b[2], rec)
    per = MS.batch_scene([_prims(MS), [MS.floor()], []], 3)
    assert per.shape == (3, 5, 12) and torch.equal(per[0], rec) and per[1, 1:, 0].tolist() == [0] * 4 and not per[2].any()
    assert torch.equal(MS.batch_scene(rec, 2), rec[None].expand(2, -1, -1))
    jp = MS.joint_params(22)
    assert jp.shape == (22, 2) and jp[:, 0].tolist() == [0.0] * 22 and jp[:, 1].tolist() == [1.0] * 22
    jp = MS.joint_params(21, 0.05, [2.0] * 20 + [0.0])
    assert jp[:, 0].tolist() == pytest.approx([0.05] * 21) and jp[20, 1] == 0.0


def test_constructor_and_pack_errors():
    MS = pkg("motion_scene")
    nan, inf = float("nan"), float("inf")
    bad = [lambda: MS.sphere((0, 0, 0), 0.0), lambda: MS.sphere((0, 0, 0), -1.0), lambda: MS.sphere((0, nan, 0), 1.0),
           lambda: MS.sphere((0, 0), 1.0), lambda: MS.sphere((0, 0, 0), inf), lambda: MS.sphere((0, 0, 0), 1.0, weight=-1.0),
           lambda: MS.sphere((0, 0, 0), 1.0, margin=nan), lambda: MS.sphere((0, 0, 0), 1.0, weight=nan),
           lambda: MS.capsule((0, 0, 0), (0, 1, 0), 0.0), lambda: MS.capsule((0, 0, 0), (0, inf, 0), 1.0),
           lambda: MS.box((0, 0, 0), (1, 0, 1)), lambda: MS.box((0, 0, 0), (1, -1, 1)), lambda: MS.box((0, 0, 0), (1, 1, 1), nan),
           lambda: MS.box((0, 0, 0), (1, 1)), lambda: MS.half_space((0, 0, 0), 0.0), lambda: MS.half_space((0, 1, 0), nan),
           lambda: MS.half_space((0, nan, 0), 0.0), lambda: MS.floor(inf),
           lambda: MS.pack_scene([MS.floor()] * 17), lambda: MS.pack_scene([[4.0] * 12]),
           lambda: MS.batch_scene([[MS.floor()], [MS.floor()]], 3), lambda: MS.batch_scene(torch.zeros(2, 1, 12), 3),
           lambda: MS.joint_params(22, [0.1] * 21), lambda: MS.joint_params(22, [-0.1] * 22),
           lambda: MS.joint_params(22, None, [-1.0] * 22), lambda: MS.joint_params(22, None, [1.0] * 23),
           lambda: MS.joint_params(22, [nan] * 22), lambda: MS.max_frames(263, 17), lambda: MS.max_frames(262, 4)]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f"case {i} raised nothing")
    rec = MS.pack_scene(_prims(MS))
    for col, v in ((0, 5.0), (0, 1.5), (1, 0.5), (2, -1.0), (7, 0.0), (5, nan)):  # kind, sign, weight, a sphere's radius
        r = rec.clone()
        r[0, col] = v
        with pytest.raises(ValueError):
            MS.check_records(r)
    for row, col in ((1, 10), (2, 8)):  # a capsule's radius, a box's half extent
        r = rec.clone()
        r[row, col] = 0.0
        with pytest.raises(ValueError):
            MS.check_records(r)
    r = rec.clone()
    r[3, 4:7] = 0.0
    with pytest.raises(ValueError):
        MS.check_records(r)
    with pytest.raises(ValueError):
        MS.check_records(torch.zeros(17, 12))
    with pytest.raises(ValueError):
        MS.check_records(torch.zeros(3, 11))
    r = rec.clone()
    r[0] = float("nan")
    r[0, 0] = 0.0
    with pytest.raises(ValueError):  # padding has to be finite as well
        MS.check_records(r)


def test_frame_limit():
    MS, M = pkg("motion_scene"), pkg("motion_control")
    assert MS.max_frames(263, 16) == 202 and MS.max_frames(251, 16) == 208
    assert MS.max_frames(263, 16) >= 196 and MS.max_frames(251, 16) >= 196
    assert MS.max_frames(263, 0) == 205 and MS.max_frames(263, 0) <= M.max_frames(263)
    lib = pkg("_lib").lib()  # no GPU needed: a host function
    for F in (263, 251):
        assert lib.mdm_joint_scene_max_frames(F, 16) >= 196
        for K in (0, 1, 5, 16):
            assert lib.mdm_joint_scene_max_frames(F, K) == MS.max_frames(F, K), (F, K)
    assert lib.mdm_joint_scene_max_frames(262, 4) == 0 and lib.mdm_joint_scene_max_frames(263, 17) == 0
    assert lib.mdm_joint_scene_max_frames(263, -1) == 0


def test_argument_validation_without_gpu():
    """Every refusal happens before the launch, so it shows without a device (as tests/test_abi.py's)."""
    lib = pkg("_lib").lib()
    buf = (C.c_float * 16)()
    p = C.addressof(buf)
    ok = dict(x0=p, length=p, mean=p, std=p, targets=p, weights=p, scene=p, K=4, jp=p, B=1, T=8, F=263, loss=p, grad=p)

    def lg(**ch):
        a = dict(ok, **ch)
        return lib.mdm_joint_scene_loss_grad(a["x0"], a["length"], a["mean"], a["std"], a["targets"], a["weights"], a["scene"],
                                             a["K"], a["jp"], a["B"], a["T"], a["F"], a["loss"], a["grad"], None)

    for ch in (dict(K=17), dict(K=-1), dict(scene=None), dict(jp=None), dict(targets=None), dict(weights=None), dict(x0=None),
               dict(T=203, K=16), dict(T=0), dict(F=262), dict(B=-1), dict(loss=None), dict(grad=None), dict(mean=None)):
        assert lg(**ch) == 1, ch
    assert lg(B=0) == 0 and lg(B=0, targets=None, weights=None) == 0 and lg(B=0, K=0, scene=None) == 0

    def cg(**ch):
        a = dict(dict(ok, M=0, iters=1, steps=10, scale=0.1), **ch)
        return lib.mdm_canvas_scene_guidance(p, p, None, p, p, p, p, a["targets"], a["weights"], a["scene"], a["K"], a["jp"], a["M"],
                                             a["F"], a["scale"], a["iters"], p, a["steps"], None, 0, p, None)

    assert cg() == 0 and cg(targets=None, weights=None) == 0
    for ch in (dict(K=17), dict(scene=None), dict(jp=None), dict(weights=None), dict(F=262), dict(M=-1), dict(iters=0),
               dict(iters=33), dict(scale=float("nan")), dict(steps=0)):
        assert cg(**ch) == 1, ch


# ---- the restatement ----------------------------------------------------------------------------------------------------
def _case(T=6, F=263, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(1, T, F, generator=g, dtype=torch.float64) * 0.5
    mean = torch.randn(F, generator=g, dtype=torch.float64) * 0.1
    std = torch.rand(F, generator=g, dtype=torch.float64) + 0.5
    return x, mean, std


@pytest.mark.parametrize("kind", ["sphere", "capsule", "box", "half_space", "keep_in", "all"])
def test_reference_gradient_matches_finite_differences(kind):
    """One primitive of each kind placed from the positions (so that it penalises joints, clear of its jump set), a keep-in
    box, and all of them with radii, joint weights and targets: autograd against central differences of the fp64 loss."""
    T, F, J = 6, 263, 22
    x, mean, std = _case(T, F, seed=3)
    P = ref_positions(x[0, :T - 1], mean, std).detach()
    jp = torch.zeros(J, 2, dtype=torch.float64)
    jp[:, 1] = 1.0
    tg = w = None
    if kind == "all":
        g = torch.Generator().manual_seed(5)
        jp[:, 0] = torch.rand(J, generator=g, dtype=torch.float64) * 0.1
        jp[:, 1] = torch.rand(J, generator=g, dtype=torch.float64) * 2
        jp[3, 1] = 0.0
        tg = torch.randn(1, T, J, 3, generator=g, dtype=torch.float64)
        w = torch.rand(1, T, J, 3, generator=g, dtype=torch.float64)
    full = R.place_scene(P, jp, 5)
    scene = full if kind == "all" else full[["sphere", "capsule", "box", "half_space", "keep_in"].index(kind)][None]
    jump, share = R.scene_stats(P, scene, jp)
    assert float(jump.min()) >= R.JUMP_CLEAR and float(share.min()) > 0.02, (jump, share)
    loss, grad = R.ref_scene_loss_grad(x, [T - 1], mean, std, scene[None], jp[None], tg, w)
    assert float(loss[0]) > 0 and float(grad.abs().max()) > 0
    D = 3 * J + 1
    assert torch.equal(grad[0, :, D:], torch.zeros(T, F - D, dtype=torch.float64))
    assert torch.equal(grad[0, T - 1], torch.zeros(F, dtype=torch.float64))  # past the length
    h = 1e-6
    rng = np.random.RandomState(1)
    picks = [(t, c) for t in range(T - 1) for c in (0, 1, 2, 3)] + [(int(rng.randint(T - 1)), int(rng.randint(4, D)))
                                                                     for _ in range(16)]
    for t, c in picks:
        xp, xm = x.clone(), x.clone()
        xp[0, t, c] += h
        xm[0, t, c] -= h
        lp, _ = R.ref_scene_loss_grad(xp, [T - 1], mean, std, scene[None], jp[None], tg, w)
        lm, _ = R.ref_scene_loss_grad(xm, [T - 1], mean, std, scene[None], jp[None], tg, w)
        fd = float((lp - lm) / (2 * h))
        assert abs(fd - float(grad[0, t, c])) <= 1e-6 * max(1.0, abs(fd)), (kind, t, c, fd, float(grad[0, t, c]))


def test_reference_distances_by_hand_and_against_the_package():
    MS = pkg("motion_scene")
    rec = MS.pack_scene(_prims(MS)).double()
    p = torch.tensor([[0.3, 0.8, 1.2], [1.0, 3.0, 0.0], [1.0, 0.5, 0.4], [0.0, 0.5, 1.0], [0.0, -0.2, 0.0], [3.0, 1.0, 0.0]],
                     dtype=torch.float64)
    assert float(R.distance(p[0], rec[0])) == pytest.approx(1.0 - 0.7, abs=1e-7)      # sphere: 1 from the centre
    assert float(R.distance(p[1], rec[1])) == pytest.approx(1.0 - 0.3, abs=1e-7)      # capsule: 1 above its upper end
    assert float(R.distance(p[2], rec[1])) == pytest.approx(0.4 - 0.3, abs=1e-7)      # ... 0.4 beside its axis
    assert float(R.distance(p[3], rec[2])) == pytest.approx(-0.4, abs=1e-7)           # box: its centre, nearest face at 0.4
    assert float(R.distance(p[4], rec[3])) == pytest.approx(-0.3, abs=1e-7)           # half-space: 0.3 below Y = 0.1
    c, s = math.cos(-0.3), math.sin(-0.3)                                             # keep-in box: 3 along X, in its frame
    loc = (c * 3.0, 0.0, s * 3.0)
    want = math.hypot(max(abs(loc[0]) - 2, 0), max(abs(loc[2]) - 2, 0))
    assert float(R.distance(p[5], rec[4])) == pytest.approx(want, abs=1e-6)
    g = torch.Generator().manual_seed(2)
    pts = torch.randn(500, 3, generator=g, dtype=torch.float64) * 1.5
    ours = MS.signed_distances(pts, MS.pack_scene(_prims(MS)))
    ref = torch.stack([R.distance(pts, q) for q in rec], -1)
    assert ours.dtype == torch.float64 and float((ours - ref).abs().max()) <= 1e-12


# ---- penetration --------------------------------------------------------------------------------------------------------
def test_penetration_on_hand_placed_joints():
    MS = pkg("motion_scene")
    J = 22
    joints = torch.zeros(2, 4, J, 3)
    joints[..., 1] = 1.0                      # every joint at height 1, at the XZ origin
    joints[0, 1, 5] = torch.tensor([0.0, -0.25, 0.0])   # sample 0: one joint 0.25 under the floor in frame 1
    joints[0, 2, 7] = torch.tensor([0.0, 0.05, 0.0])    # ... one inside the floor's margin of 0.1 in frame 2
    joints[0, 3, 9] = torch.tensor([0.0, -5.0, 0.0])    # ... frame 3 lies past the length
    joints[1, 0, 0] = torch.tensor([2.0, 1.0, 0.1])     # sample 1: the pelvis 0.1 from the centre of a sphere of radius 0.5
    scene = [MS.floor(0.0, margin=0.1), MS.sphere((2.0, 1.0, 0.0), 0.5), MS.sphere((0, 1, 0), 5.0, weight=0.0)]
    depth, share = MS.penetration(joints, [3, 4], scene)
    assert depth.tolist() == pytest.approx([0.25, 0.4]) and share.tolist() == pytest.approx([2 / 3, 1 / 4])
    depth, share = MS.penetration(joints, [3, 4], scene, joint_radius=[0.1] * J)
    assert depth.tolist() == pytest.approx([0.35, 0.5]) and share.tolist() == pytest.approx([2 / 3, 1 / 4])
    keep_in = [[MS.box((0, 1, 0), (1, 1, 1), inside=True)], [MS.box((0, 1, 0), (1, 5, 1), inside=True)]]
    depth, share = MS.penetration(joints, [4, 4], keep_in)   # sample 0's joint 9 is 5 below its box, sample 1's pelvis 1 beside
    assert depth.tolist() == pytest.approx([5.0, 1.0]) and share.tolist() == pytest.approx([2 / 4, 1 / 4])
    depth, share = MS.penetration(joints, [0, 4], [])
    assert depth.tolist() == [0.0, 0.0] and share.tolist() == [0.0, 0.0]
    with pytest.raises(ValueError):
        MS.penetration(joints[0], [3], scene)


# ---- model kwargs -------------------------------------------------------------------------------------------------------
def _kw(B=2, T=8, F=263, targets=True):
    MS = pkg("motion_scene")
    J = (F + 1) // 12
    kw = {"control_mean": torch.zeros(B, F), "control_std": torch.ones(B, F), "control_scale": 0.5, "control_iters": 3,
          "control_scene": MS.batch_scene(_prims(MS), B), "control_joint_params": MS.joint_params(J)[None].expand(B, -1, -1)}
    if targets:
        kw.update(control_joints=torch.zeros(B, T, J, 3), control_weights=torch.ones(B, T))
    return kw


def test_check_control_kwargs_accepts_a_scene():
    D = pkg("diffusion")
    c = D.check_control_kwargs(_kw(), (2, 8, 263))
    assert c["scene"].shape == (2, 5, 12) and c["joint_params"].shape == (2, 22, 2) and c["targets"].shape == (2, 8, 22, 3)
    c = D.check_control_kwargs(_kw(targets=False), (2, 8, 263))  # a scene without targets
    assert c["targets"] is None and c["weights"] is None and c["scene"].shape == (2, 5, 12) and c["iters"] == 3
    kw = _kw(targets=False)
    del kw["control_joint_params"], kw["control_scale"], kw["control_iters"]
    c = D.check_control_kwargs(kw, (2, 8, 263))
    assert c["joint_params"].shape == (2, 22, 2) and c["joint_params"][0, 0].tolist() == [0.0, 1.0] and c["scale"] == 1.0
    no_scene = {k: v for k, v in _kw().items() if k not in ("control_scene", "control_joint_params")}
    assert "scene" not in D.check_control_kwargs(no_scene, (2, 8, 263))
    assert D.check_control_kwargs(_kw(T=202), (2, 202, 263)) is not None
    assert D.check_control_kwargs(dict(_kw(T=196, F=251)), (2, 196, 251))["scene"].shape == (2, 5, 12)


def _bad_scene(col, v, row=0):
    MS = pkg("motion_scene")
    r = MS.batch_scene(_prims(MS), 2).clone()
    r[1, row, col] = v
    return r


@pytest.mark.parametrize("change", [
    dict(control_mean=None), dict(control_std=None), dict(control_scene=None), dict(control_weights=None),
    dict(control_joints=None), dict(control_scene=torch.zeros(2, 17, 12)), dict(control_scene=torch.zeros(2, 5, 11)),
    dict(control_scene=torch.zeros(3, 5, 12)), dict(control_scene=torch.zeros(5, 12)),
    dict(control_scene=torch.zeros(2, 5, 12, dtype=torch.int64)),
    dict(control_scene=_bad_scene(5, float("nan"))), dict(control_scene=_bad_scene(0, 7.0)), dict(control_scene=_bad_scene(1, 0.0)),
    dict(control_scene=_bad_scene(2, -1.0)), dict(control_scene=_bad_scene(7, 0.0)), dict(control_scene=_bad_scene(8, -1.0, row=2)),
    dict(control_scene=_bad_scene(5, 0.0, row=3)),
    dict(control_joint_params=torch.zeros(2, 21, 2)), dict(control_joint_params=torch.zeros(22, 2)),
    dict(control_joint_params=-torch.ones(2, 22, 2)), dict(control_joint_params=torch.full((2, 22, 2), float("inf"))),
    dict(control_joint_params=torch.zeros(2, 22, 2, dtype=torch.int64)),
    dict(control_scale=float("nan")), dict(control_iters=0), dict(control_iters=33),
])
def test_check_control_kwargs_scene_errors(change):
    D = pkg("diffusion")
    kw = {k: v for k, v in dict(_kw(), **change).items() if v is not None}
    with pytest.raises(ValueError):
        D.check_control_kwargs(kw, (2, 8, 263))


def test_check_control_kwargs_scene_frame_limit_and_partners():
    D = pkg("diffusion")
    with pytest.raises(ValueError):  # T over the LDS limit with 5 primitives (204) though under the plain limit (205)
        D.check_control_kwargs(_kw(T=205), (2, 205, 263))
    MS = pkg("motion_scene")
    full = dict(_kw(T=203), control_scene=MS.batch_scene([MS.floor()] * 16, 2))
    with pytest.raises(ValueError):
        D.check_control_kwargs(full, (2, 203, 263))
    assert D.check_control_kwargs(dict(_kw(T=202), control_scene=full["control_scene"]), (2, 202, 263)) is not None
    with pytest.raises(ValueError):  # joint parameters without a scene
        D.check_control_kwargs({k: v for k, v in _kw().items() if k != "control_scene"}, (2, 8, 263))
    with pytest.raises(ValueError):  # a scene needs mean / std even without targets
        D.check_control_kwargs({"control_scene": _kw()["control_scene"]}, (2, 8, 263))
    with pytest.raises(NotImplementedError):  # a per-window scene over a long motion
        D.check_handshake_kwargs(dict(_kw(targets=False), handshake_offsets=torch.tensor([0, 2]), handshake_rows=torch.tensor([7, 8]),
                                      handshake_weights=torch.tensor([0.5, 0.5]), handshake_owner_rows=torch.tensor([7, 8])),
                                 (2, 8, 263))


def test_check_canvas_control_kwargs_with_a_scene():
    D, MS = pkg("diffusion"), pkg("motion_scene")
    B, T, F, J = 1, 8, 263, 22
    base = {"canvas_control_offsets": torch.tensor([0, 6]), "canvas_control_rows": torch.arange(6),
            "canvas_control_mean": torch.zeros(1, F), "canvas_control_std": torch.ones(1, F),
            "canvas_control_scene": MS.batch_scene(_prims(MS), 1)}
    c = D.check_canvas_control_kwargs(base, (B, T, F))
    assert c["targets"] is None and c["weights"] is None and c["scene"].shape == (1, 5, 12)
    assert c["joint_params"].shape == (1, J, 2) and c["total"] == 6
    both = dict(base, canvas_control_joints=torch.zeros(6, J, 3), canvas_control_weights=torch.ones(6),
                canvas_control_joint_params=MS.joint_params(J, 0.1)[None])
    c = D.check_canvas_control_kwargs(both, (B, T, F))
    assert c["targets"].shape == (6, J, 3) and c["weights"].shape == (6, J, 3) and float(c["joint_params"][0, 0, 0]) == pytest.approx(0.1)
    assert D.check_control_kwargs(dict(base, control_scale=0.1), (B, T, F)) is None  # the scale is the canvas control's
    for change in (dict(canvas_control_mean=None), dict(canvas_control_rows=None), dict(canvas_control_scene=torch.zeros(2, 5, 12)),
                   dict(canvas_control_scene=torch.zeros(1, 17, 12)), dict(canvas_control_joint_params=torch.zeros(1, 21, 2)),
                   dict(canvas_control_joint_params=-torch.ones(1, J, 2)), dict(canvas_control_weights=torch.ones(6)),
                   dict(canvas_control_scene=None, canvas_control_joint_params=torch.zeros(1, J, 2))):
        kw = {k: v for k, v in dict(base, **change).items() if v is not None}
        with pytest.raises(ValueError):
            D.check_canvas_control_kwargs(kw, (B, T, F))


def test_shard_kwargs_gives_each_rank_its_rows():
    Dist, MS = pkg("dist"), pkg("motion_scene")
    kw = _kw(B=5)
    kw["control_scene"] = MS.batch_scene([[MS.floor(0.1 * i)] * (1 + i % 2) for i in range(5)], 5)
    kw["control_joint_params"] = torch.arange(5 * 22 * 2, dtype=torch.float32).reshape(5, 22, 2)
    for lo, hi in ((0, 3), (3, 5)):
        s = Dist.shard_kwargs(kw, lo, hi)
        for k in ("control_scene", "control_joint_params", "control_joints", "control_mean"):
            assert torch.equal(s[k], kw[k][lo:hi]), k
        c = pkg("diffusion").check_control_kwargs(s, (hi - lo, 8, 263))
        assert c["scene"].shape == (hi - lo, 2, 12) and c["joint_params"].shape[0] == hi - lo


# ---- trainer arguments --------------------------------------------------------------------------------------------------
def test_trainer_scene_arguments():
    Cond, MS = pkg("conditioning").Conditioning, pkg("motion_scene")
    caps = ["a", "b", "c"]
    mean, std = np.zeros(263, np.float32), np.ones(263, np.float32)
    c = Cond(caps, 263, scene=_prims(MS), mean=mean, std=std, control_scale=0.3)
    kw = c.control_kwargs(slice(1, 3), 6, "cpu")
    assert "control_joints" not in kw and kw["control_scene"].shape == (2, 5, 12) and kw["control_joint_params"].shape == (2, 22, 2)
    assert kw["control_mean"].shape == (2, 263) and kw["control_scale"] == 0.3
    assert pkg("diffusion").check_control_kwargs(kw, (2, 6, 263))["targets"] is None
    per = [[MS.floor()], _prims(MS), []]
    c = Cond(caps, 263, scene=per, scene_joint_radius=[0.1] * 22, scene_joint_weights=[1.0] * 21 + [0.0], mean=mean, std=std,
             control_joints=torch.zeros(3, 10, 22, 3), control_weights=torch.ones(3))
    kw = c.kwargs(torch.tensor([2, 0]), 10, "cpu")
    assert kw["control_joints"].shape == (2, 10, 22, 3) and kw["control_scene"].shape == (2, 5, 12)
    assert not kw["control_scene"][0].any() and kw["control_scene"][1, 0, 0] == 4 and kw["control_joint_params"][1, 21].tolist() == [pytest.approx(0.1), 0.0]
    assert Cond(caps, 263, mean=mean, std=std).control_kwargs(slice(0, 3), 6, "cpu") == {}
    for bad in (dict(scene=_prims(MS)), dict(scene=_prims(MS), mean=mean), dict(scene=per[:2], mean=mean, std=std),
                dict(scene=[MS.floor()] * 17, mean=mean, std=std), dict(scene_joint_radius=[0.1] * 22, mean=mean, std=std),
                dict(scene=_prims(MS), scene_joint_radius=[0.1] * 21, mean=mean, std=std),
                dict(scene=_prims(MS), scene_joint_weights=[-1.0] * 22, mean=mean, std=std),
                dict(scene=[[1.0] * 12], mean=mean, std=std)):
        with pytest.raises(ValueError):
            Cond(caps, 263, **bad)
    Tr = pkg("trainer")
    tr = Tr.DDPMTrainer.__new__(Tr.DDPMTrainer)  # the checks run before anything touches a device
    tr.encoder, tr.device = types.SimpleNamespace(num_frames=16, eval=lambda: None), "cpu"
    lens = torch.tensor([16, 12, 8])
    for method in (tr.generate_batch, tr.generate, tr.generate_bucketed):
        with pytest.raises(ValueError, match="mean and std"):
            method(caps, lens, 263, scene=_prims(MS))
        with pytest.raises(ValueError, match="go with scene"):
            method(caps, lens, 263, scene_joint_radius=[0.1] * 22, mean=mean, std=std)
        with pytest.raises(ValueError, match="at most 16"):
            method(caps, lens, 263, scene=[MS.floor()] * 17, mean=mean, std=std)
    with pytest.raises(ValueError, match="one list of primitives per motion"):
        tr.generate_long([[("a", 16)]], 263, overlap=4, scene=_prims(MS), mean=mean, std=std)
    with pytest.raises(ValueError, match="mean and std"):
        tr.generate_long([[("a", 16)]], 263, overlap=4, scene=[_prims(MS)])
    with pytest.raises(ValueError, match="must have 22 entries"):  # through an output method's **kw
        tr.generate_joints(caps, lens, 263, mean, std, scene=_prims(MS), scene_joint_radius=[0.1] * 3)


def test_canvas_control_takes_a_scene_per_motion():
    ML, MS = pkg("motion_long"), pkg("motion_scene")
    plans = ML.script_plans([[("a", 16), ("b", 12)], [("c", 10)]], 4, 16)
    mean, std = np.zeros(263, np.float32), np.ones(263, np.float32)
    scenes = [_prims(MS), [MS.floor()]]
    tables = ML.canvas_control(plans, 263, mean=mean, std=std, scene=scenes, scene_joint_radius=[0.1] * 22, control_iters=2)
    kw = tables([1, 0], 16)
    assert "canvas_control_joints" not in kw and kw["canvas_control_scene"].shape == (2, 5, 12) and kw["control_iters"] == 2
    assert kw["canvas_control_scene"][0, 0, 0] == 4 and kw["canvas_control_joint_params"].shape == (2, 22, 2)
    assert kw["canvas_control_rows"].numel() == 24 + 10 and kw["canvas_control_mean"].shape == (2, 263)
    full = dict(kw, **ML.batch_tables(plans, [1, 0], 16, 4), length=torch.tensor([10, 16, 12]))
    c = pkg("diffusion").check_canvas_control_kwargs(full, (3, 16, 263))
    assert c["targets"] is None and c["scene"].shape == (2, 5, 12)
    assert ML.canvas_control(plans, 263)([0], 16) == {}
    for bad in (dict(scene=scenes), dict(scene=scenes, mean=mean), dict(scene=_prims(MS), mean=mean, std=std),
                dict(scene=scenes[:1], mean=mean, std=std), dict(scene_joint_radius=[0.1] * 22, mean=mean, std=std),
                dict(scene=[scenes[0], None], mean=mean, std=std), dict(scene=scenes, scene_joint_weights=[1.0] * 3, mean=mean, std=std)):
        with pytest.raises(ValueError):
            ML.canvas_control(plans, 263, **bad)

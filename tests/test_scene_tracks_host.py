"""CPU: tracks, the host side: the moving constructors, packing and padding, the broad phase's balls, characters
as obstacles and the world transform, the fp64 restatement of tests/scene_tracks_ref.py against central differences,
``penetration(tracks=)``, the model-kwargs checks, sharding, the trainer's arguments and the argument errors of the four new
entries on the loaded library."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

from conftest import pkg

import scene_ref as R
import scene_tracks_ref as TR
from test_motion_control_host import ref_positions

T = 6


def _line(a, b, n=T):
    return torch.stack([torch.linspace(a[k], b[k], n, dtype=torch.float64) for k in range(3)], 1)


def _tracks(MS, n=T):
    """One track of each kind and a keep-in box, over n frames."""
    t = torch.arange(n, dtype=torch.float64)
    return [MS.moving_sphere(_line((0, 1, 0), (1, 1, 0), n), 0.5, margin=0.1),
            MS.moving_capsule(_line((1, 0, 1), (1, 0, 2), n), _line((1, 2, 1), (1, 2, 2), n), 0.3, weight=2.0),
            MS.moving_box(_line((0, 0.5, 1), (1, 0.5, 1), n), (0.5, 0.4, 0.6), 0.1 * t),
            MS.moving_half_space((0, 2, 0), 0.1 * t),
            MS.moving_box(torch.zeros(n, 3), (2, 2, 2), -0.3, inside=True)]


# ---- constructors and packing -------------------------------------------------------------------------------------------
def test_constructors_and_packing():
    MS = pkg("motion_scene")
    assert MS.MAX_TRACKS == 24 == pkg("_lib").SCENE_MAX_TRACKS
    sp, cap, box, hs, keep = _tracks(MS)
    for tr in (sp, cap, box, hs, keep):
        assert tuple(tr.shape) == (T, 12) and tr.dtype == torch.float64
    assert sp[2].tolist() == [1, 1, 1, 0.1, pytest.approx(0.4), 1, 0, 0.5, 0, 0, 0, 0]
    assert cap[0, :4].tolist() == [2, 1, 2, 0] and cap[5, 4:11].tolist() == [1, 0, 2, 1, 2, 2, pytest.approx(0.3)]
    assert box[3, 10:].tolist() == [pytest.approx(math.cos(0.3)), pytest.approx(math.sin(0.3))] and box[3, 7:10].tolist() == [0.5, 0.4, 0.6]
    assert hs[4, 4:8].tolist() == [0, 1, 0, pytest.approx(0.4)]  # the normal is normalised, the offset is not touched
    assert keep[0, 1] == -1 and keep[:, 0].tolist() == [3] * T
    # a frame's record is the static constructor's
    assert MS.pack_tracks([sp], T)[2, 0].tolist() == MS.pack_scene([MS.sphere((0.4, 1, 0), 0.5, margin=0.1)])[0].tolist()
    # scalars and per-frame values broadcast; active= gives padding frames
    on = np.array([True, False, True, True, False, True])
    v = MS.moving_sphere(_line((0, 0, 0), (1, 0, 0)), torch.linspace(0.1, 0.6, T), weight=np.linspace(1, 2, T), active=on)
    assert v[3, 7] == pytest.approx(0.4) and v[3, 2] == pytest.approx(1.6) and not v[1].any() and not v[4].any() and v[5, 0] == 1
    still = MS.moving_sphere((0, 1, 0), 0.5, active=np.ones(4, bool))  # nothing moves: the frames come from active=
    assert tuple(still.shape) == (4, 12) and still[3, 4:8].tolist() == [0, 1, 0, 0.5]
    rec = MS.pack_tracks([sp, cap[:4], keep], T)
    assert tuple(rec.shape) == (T, 3, 12) and rec.dtype == torch.float32
    assert rec[3, 1, 0] == 2 and not rec[4:, 1].any()  # frames past a track's own length are padding
    assert tuple(MS.pack_tracks([sp], 4).shape) == (4, 1, 12) and tuple(MS.pack_tracks([], 4).shape) == (4, 0, 12)
    b = MS.batch_tracks([sp, cap], 3, 8)
    assert tuple(b.shape) == (3, 8, 2, 12) and torch.equal(b[0], b[2]) and not b[:, T:].any()
    b = MS.batch_tracks([[sp, cap, box], [hs], []], 3, T)
    assert tuple(b.shape) == (3, T, 3, 12) and b[1, 0, 0, 0] == 4 and not b[1, :, 1:].any() and not b[2].any()
    packed = MS.batch_tracks(b, 3, 4)  # packed records: their first T frames
    assert torch.equal(packed, b[:, :4]) and torch.equal(MS.batch_tracks(b[0], 2, T)[1], b[0])
    assert tuple(MS.batch_tracks(b, 3, 8, lengths=[6, 2, 0]).shape) == (3, 8, 3, 12)  # longer than every sample: padded
    c = MS.canvas_tracks([[sp], [cap, hs]], [0, 4, 4 + T])
    assert tuple(c.shape) == (4 + T, 2, 12) and c[3, 0, 0] == 1 and not c[:4, 1].any() and c[4, 1, 0] == 4


def test_constructor_and_packing_errors():
    MS = pkg("motion_scene")
    c = _line((0, 0, 0), (1, 0, 0))
    sp = MS.moving_sphere(c, 0.5)
    bad = [lambda: MS.pack_tracks([sp] * 25, T),                                 # more than 24 tracks
           lambda: MS.batch_tracks(torch.zeros(2, T, 25, 12), 2, T),
           lambda: MS.moving_sphere(c * float("nan"), 0.5),                      # non-finite values
           lambda: MS.moving_sphere(c, float("inf")),
           lambda: MS.moving_capsule(c, c + 1, 0.2, margin=float("nan")),
           lambda: MS.moving_sphere(c, 0.0),                                     # a radius or half extent <= 0
           lambda: MS.moving_sphere(c, torch.tensor([0.5, 0.5, -0.1, 0.5, 0.5, 0.5])),
           lambda: MS.moving_capsule(c, c + 1, -1.0),
           lambda: MS.moving_box(c, (0.5, 0.0, 0.5)),
           lambda: MS.moving_half_space(torch.zeros(T, 3), 0.0),                 # a zero normal
           lambda: MS.moving_half_space((0, 0, 0), torch.zeros(T)),
           lambda: MS.moving_sphere(c, 0.5, weight=-1.0),                        # a weight < 0
           lambda: MS.moving_sphere(c, torch.full((T + 1,), 0.5)),               # per-frame shapes that disagree
           lambda: MS.moving_capsule(c, c[:4], 0.2),
           lambda: MS.moving_sphere(c, 0.5, active=np.ones(T + 2, bool)),
           lambda: MS.moving_sphere(c[:, :2], 0.5),
           lambda: MS.moving_sphere((0, 1, 0), 0.5),                             # no frame count at all
           lambda: MS.moving_sphere(c, 0.5, active=np.ones(T)),                  # active must be bool
           lambda: MS.batch_tracks(torch.zeros(2, 4, 3, 12), 2, T),              # tracks shorter than a sample's length
           lambda: MS.batch_tracks(torch.zeros(2, 4, 3, 12), 2, 8, lengths=[3, 5]),
           lambda: MS.batch_tracks([[sp], [sp]], 3, T),                          # one list per sample, or one for all
           lambda: MS.pack_tracks([torch.zeros(T, 11)], T),
           lambda: MS.canvas_tracks(torch.zeros(9, 2, 12), [0, 4, 10]),
           lambda: MS.canvas_tracks([[sp]], [0, 4, 10]),
           lambda: MS.check_tracks(torch.zeros(3, 12))]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f"case {i} raised nothing")
    r = MS.batch_tracks([sp], 1, T).clone()
    for col, v in ((0, 7.0), (1, 0.0), (2, -1.0), (7, 0.0), (5, float("nan"))):
        q = r.clone()
        q[0, 2, 0, col] = v
        with pytest.raises(ValueError):
            MS.check_tracks(q)
    assert MS.batch_tracks(torch.zeros(2, 4, 3, 12), 2, 8, lengths=[3, 4]).shape == (2, 8, 3, 12)


# ---- the broad phase ----------------------------------------------------------------------------------------------------
def _surface(q, n, g):
    """n points on the surface of the keep-out primitive of record q (fp64), pushed outwards by its margin."""
    kind, m = int(q[0]), max(float(q[3]), 0.0)
    u = torch.randn(n, 3, generator=g, dtype=torch.float64)
    u = u / u.norm(dim=1, keepdim=True)
    if kind == R.SPHERE:
        return q[4:7] + (float(q[7]) + m) * u
    if kind == R.CAPSULE:
        s = torch.rand(n, 1, generator=g, dtype=torch.float64)
        return q[4:7] + s * (q[7:10] - q[4:7]) + (float(q[10]) + m) * u
    loc = (torch.rand(n, 3, generator=g, dtype=torch.float64) * 2 - 1) * q[7:10]  # a box: points of the box, corners included
    loc[:8] = torch.tensor([[a, b, c] for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)], dtype=torch.float64) * q[7:10]
    c, s = q[10], q[11]
    return q[4:7] + torch.stack([c * loc[:, 0] + s * loc[:, 2], loc[:, 1], c * loc[:, 2] - s * loc[:, 0]], 1) + m * u


def test_track_bounds_contain_every_inflated_keep_out_record():
    MS = pkg("motion_scene")
    g = torch.Generator().manual_seed(4)
    sp, cap, box, hs, keep = _tracks(MS)
    far = MS.moving_sphere(_line((40, 3, -20), (45, 3, -20)), 2.0, margin=0.5)
    rec = MS.pack_tracks([sp, cap, box, far], T)
    bnd = MS.track_bounds(rec)
    assert tuple(bnd.shape) == (T, 4) and bnd.dtype == torch.float32 and bool(torch.isfinite(bnd).all())
    for t in range(T):
        c, rad = bnd[t, :3].double(), float(bnd[t, 3])
        for k in range(4):
            q = rec[t, k].double()
            pts = _surface(q, 400, g)
            # on or inside the inflated surface (the fp32 cosine and sine of a box's yaw are a rotation to 1e-7 only)
            assert float(R.distance(pts, q).max()) <= max(float(q[3]), 0) + 1e-6
            assert float((pts - c).norm(dim=1).max()) <= rad, (t, k)
    # a tight case by hand: one sphere of radius 0.5 with margin 0.1 -> 0.6 inflated by 1e-3 relative + 1e-3 m
    one = MS.track_bounds(MS.pack_tracks([sp], T))
    assert one[2].tolist() == pytest.approx([0.4, 1.0, 0.0, 0.6 * 1.001 + 0.001], abs=1e-6)
    # +inf for a frame with a half-space or a keep-in track, weight 0 and padding do not count, -inf for an empty frame
    assert MS.track_bounds(MS.pack_tracks([sp, hs], T))[:, 3].tolist() == [float("inf")] * T
    assert MS.track_bounds(MS.pack_tracks([sp, keep], T))[:, 3].tolist() == [float("inf")] * T
    quiet = MS.moving_half_space((0, 1, 0), 0.0, weight=0.0, active=np.ones(T, bool))
    assert torch.equal(MS.track_bounds(MS.pack_tracks([sp, quiet], T)), one)
    on = np.array([True, True, False, True, True, True])
    gap = MS.track_bounds(MS.pack_tracks([MS.moving_sphere(_line((0, 1, 0), (1, 1, 0)), 0.5, margin=0.1, active=on)], T))
    assert gap[2].tolist() == [0, 0, 0, float("-inf")] and torch.equal(gap[3], one[3])
    assert MS.track_bounds(torch.zeros(2, 3, 0, 12))[..., 3].tolist() == [[float("-inf")] * 3] * 2
    assert tuple(MS.track_bounds(MS.batch_tracks([sp, cap], 3, T)).shape) == (3, T, 4)
    # a negative margin shrinks nothing: the ball still holds the primitive itself
    neg = MS.track_bounds(MS.pack_tracks([MS.moving_sphere(_line((0, 1, 0), (1, 1, 0)), 0.5, margin=-0.2)], T))
    assert float(neg[0, 3]) >= 0.5


# ---- characters as obstacles --------------------------------------------------------------------------------------------
def test_character_tracks_and_the_world_transform():
    MS, MF = pkg("motion_scene"), pkg("motion_features")
    g = torch.Generator().manual_seed(1)
    joints = torch.randn(T, 22, 3, generator=g, dtype=torch.float64)
    tr = MS.character_tracks(joints, 0.07, margin=0.02, weight=3.0)
    parents = MF.SKELETONS["t2m"].parents
    assert len(tr) == 21 and all(tuple(t.shape) == (T, 12) for t in tr)
    for t, child in zip(tr, range(1, 22)):  # bone ends are the joints, in the order of the skeleton's tree
        assert torch.equal(t[:, 4:7], joints[:, parents[child]]) and torch.equal(t[:, 7:10], joints[:, child])
        assert t[0, :4].tolist() == [2, 1, 3.0, 0.02] and t[0, 10] == 0.07
    assert len(MS.character_tracks(torch.randn(T, 21, 3))) == 20  # the 21-joint skeleton
    arm = MS.character_tracks(joints, bones=[(16, 18), (18, 20)])
    assert len(arm) == 2 and torch.equal(arm[1][:, 7:10], joints[:, 20])
    for bad in (lambda: MS.character_tracks(joints[0]), lambda: MS.character_tracks(torch.zeros(T, 7, 3)),
                lambda: MS.character_tracks(joints, bones=[(0, 22)]), lambda: MS.character_tracks(joints, 0.0)):
        with pytest.raises(ValueError):
            bad()
    # p_world = R_y(yaw) p + (x, 0, z)
    w = MS.to_world(torch.tensor([[1.0, 2.0, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64), (3.0, -1.0), math.pi / 2)
    assert w.tolist() == [pytest.approx([3.0, 2.0, -2.0]), pytest.approx([4.0, 0.0, -1.0])]
    back = MS.to_local(MS.to_world(joints, (0.7, -2.5), 1.234), (0.7, -2.5), 1.234)
    assert back.dtype == torch.float64 and float((back - joints).abs().max()) <= 1e-12
    assert MS.to_world(joints.float(), (0.0, 0.0), 0.0).dtype == torch.float32
    # records move with the world: distances in a character's frame are the world's
    rec = MS.pack_tracks(_tracks(MS), T).double()
    d_world = torch.stack([torch.stack([R.distance(joints[t], rec[t, k]) for k in range(5)], -1) for t in range(T)])
    loc = MS.records_to_local(rec, (0.7, -2.5), 1.234)
    pl = MS.to_local(joints, (0.7, -2.5), 1.234)
    d_local = torch.stack([torch.stack([R.distance(pl[t], loc[t, k]) for k in range(5)], -1) for t in range(T)])
    assert float((d_world - d_local).abs().max()) <= 1e-12
    assert float((MS.track_distances(joints, rec) - d_world).abs().max()) <= 1e-12
    assert not MS.records_to_local(torch.zeros(3, 12), (1.0, 2.0), 0.5).any()


# ---- the restatement ----------------------------------------------------------------------------------------------------
def _case(n=T, F=263, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(1, n, F, generator=g, dtype=torch.float64) * 0.5
    mean = torch.randn(F, generator=g, dtype=torch.float64) * 0.1
    std = torch.rand(F, generator=g, dtype=torch.float64) + 0.5
    return x, mean, std


@pytest.mark.parametrize("kind", ["sphere", "capsule", "box", "half_space", "keep_in", "all"])
def test_reference_gradient_matches_finite_differences(kind):
    """One track of each kind that follows the positions (so that it penalises joints, clear of its jump set), and all of them
    with a static scene, radii, joint weights and targets: autograd against central differences of the fp64 loss."""
    F, J = 263, 22
    x, mean, std = _case(T, F, seed=3)
    P = ref_positions(x[0, :T - 1], mean, std).detach()
    jp = torch.zeros(J, 2, dtype=torch.float64)
    jp[:, 1] = 1.0
    tg = w = scene = None
    if kind == "all":
        g = torch.Generator().manual_seed(5)
        jp[:, 0] = torch.rand(J, generator=g, dtype=torch.float64) * 0.1
        jp[:, 1] = torch.rand(J, generator=g, dtype=torch.float64) * 2
        jp[3, 1] = 0.0
        tg = torch.randn(1, T, J, 3, generator=g, dtype=torch.float64)
        w = torch.rand(1, T, J, 3, generator=g, dtype=torch.float64)
        scene = R.place_scene(P, jp, 5)[None]
    full = TR.place_tracks(P, jp, 5, seed=2, T=T)
    tracks = full if kind == "all" else full[:, ["sphere", "capsule", "box", "half_space", "keep_in"].index(kind)][:, None]
    jump, share = TR.track_stats(P, tracks, jp)
    assert float(jump.min()) >= R.JUMP_CLEAR and float(share.min()) > 0.02, (jump, share)
    assert not torch.equal(tracks[0], tracks[1])  # the records do move
    loss, grad = TR.ref_tracks_loss_grad(x, [T - 1], mean, std, tracks[None], jp[None], scene, tg, w)
    assert float(loss[0]) > 0 and float(grad.abs().max()) > 0
    if kind != "all":  # the tracks term alone is the static scene's of every frame's records
        per = sum(float(R.scene_loss(P[t:t + 1], tracks[t], jp)) for t in range(T - 1))
        assert float(loss[0]) == pytest.approx(per, rel=1e-12)
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
        lp, _ = TR.ref_tracks_loss_grad(xp, [T - 1], mean, std, tracks[None], jp[None], scene, tg, w)
        lm, _ = TR.ref_tracks_loss_grad(xm, [T - 1], mean, std, tracks[None], jp[None], scene, tg, w)
        fd = float((lp - lm) / (2 * h))
        assert abs(fd - float(grad[0, t, c])) <= 1e-6 * max(1.0, abs(fd)), (kind, t, c, fd, float(grad[0, t, c]))


# ---- penetration --------------------------------------------------------------------------------------------------------
def test_penetration_with_tracks_on_hand_placed_joints():
    MS = pkg("motion_scene")
    J = 22
    joints = torch.zeros(2, 4, J, 3)
    joints[..., 1] = 1.0                                 # every joint at height 1, at the XZ origin
    ball = MS.moving_sphere([[5, 1, 0], [0.2, 1, 0], [5, 1, 0], [0, 1, 0]], 0.5, margin=0.1)  # at the joints in frames 1 and 3
    lift = MS.moving_half_space((0, 1, 0), [0.0, 0.0, 1.05, 3.0], margin=0.1)                 # a floor that rises past them
    depth, share = MS.penetration(joints, [3, 4], None, tracks=[ball])
    assert depth.tolist() == pytest.approx([0.3, 0.5]) and share.tolist() == pytest.approx([1 / 3, 2 / 4])
    depth, share = MS.penetration(joints, [3, 4], [], tracks=[[ball, lift], [lift]])
    assert depth.tolist() == pytest.approx([0.3, 2.0]) and share.tolist() == pytest.approx([2 / 3, 2 / 4])
    depth, share = MS.penetration(joints, [3, 4], None, [0.1] * J, tracks=[ball])
    assert depth.tolist() == pytest.approx([0.4, 0.6])
    # next to a static scene: the deeper of the two, a frame counts once
    depth, share = MS.penetration(joints, [3, 4], [MS.floor(1.2)], tracks=[ball])
    assert depth.tolist() == pytest.approx([0.3, 0.5]) and share.tolist() == [1.0, 1.0]
    gone = MS.moving_sphere([[0, 1, 0]] * 4, 0.5, active=np.zeros(4, bool))
    quiet = MS.moving_sphere([[0, 1, 0]] * 4, 0.5, weight=0.0)
    depth, share = MS.penetration(joints, [3, 4], None, tracks=[gone, quiet])
    assert depth.tolist() == [0.0, 0.0] and share.tolist() == [0.0, 0.0]
    assert MS.penetration(joints, [3, 4], [MS.floor(0.0)])[0].tolist() == [0.0, 0.0]  # without tracks: as before


# ---- model kwargs -------------------------------------------------------------------------------------------------------
def _kw(B=2, n=8, F=263, targets=False, scene=False):
    MS = pkg("motion_scene")
    J = (F + 1) // 12
    kw = {"control_mean": torch.zeros(B, F), "control_std": torch.ones(B, F), "control_scale": 0.5, "control_iters": 3,
          "control_tracks": MS.batch_tracks(_tracks(MS, n), B, n)}
    if scene:
        kw.update(control_scene=MS.batch_scene([MS.floor(), MS.sphere((0, 1, 0), 0.3)], B),
                  control_joint_params=MS.joint_params(J, 0.05)[None].expand(B, -1, -1))
    if targets:
        kw.update(control_joints=torch.zeros(B, n, J, 3), control_weights=torch.ones(B, n))
    return kw


def test_check_control_kwargs_accepts_tracks():
    D, MS = pkg("diffusion"), pkg("motion_scene")
    c = D.check_control_kwargs(_kw(), (2, 8, 263))  # tracks alone: no scene, no targets, still mean and std
    assert c["targets"] is None and c["tracks"].shape == (2, 8, 5, 12) and c["scene"].shape == (2, 0, 12)
    assert c["joint_params"].shape == (2, 22, 2) and c["joint_params"][0, 0].tolist() == [0.0, 1.0] and c["iters"] == 3
    assert torch.equal(c["track_bounds"], MS.track_bounds(c["tracks"])) and c["track_bounds"].shape == (2, 8, 4)
    c = D.check_control_kwargs(_kw(targets=True, scene=True), (2, 8, 263))
    assert c["targets"].shape == (2, 8, 22, 3) and c["scene"].shape == (2, 2, 12) and c["tracks"].shape == (2, 8, 5, 12)
    assert float(c["joint_params"][1, 3, 0]) == pytest.approx(0.05)
    jp_only = dict(_kw(), control_joint_params=MS.joint_params(22, 0.1)[None].expand(2, -1, -1))  # joint parameters go with tracks
    assert float(D.check_control_kwargs(jp_only, (2, 8, 263))["joint_params"][0, 0, 0]) == pytest.approx(0.1)
    assert "tracks" not in D.check_control_kwargs({k: v for k, v in _kw(targets=True).items() if k != "control_tracks"}, (2, 8, 263))
    assert D.check_control_kwargs(dict(_kw(n=202)), (2, 202, 263)) is not None


def _bad_tracks(col, v):
    MS = pkg("motion_scene")
    r = MS.batch_tracks(_tracks(MS, 8), 2, 8).clone()
    r[1, 3, 0, col] = v
    return r


@pytest.mark.parametrize("change", [
    dict(control_mean=None), dict(control_std=None), dict(control_tracks=torch.zeros(2, 8, 25, 12)),
    dict(control_tracks=torch.zeros(2, 8, 5, 11)), dict(control_tracks=torch.zeros(3, 8, 5, 12)),
    dict(control_tracks=torch.zeros(2, 7, 5, 12)), dict(control_tracks=torch.zeros(8, 5, 12)),
    dict(control_tracks=torch.zeros(2, 8, 5, 12, dtype=torch.int64)),
    dict(control_tracks=_bad_tracks(5, float("nan"))), dict(control_tracks=_bad_tracks(0, 7.0)), dict(control_tracks=_bad_tracks(1, 0.0)),
    dict(control_tracks=_bad_tracks(2, -1.0)), dict(control_tracks=_bad_tracks(7, 0.0)),
    dict(control_weights=torch.ones(2, 8)), dict(control_scale=float("nan")), dict(control_iters=0),
])
def test_check_control_kwargs_tracks_errors(change):
    D = pkg("diffusion")
    kw = {k: v for k, v in dict(_kw(), **change).items() if v is not None}
    with pytest.raises(ValueError):
        D.check_control_kwargs(kw, (2, 8, 263))


def test_tracks_frame_limit_and_the_handshake_refusal():
    D, MS = pkg("diffusion"), pkg("motion_scene")
    with pytest.raises(ValueError):  # the T limit is the scene's: 205 frames without primitives
        D.check_control_kwargs(_kw(n=206), (2, 206, 263))
    full = dict(_kw(n=203), control_scene=MS.batch_scene([MS.floor()] * 16, 2))
    with pytest.raises(ValueError):
        D.check_control_kwargs(full, (2, 203, 263))
    hs = dict(handshake_offsets=torch.tensor([0, 2]), handshake_rows=torch.tensor([7, 8]),
              handshake_weights=torch.tensor([0.5, 0.5]), handshake_owner_rows=torch.tensor([7, 8]))
    with pytest.raises(NotImplementedError):  # per-window tracks over a long motion, as a per-window scene
        D.check_handshake_kwargs(dict(_kw(), **hs), (2, 8, 263))
    with pytest.raises(NotImplementedError):
        D.check_handshake_kwargs(dict(hs, control_tracks=_kw()["control_tracks"]), (2, 8, 263))


def test_check_canvas_control_kwargs_with_tracks():
    D, MS = pkg("diffusion"), pkg("motion_scene")
    B, n, F, J = 1, 8, 263, 22
    trk = MS.canvas_tracks([_tracks(MS, 6)], [0, 6])
    base = {"canvas_control_offsets": torch.tensor([0, 6]), "canvas_control_rows": torch.arange(6),
            "canvas_control_mean": torch.zeros(1, F), "canvas_control_std": torch.ones(1, F), "canvas_control_tracks": trk}
    c = D.check_canvas_control_kwargs(base, (B, n, F))
    assert c["targets"] is None and c["scene"].shape == (1, 0, 12) and c["tracks"].shape == (6, 5, 12) and c["total"] == 6
    assert torch.equal(c["track_bounds"], MS.track_bounds(trk)) and c["joint_params"].shape == (1, J, 2)
    both = dict(base, canvas_control_joints=torch.zeros(6, J, 3), canvas_control_weights=torch.ones(6),
                canvas_control_scene=MS.batch_scene([MS.floor()], 1))
    c = D.check_canvas_control_kwargs(both, (B, n, F))
    assert c["targets"].shape == (6, J, 3) and c["scene"].shape == (1, 1, 12) and c["tracks"].shape == (6, 5, 12)
    assert D.check_control_kwargs(dict(base, control_scale=0.1), (B, n, F)) is None  # the scale is the canvas control's
    for change in (dict(canvas_control_mean=None), dict(canvas_control_rows=None), dict(canvas_control_tracks=torch.zeros(5, 5, 12)),
                   dict(canvas_control_tracks=torch.zeros(6, 25, 12)), dict(canvas_control_tracks=torch.zeros(1, 6, 5, 12)),
                   dict(control_tracks=torch.zeros(1, 8, 2, 12))):
        kw = {k: v for k, v in dict(base, **change).items() if v is not None}
        with pytest.raises(ValueError):
            D.check_canvas_control_kwargs(kw, (B, n, F))
    with pytest.raises(ValueError, match="whole long motions"):
        pkg("dist").shard_kwargs(base, 0, 1)


def test_shard_kwargs_gives_each_rank_its_rows():
    Dist, MS = pkg("dist"), pkg("motion_scene")
    kw = _kw(B=5, scene=True)
    kw["control_tracks"] = MS.batch_tracks([_tracks(MS, 8)[:1 + i % 3] for i in range(5)], 5, 8)
    for lo, hi in ((0, 3), (3, 5)):
        s = Dist.shard_kwargs(kw, lo, hi)
        for k in ("control_tracks", "control_scene", "control_joint_params", "control_mean"):
            assert torch.equal(s[k], kw[k][lo:hi]), k
        c = pkg("diffusion").check_control_kwargs(s, (hi - lo, 8, 263))
        assert c["tracks"].shape == (hi - lo, 8, 3, 12) and torch.equal(c["track_bounds"], MS.track_bounds(kw["control_tracks"][lo:hi]))


# ---- trainer arguments --------------------------------------------------------------------------------------------------
def test_trainer_tracks_arguments():
    Cond, MS = pkg("conditioning").Conditioning, pkg("motion_scene")
    caps = ["a", "b", "c"]
    mean, std = np.zeros(263, np.float32), np.ones(263, np.float32)
    trk = _tracks(MS, 10)
    c = Cond(caps, 263, scene_tracks=trk, mean=mean, std=std, control_scale=0.3)
    kw = c.control_kwargs(slice(1, 3), 6, "cpu")  # a batch takes its rows and its first T frames
    assert "control_joints" not in kw and kw["control_tracks"].shape == (2, 6, 5, 12) and kw["control_scene"].shape == (2, 0, 12)
    assert torch.equal(kw["control_tracks"][0], MS.pack_tracks(trk, 6)) and kw["control_scale"] == 0.3
    assert pkg("diffusion").check_control_kwargs(kw, (2, 6, 263))["tracks"].shape == (2, 6, 5, 12)
    kw = c.control_kwargs(slice(0, 3), 12, "cpu")  # past the tracks' end: padding
    assert kw["control_tracks"].shape == (3, 12, 5, 12) and not kw["control_tracks"][:, 10:].any()
    per = [trk[:2], [], trk]
    c = Cond(caps, 263, scene_tracks=per, scene=[MS.floor()], scene_joint_radius=[0.1] * 22, mean=mean, std=std,
             control_joints=torch.zeros(3, 10, 22, 3), control_weights=torch.ones(3))
    kw = c.kwargs(torch.tensor([2, 0]), 10, "cpu")
    assert kw["control_tracks"].shape == (2, 10, 5, 12) and kw["control_scene"].shape == (2, 1, 12)
    assert kw["control_tracks"][0, 0, 4, 0] == 3 and not kw["control_tracks"][1, :, 2:].any()
    assert float(kw["control_joint_params"][1, 21, 0]) == pytest.approx(0.1)
    for bad in (dict(scene_tracks=trk), dict(scene_tracks=trk, mean=mean), dict(scene_tracks=per[:2], mean=mean, std=std),
                dict(scene_tracks=trk * 5, mean=mean, std=std), dict(scene_tracks=[torch.zeros(10, 11)], mean=mean, std=std)):
        with pytest.raises(ValueError):
            Cond(caps, 263, **bad)
    Tr = pkg("trainer")
    tr = Tr.DDPMTrainer.__new__(Tr.DDPMTrainer)  # the checks run before anything touches a device
    tr.encoder, tr.device = types.SimpleNamespace(num_frames=16, eval=lambda: None), "cpu"
    lens = torch.tensor([16, 12, 8])
    for method in (tr.generate_batch, tr.generate, tr.generate_bucketed):
        with pytest.raises(ValueError, match="mean and std"):
            method(caps, lens, 263, scene_tracks=trk)
        with pytest.raises(ValueError, match="at most 24"):
            method(caps, lens, 263, scene_tracks=trk * 5, mean=mean, std=std)
    with pytest.raises(ValueError, match="one list of track stacks per motion"):
        tr.generate_long([[("a", 16)]], 263, overlap=4, scene_tracks=trk, mean=mean, std=std)
    with pytest.raises(ValueError, match="mean and std"):
        tr.generate_long([[("a", 16)]], 263, overlap=4, scene_tracks=[trk])
    with pytest.raises(ValueError, match="at most 24"):  # through an output method's **kw
        tr.generate_joints(caps, lens, 263, mean, std, scene_tracks=trk * 5)
    with pytest.raises(ValueError, match="at most 24"):  # two earlier characters with every bone: 42 tracks
        fake = types.SimpleNamespace(generate_joints=lambda caps, lens, *a, **k: [torch.zeros(int(n), 22, 3) for n in lens])
        Tr.DDPMTrainer.generate_together(fake, [[dict(caption="a", length=8)] * 3], 263, mean, std)


def test_generate_together_stages_on_a_stand_in():
    """The staging alone, on a stand-in for ``generate_joints`` that records its arguments: stage i sees the earlier characters
    of its own scene as 21 capsule tracks in its own frame, world targets and primitives moved the same way, ``seed + i``."""
    Tr, MS = pkg("trainer"), pkg("motion_scene")
    calls = []

    def fake_joints(caps, lens, dim_pose, mean, std, **kw):
        calls.append(dict(kw, caps=list(caps), lens=lens.tolist()))
        g = torch.Generator().manual_seed(len(calls))
        return [torch.randn(int(n), 22, 3, generator=g) for n in lens]

    fake = types.SimpleNamespace(generate_joints=fake_joints)
    tg = torch.zeros(6, 22, 3)
    tg[:, 0] = torch.tensor([2.0, 0.9, 1.0])
    scenes = [[dict(caption="a", length=8, position=(1.0, 0.0), yaw=0.5),
               dict(caption="b", length=6, position=(0.0, 2.0), yaw=-1.0, control_joints=tg, control_weights=torch.ones(6, 22),
                    scene=[MS.sphere((2.0, 1.0, 1.0), 0.4)])],
              [dict(caption="c", length=4)]]
    mean, std = np.zeros(263, np.float32), np.ones(263, np.float32)
    out = Tr.DDPMTrainer.generate_together(fake, scenes, 263, mean, std, radius=0.1, margin=0.02, weight=3.0, seed=7, sampler="ddim")
    assert [len(s) for s in out] == [2, 1] and [tuple(j.shape) for j in out[0]] == [(8, 22, 3), (6, 22, 3)]
    assert calls[0]["caps"] == ["a", "c"] and calls[0]["lens"] == [8, 4] and calls[0]["seed"] == 7 and calls[0]["sampler"] == "ddim"
    assert "scene_tracks" not in calls[0] and "scene" not in calls[0] and "control_joints" not in calls[0]
    assert calls[1]["caps"] == ["b"] and calls[1]["seed"] == 8
    trk = calls[1]["scene_tracks"]
    assert len(trk) == 1 and len(trk[0]) == 21 and tuple(trk[0][0].shape) == (8, 12)
    first = MS.to_local(out[0][0], (0.0, 2.0), -1.0).double()  # character 0, already in the world, in character 1's frame
    assert float((trk[0][0][:, 7:10] - first[:, 1]).abs().max()) <= 1e-6 and trk[0][0][0, [2, 3, 10]].tolist() == [3.0, 0.02, 0.1]
    local = MS.to_local(torch.tensor([2.0, 0.9, 1.0]), (0.0, 2.0), -1.0)
    assert float((calls[1]["control_joints"][0, :, 0] - local).abs().max()) <= 1e-6 and calls[1]["control_weights"].shape == (1, 6, 22, 3)
    centre = MS.to_local(torch.tensor([2.0, 1.0, 1.0]), (0.0, 2.0), -1.0)
    assert float((calls[1]["scene"][0, 0, 4:7] - centre).abs().max()) <= 1e-6 and calls[1]["scene"][0, 0, 7] == pytest.approx(0.4)


def test_canvas_control_takes_tracks_per_motion():
    ML, MS = pkg("motion_long"), pkg("motion_scene")
    plans = ML.script_plans([[("a", 16), ("b", 12)], [("c", 10)]], 4, 16)
    mean, std = np.zeros(263, np.float32), np.ones(263, np.float32)
    tracks = [_tracks(MS, 24), _tracks(MS, 10)[:2]]
    tables = ML.canvas_control(plans, 263, mean=mean, std=std, scene_tracks=tracks, scene_joint_radius=[0.1] * 22, control_iters=2)
    kw = tables([1, 0], 16)
    assert "canvas_control_joints" not in kw and kw["canvas_control_tracks"].shape == (10 + 24, 5, 12) and kw["control_iters"] == 2
    assert not kw["canvas_control_tracks"][:10, 2:].any() and kw["canvas_control_tracks"][10, 4, 0] == 3
    assert kw["canvas_control_scene"].shape == (2, 0, 12) and kw["canvas_control_joint_params"].shape == (2, 22, 2)
    full = dict(kw, **ML.batch_tables(plans, [1, 0], 16, 4), length=torch.tensor([10, 16, 12]))
    c = pkg("diffusion").check_canvas_control_kwargs(full, (3, 16, 263))
    assert c["targets"] is None and c["tracks"].shape == (34, 5, 12) and c["track_bounds"].shape == (34, 4)
    assert tables([1], 16)["canvas_control_tracks"].shape == (10, 2, 12)
    for bad in (dict(scene_tracks=tracks), dict(scene_tracks=tracks, mean=mean), dict(scene_tracks=tracks[0], mean=mean, std=std),
                dict(scene_tracks=tracks[:1], mean=mean, std=std), dict(scene_tracks=[tracks[0], None], mean=mean, std=std),
                dict(scene_tracks=[tracks[0] * 5, []], mean=mean, std=std)):
        with pytest.raises(ValueError):
            ML.canvas_control(plans, 263, **bad)


# ---- the C entries ------------------------------------------------------------------------------------------------------
def test_argument_validation_without_gpu():
    """Every refusal happens before the launch, so it shows without a device (as tests/test_abi.py's)."""
    lib = pkg("_lib").lib()
    buf = (C.c_float * 64)()
    p = (C.addressof(buf) + 15) // 16 * 16  # records and bounds are read 16 bytes at a time
    ok = dict(x0=p, length=p, mean=p, std=p, targets=p, weights=p, scene=p, K=4, jp=p, tracks=p, Km=5, bounds=p, B=0, T=8, F=263,
              loss=p, grad=p)

    def lg(**ch):
        a = dict(ok, **ch)
        return lib.mdm_joint_tracks_loss_grad(a["x0"], a["length"], a["mean"], a["std"], a["targets"], a["weights"], a["scene"],
                                              a["K"], a["jp"], a["tracks"], a["Km"], a["bounds"], a["B"], a["T"], a["F"], a["loss"],
                                              a["grad"], None)

    assert lg() == 0 and lg(bounds=None) == 0 and lg(targets=None, weights=None) == 0 and lg(K=0, scene=None) == 0
    assert lg(Km=0, tracks=None) == 0 and lg(Km=24) == 0
    for ch in (dict(Km=25), dict(Km=-1), dict(tracks=None), dict(tracks=p + 4), dict(bounds=p + 8), dict(K=17), dict(K=-1),
               dict(scene=None), dict(jp=None), dict(targets=None), dict(weights=None), dict(x0=None), dict(T=203, K=16),
               dict(T=0), dict(F=262), dict(B=-1), dict(loss=None), dict(grad=None), dict(mean=None), dict(Km=0, K=17),
               dict(Km=0, tracks=None, jp=None)):
        assert lg(**ch) == 1, ch

    def gd(**ch):
        a = dict(dict(ok, iters=1, steps=10, scale=0.1), **ch)
        return lib.mdm_joint_tracks_guidance(p, p, None, p, p, p, a["targets"], a["weights"], a["scene"], a["K"], a["jp"], a["tracks"],
                                             a["Km"], a["bounds"], a["B"], a["T"], a["F"], a["scale"], a["iters"], p, a["steps"], None,
                                             0, None)

    assert gd() == 0 and gd(bounds=None) == 0 and gd(Km=0, tracks=None) == 0
    for ch in (dict(Km=25), dict(Km=-1), dict(tracks=None), dict(tracks=p + 4), dict(K=17), dict(jp=None), dict(weights=None),
               dict(T=206), dict(iters=0), dict(iters=33), dict(scale=float("inf")), dict(steps=0)):
        assert gd(**ch) == 1, ch

    def cl(**ch):
        a = dict(dict(ok, M=0), **ch)
        return lib.mdm_canvas_tracks_loss_grad(p, p, p, p, p, a["targets"], a["weights"], a["scene"], a["K"], a["jp"], a["tracks"],
                                               a["Km"], a["bounds"], a["M"], a["F"], a["loss"], a["grad"], p, None)

    assert cl() == 0 and cl(bounds=None) == 0 and cl(Km=0, tracks=None) == 0 and cl(targets=None, weights=None) == 0
    for ch in (dict(Km=25), dict(Km=-1), dict(tracks=None), dict(bounds=p + 4), dict(K=17), dict(jp=None), dict(targets=None),
               dict(F=262), dict(M=-1), dict(loss=None)):
        assert cl(**ch) == 1, ch

    def cg(**ch):
        a = dict(dict(ok, M=0, iters=1, steps=10, scale=0.1), **ch)
        return lib.mdm_canvas_tracks_guidance(p, p, None, p, p, p, p, a["targets"], a["weights"], a["scene"], a["K"], a["jp"],
                                              a["tracks"], a["Km"], a["bounds"], a["M"], a["F"], a["scale"], a["iters"], p, a["steps"],
                                              None, 0, p, None)

    assert cg() == 0 and cg(bounds=None) == 0 and cg(Km=0, tracks=None) == 0
    for ch in (dict(Km=25), dict(Km=-1), dict(tracks=None), dict(tracks=p + 4), dict(K=17), dict(scene=None), dict(jp=None),
               dict(weights=None), dict(F=262), dict(M=-1), dict(iters=0), dict(iters=33), dict(scale=float("nan")), dict(steps=0)):
        assert cg(**ch) == 1, ch

"""GPU: the world view (mdm_world_render) against its restatement tests/world_render_ref.py.

* parity on a static scene with one primitive of each kind (a sphere, a capsule, a yawed box, a wall half-space, floor()):
  B = 2 worlds, C = 2 characters, T = 5, lengths [[5, 3], [2, 0]] (one character ends early, one is absent), 48 x 64, at the
  fitted camera and at elev 60 / azim 135 / dist 4 / fov 60, and once with KIT joints;
* tracks: a moving sphere, a moving box whose yaw changes per frame, a record inactive in frames 1 and 3, character_tracks;
* order: two characters swap which is nearer between frames 1 and 3 with a box between them, asserted on the device output;
* the near plane through a box, a capsule and a bone, a sphere dropped by it; a keep-in box; non-default style values;
  T = 300 at 24 x 32 with frames= around the trajectory's chunk boundary and two characters;
* bit for bit: NaN past every length, a world against its own run at B = 1, palette mode, frames=, a character of alpha 0;
* through a tiny trainer: generate_together_frames, generate_frames(view="world"), view="root" untouched, generate_together_gif.

The gate.  Every pixel of every frame within ONE grey level of the fp64 restatement, none left out: coverage and compositing
are continuous (slope <= 1 per pixel of distance) in the projected coordinates, whose fp32 error is about 1e-3 pixel.  Two
decisions are not continuous, the order of the items and which faces of a box the eye sees, and neither gets a tolerance:
``truth`` asserts on the test's own inputs, from the fp64 restatement, that in every tested frame consecutive depth keys differ by
>= 1e-3 m and every |e_axis - h_axis| of every box is >= 1e-3 m, three orders above fp32's error at these distances, and that
the fp32 restatement then agrees with the fp64 one to one level.  Both shares of differing pixels are printed.
tests/test_world_render_host.py shows that each likely mistake moves >= 20 pixels by >= 64 levels.
"""
import numpy as np
import pytest
import torch

from conftest import pkg

import render_ref as RR
import world_render_ref as WR

pytestmark = pytest.mark.gpu

H, W = 48, 64
CAMERA2 = dict(elev=60.0, azim=135.0, dist=4.0, fov=60.0)
FRONT = dict(elev=5.0, azim=0.0, dist=5.0, fov=40.0, target=(0.0, 0.7, 0.0))
MARGIN = 1e-3  # metres
_MEMO = {}


def memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def truth(what, sk, joints, lens, prims, tracks, size, camera, style=None, ground=None, frames=None):
    """The fp64 restatement of a batch, after the conditions on the inputs: the two discontinuous decisions are at least
    MARGIN away from flipping, and the fp32 restatement agrees with the fp64 one to one level.  CPU only."""
    keys = []
    w64 = WR.render(sk.chains, joints, lens, prims, tracks, size[0], size[1], camera, style, ground, np.float64, frames, keys_out=keys)
    w32 = WR.render(sk.chains, joints, lens, prims, tracks, size[0], size[1], camera, style, ground, np.float32, frames)
    gap, face = WR.margins(keys)
    own = np.abs(w32.astype(np.int32) - w64.astype(np.int32))
    print(f"{what}: depth keys at least {gap:.2e} m apart, box faces at least {face:.2e} m from turning; the fp32 restatement: "
          f"worst {int(own.max())}, {100 * (own > 0).any(-1).mean():.3f} % of pixels differ")
    assert gap >= MARGIN and face >= MARGIN, (what, gap, face)
    assert int(own.max()) <= 1, (what, int(own.max()))
    return w64


def held(what, got, w64):
    """The gate: got (B, NF, H, W, 3) uint8 within one grey level of the fp64 restatement on every pixel."""
    assert got.shape == w64.shape and got.dtype == np.uint8, (what, got.shape, w64.shape)
    d = np.abs(got.astype(np.int32) - w64.astype(np.int32))
    print(f"{what}: worst {int(d.max())} level(s), {100 * (d > 0).any(-1).mean():.3f} % of pixels differ")
    assert int(d.max()) <= 1, (what, int(d.max()), int((d > 1).sum()))


def render(joints, lens, prims=None, tracks=None, **kw):
    R = pkg("motion_render")
    return R.render_world(torch.from_numpy(np.asarray(joints)).cuda(), lens, scene=None if prims is None else torch.from_numpy(prims),
                          tracks=None if tracks is None else torch.from_numpy(tracks), **kw)


def fitted(joints, lens, prims=None, tracks=None, size=(H, W)):
    """The camera render_world(camera=None) fits, as the restatement's dict."""
    R = pkg("motion_render")
    ext = R.world_extent(torch.from_numpy(joints).cuda(), lens, None if prims is None else torch.from_numpy(prims),
                         None if tracks is None else torch.from_numpy(tracks))
    return R.fit_camera(ext, size=size), ext


@pytest.mark.parametrize("name,camera", [("t2m", None), ("t2m", CAMERA2), ("kit", None)], ids=["t2m-fitted", "t2m-elev60", "kit-fitted"])
def test_parity_static_scene(name, camera):
    sk, j, lens, prims = memo(("static", name), lambda: WR.static_world(name))
    out = render(j, lens, prims, size=(H, W), camera=camera)
    assert out.shape == (2, 5, H, W, 3) and out.dtype == torch.uint8 and out.is_cuda
    cam = camera
    if camera is None:
        fit, ext = fitted(j, lens, prims)
        for b in range(2):  # the extent, computed on the device
            lo, hi = WR.extent(j[b], lens[b], prims[b], np.zeros((5, 0, 12)))
            assert np.allclose(ext[b].cpu().numpy(), np.concatenate([lo, hi]), rtol=0, atol=1e-6)
        cam = WR.camera_dict(fit)
        assert torch.equal(render(j, lens, prims, size=(H, W), camera=fit), out)  # one camera for the batch, fitted per call
    got = out.cpu().numpy()
    w64 = truth(f"static {name}", sk, j, lens, prims, None, (H, W), cam)
    held(f"static {name} {'fitted' if camera is None else 'elev 60'}", got, w64)
    assert not got[1, 2:].any() and (got[0] != 255).any(-1).reshape(5, -1).sum(-1).min() > 100  # zeros past a world's length
    assert not np.array_equal(got[0, 2], got[0, 3])  # the second character has left


def test_tracks():
    sk = WR.skel("t2m")
    j, lens, tracks = memo("tracks", lambda: WR.track_world(sk))
    assert tracks.shape == (1, 5, 11, 12) and not tracks[0, [1, 3], 2].any() and tracks[0, [0, 2, 4], 2, 0].all()
    cam = dict(elev=25.0, azim=20.0, dist=4.5, fov=45.0, target=(0.2, 0.6, 0.0))
    w64 = truth("tracks", sk, j, lens, None, tracks, (H, W), cam)
    held("tracks", render(j, lens, None, tracks, size=(H, W), camera=cam).cpu().numpy(), w64)
    assert RR.moved(w64[0, 0], w64[0, 4]) >= 20 and RR.moved(w64[0, 2], w64[0, 3]) >= 20  # things move, one flickers


def test_order():
    """Characters in one colour each on the camera's axis, a thin box between them: in frames 1 and 2 character 0 is the
    nearer, in frame 3 character 1, and the pixel at the centre of where all three overlap has the nearer one's colour."""
    sk = WR.skel("t2m")
    j, lens, prims = memo("order", lambda: WR.order_world(sk))
    style = dict(character_colors=((RR.RED,), (RR.BLUE,)), chain_width=40.0, solid_alpha=1.0)
    w64 = truth("order", sk, j, lens, prims, None, (H, W), FRONT, style)
    got = render(j, lens, prims, size=(H, W), camera=FRONT, **style).cpu().numpy()
    held("order", got, w64)
    for t, colour in ((1, (255, 0, 0)), (2, (255, 0, 0)), (3, (0, 0, 255))):
        y, x = _overlap_centre(sk, j, lens, prims, style, t)
        print(f"order: frame {t}, pixel ({y}, {x}) at the centre of the overlap: {got[0, t, y, x]}")
        assert tuple(got[0, t, y, x]) == colour, (t, got[0, t, y, x])


def _overlap_centre(sk, j, lens, prims, style, t):
    """The pixel nearest to the centroid of those that each character alone and the box alone paint in full in frame t."""
    ink = dict(style, character_colors=((RR.BLACK,),), solid_color=RR.BLACK, edge_color=RR.BLACK, floor_alpha=0.0, trajectory_alpha=0.0)
    full = [(WR.render(sk.chains, j[:, c:c + 1], lens[:, c:c + 1], None, None, H, W, FRONT, ink, 0.0, frames=[t])[0, 0] == 0).all(-1)
            for c in (0, 1)]
    full.append((WR.render(sk.chains, j, lens, prims, None, H, W, FRONT, dict(ink, chain_alpha=0.0), 0.0, frames=[t])[0, 0] == 0).all(-1))
    ys, xs = np.nonzero(full[0] & full[1] & full[2])
    assert len(ys) >= 3, (t, len(ys))
    k = int(np.argmin((ys - ys.mean()) ** 2 + (xs - xs.mean()) ** 2))
    return int(ys[k]), int(xs[k])


def _near_world():
    MS = pkg("motion_scene")
    sk = WR.skel("t2m")
    cam = dict(elev=10.0, azim=20.0, dist=1.0, fov=60.0, target=(0.0, 0.6, 0.0), near=0.5)
    eye, r, u, f = RR.camera_basis(cam, np.float64)
    at = lambda z, x=0.0, y=0.0: tuple(eye + z * f + x * r + y * u)  # noqa: E731
    prims = MS.batch_scene([MS.box(at(0.62, 0.45, -0.1), (0.2, 0.15, 0.2), yaw=0.3), MS.capsule(at(0.2, -0.45), at(1.6, -0.3, 0.2), 0.06),
                            MS.sphere(at(0.7, 0.0, 0.35), 0.3), MS.sphere(at(1.8, 0.5, 0.3), 0.2)], 1).numpy()
    walk = RR.walk(sk, 3, 4)
    spot = np.array(at(0.55, 0.05))
    j, lens = WR.world([[(walk - walk[0, 0] * np.array([1, 0, 1], np.float32) + np.array([spot[0], 0, spot[2]], np.float32)).astype(np.float32)]])
    return sk, j, lens, prims, cam


def test_the_near_plane():
    """The near plane cuts through a box, a capsule and a bone, and drops a sphere (another one stays)."""
    sk, j, lens, prims, cam = memo("near", _near_world)
    eye, r, u, f = RR.camera_basis(cam, np.float64)
    depth = lambda p: (np.asarray(p, np.float64) - eye) @ f  # noqa: E731
    centre, h, co, si, _ = WR.box_frame(prims[0, 0], eye, np.float64)
    corners = [depth(centre + np.array([co * a * h[0] + si * c * h[2], b * h[1], -si * a * h[0] + co * c * h[2]]))
               for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)]
    assert min(corners) < cam["near"] < max(corners)
    assert depth(prims[0, 1, 4:7]) < cam["near"] < depth(prims[0, 1, 7:10])
    assert depth(prims[0, 2, 4:7]) - prims[0, 2, 7] < cam["near"] < depth(prims[0, 2, 4:7]) and depth(prims[0, 3, 4:7]) - prims[0, 3, 7] > cam["near"]
    d = depth(j[0, 0, 1])
    assert any((d[a] < cam["near"]) != (d[b] < cam["near"]) for c in sk.chains for a, b in zip(c[:-1], c[1:]))
    w64 = truth("near plane", sk, j, lens, prims, None, (H, W), cam, None, 0.0)
    held("near plane", render(j, lens, prims, size=(H, W), camera=cam, ground=0.0).cpu().numpy(), w64)
    gone = prims.copy()
    gone[0, 2] = 0  # the dropped sphere draws what padding draws
    assert torch.equal(render(j, lens, gone, size=(H, W), camera=cam, ground=0.0), render(j, lens, prims, size=(H, W), camera=cam, ground=0.0))


def test_keep_in_box_and_style():
    MS = pkg("motion_scene")
    sk, j, lens, prims = memo(("static", "t2m"), lambda: WR.static_world("t2m"))
    room = MS.batch_scene([MS.floor(0.1), MS.box((0.0, 1.0, 0.0), (1.6, 0.9, 1.4), yaw=-0.2, inside=True), MS.sphere((0, 3, 0), 0.5, inside=True),
                           MS.half_space((1, 0, 0), -3.0, inside=True)], 2).numpy()
    cam = dict(elev=25.0, azim=20.0, dist=5.0, fov=45.0, target=(0.2, 0.6, 0.0))
    wide = dict(edge_width=30.0)  # a half-width of one pixel: an edge's middle has the edge colour itself
    w64 = truth("keep-in", sk, j, lens, room, None, (H, W), cam, wide)
    held("keep-in", render(j, lens, room, size=(H, W), camera=cam, **wide).cpu().numpy(), w64)
    edge = np.floor(np.asarray(pkg("motion_render").WORLD_STYLE["edge_color"]) * 255 + 0.5)
    assert (np.abs(w64[0, 0] - edge).max(-1) <= 1).sum() > 40  # its edges are there
    keep_out = room.copy()
    keep_out[:, 1:, 1] = 1.0
    keep_out[:, 2:, 0] = 0.0  # the same box as an obstacle: the same extent, and faces
    faces = np.abs(WR.render(sk.chains, j, lens, keep_out, None, H, W, cam, wide)[0, 0].astype(int) - w64[0, 0]).max(-1) > 8
    assert faces.sum() > 300  # and no face; the keep-in sphere and half-space draw nothing (the restatement skips them)
    style = dict(background=(0.1, 0.2, 0.3), floor_color=(0.9, 0.8, 0.1), floor_alpha=0.8, trajectory_colors=((0.0, 1.0, 0.0), (1.0, 0.0, 1.0)),
                 trajectory_alpha=(0.6, 1.0), trajectory_width=9.0, character_colors=(((1.0, 1.0, 0.0), (0.0, 1.0, 1.0)), ((1.0, 1.0, 1.0),)),
                 chain_alpha=((1.0, 0.5, 0.75, 0.25, 1.0),) * 2, chain_width=((2.0, 4.0, 8.0, 16.0, 32.0), (6.0,) * 5),
                 solid_color=(0.9, 0.3, 0.2), solid_alpha=0.6, edge_color=(1.0, 1.0, 1.0), edge_width=6.0, shade=(0.9, 0.5, 0.3))
    w64 = truth("style", sk, j, lens, prims, None, (H, W), cam, style)
    got = render(j, lens, prims, size=(H, W), camera=cam, **style).cpu().numpy()
    held("style", got, w64)
    assert not np.array_equal(got, render(j, lens, prims, size=(H, W), camera=cam).cpu().numpy())


def test_trajectory_chunks():
    """T = 300, two characters: the trajectory of frame 258 and later has more than 256 segments and goes through LDS in two
    chunks."""
    sk = WR.skel("t2m")
    j, lens = memo("long", lambda: WR.world([[WR.placed(sk, 300, 5, 0.0, 0.0), WR.placed(sk, 280, 6, 1.0, -1.0)]]))
    pick = [0, 1, 2, 256, 257, 258, 279, 280, 299]
    cam, _ = fitted(j, lens, size=(24, 32))
    for style in (None, dict(trajectory_width=60.0)):  # a stroke a pixel wide: every chunk's segments show
        w64 = truth("T 300", sk, j, lens, None, None, (24, 32), WR.camera_dict(cam), style, frames=pick)
        out = render(j, lens, size=(24, 32), frames=pick, **(style or {}))
        assert out.shape == (1, 9, 24, 32, 3)
        held("T 300", out.cpu().numpy(), w64)


def test_bit_for_bit():
    """NaN past every character's length changes nothing; a world equals its own run at B = 1; palette mode is the index of
    the RGB output; frames= equals the same frames of the full render; a character whose alphas are all 0 equals the render
    without it (inside a keep-in box that fixes the extent)."""
    R, MS = pkg("motion_render"), pkg("motion_scene")
    sk, j, lens, prims = memo(("static", "t2m"), lambda: WR.static_world("t2m"))
    _, _, tracks = memo("tracks", lambda: WR.track_world(sk))
    tracks = np.repeat(tracks, 2, 0)
    cam = dict(elev=25.0, azim=20.0, dist=5.0, fov=45.0, target=(0.2, 0.6, 0.0))
    for kw in (dict(camera=cam), dict(camera=cam, palette=True), dict(camera=None)):
        clean = render(j, lens, prims, tracks, size=(H, W), **kw)
        bad, far = j.copy(), tracks.copy()
        for b in range(2):
            far[b, lens[b].max():] = [1, 1, 1, 0, 1e6, 1e6, 1e6, 1, 0, 0, 0, 0]  # a far sphere past the world's length: not read
            for c in range(2):
                bad[b, c, lens[b, c]:] = np.nan
        assert torch.equal(render(bad, lens, prims, far, size=(H, W), **kw), clean), kw
        assert not clean[1, 2:].any()
    full = render(j, lens, prims, tracks, size=(H, W), camera=cam)
    for b in range(2):
        assert torch.equal(render(j[b:b + 1], lens[b:b + 1], prims[b:b + 1], tracks[b:b + 1], size=(H, W), camera=cam)[0], full[b]), b
    idx = render(j, lens, prims, tracks, size=(H, W), camera=cam, palette=True)
    want = R.palette_index(full)
    assert idx.shape == (2, 5, H, W) and torch.equal(idx[0], want[0]) and torch.equal(idx[1, :2], want[1, :2]) and not idx[1, 2:].any()
    assert len(torch.unique(idx)) > 5
    for frames, pick in ((slice(1, None, 2), [1, 3]), (2, [0, 2, 4]), ([4, 0, 3, 3], [4, 0, 3, 3])):
        assert torch.equal(render(j, lens, prims, tracks, size=(H, W), camera=cam, frames=frames), full[:, pick]), frames
    room = MS.batch_scene(WR.static_scene() + [MS.box((0.0, 1.0, 0.0), (3.0, 1.5, 3.0), inside=True)], 2).numpy()
    hidden = render(j, lens, room, size=(H, W), camera=cam, chain_alpha=((1.0,) * 5, (0.0,) * 5), trajectory_alpha=(1.0, 0.0))
    without = lens.copy()
    without[:, 1] = 0
    assert torch.equal(hidden[0], render(j, without, room, size=(H, W), camera=cam)[0])
    assert not torch.equal(hidden[0], render(j, lens, room, size=(H, W), camera=cam)[0])


# ---- through a tiny trainer ----------------------------------------------------------------------------------------------
FAR = dict(dist=8000.0, target=(0.0, 0.0, 0.0))  # the tiny model's joints spread over some 2000 m (test_motion_render_gpu)
OPTS = dict(seed=0, sampler="ddim", sample_steps=5)


def _trainer():
    import test_motion_features_gpu as TF
    return memo("trainer", TF._tiny_trainer)


def _stats():
    import test_motion_fk_gpu as TK
    return TK._mean_std(263, 22, 12)


def test_together_frames_are_render_world_of_generate_together():
    R, MS = pkg("motion_render"), pkg("motion_scene")
    tr = _trainer()
    mean, std = _stats()
    table = [MS.box((50.0, 0.5, 20.0), (30.0, 0.5, 20.0), yaw=0.4), MS.floor(0.0)]
    scenes = [[dict(caption="a", length=16, scene=table), dict(caption="b", length=12, position=(300.0, -200.0), yaw=0.7, scene=table)],
              [dict(caption="c", length=12, scene=[MS.sphere((0.0, 100.0, 0.0), 40.0)])]]
    kw = dict(OPTS, bones=[(0, 3), (3, 6)], weight=0.0)
    worlds = tr.generate_together(scenes, 263, mean, std, **kw)
    frames = tr.generate_together_frames(scenes, 263, mean, std, size=(H, W), camera=FAR, style=dict(chain_width=24.0), **kw)
    assert [tuple(f.shape) for f in frames] == [(16, H, W, 3), (12, H, W, 3)]
    want = R.render_world(worlds, scene=[table, scenes[1][0]["scene"]], size=(H, W), camera=FAR, chain_width=24.0)
    assert torch.equal(frames[0], want[0, :16]) and torch.equal(frames[1], want[1, :12]) and not want[1, 12:].any()
    assert len(torch.unique(frames[0].reshape(-1, 3), dim=0)) > 3


def test_generate_frames_world_and_root_views():
    R, MS = pkg("motion_render"), pkg("motion_scene")
    tr = _trainer()
    mean, std = _stats()
    caps, lens = ["a", "b"], torch.tensor([16, 12])
    scene = [MS.floor(0.0), MS.box((100.0, 50.0, 0.0), (60.0, 50.0, 80.0), yaw=0.3)]
    joints = tr.generate_joints(caps, lens, 263, mean, std, scene=scene, **OPTS)
    frames = tr.generate_frames(caps, lens, 263, mean, std, scene=scene, view="world", size=(H, W), camera=FAR, palette=True, **OPTS)
    want = R.render_world([[jn] for jn in joints], scene=scene, size=(H, W), camera=FAR, palette=True)
    assert [tuple(f.shape) for f in frames] == [(16, H, W), (12, H, W)]
    assert torch.equal(frames[0], want[0]) and torch.equal(frames[1], want[1, :12])
    fitted_frames = tr.generate_frames(caps, lens, 263, mean, std, scene=scene, view="world", size=(H, W), **OPTS)  # camera=None fits
    assert torch.equal(fitted_frames[1], R.render_world([[jn] for jn in joints], scene=scene, size=(H, W))[1, :12])
    plain = tr.generate_joints(caps, lens, 263, mean, std, **OPTS)
    for root in (tr.generate_frames(caps, lens, 263, mean, std, size=(H, W), **OPTS),
                 tr.generate_frames(caps, lens, 263, mean, std, size=(H, W), view="root", **OPTS)):
        for f, jn in zip(root, plain):
            assert torch.equal(f, R.render_motion(jn[None], size=(H, W))[0])
    with pytest.raises(ValueError, match="view"):
        tr.generate_frames(caps, lens, 263, mean, std, size=(H, W), view="sky", **OPTS)


def test_generate_together_gif_writes_the_worlds_length(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    R = pkg("motion_render")
    tr = _trainer()
    mean, std = _stats()
    scenes = [[dict(caption="a", length=16), dict(caption="b", length=10, position=(200.0, 100.0))]]  # a stage is a batch: even lengths
    kw = dict(OPTS, bones=[(0, 3)], weight=0.0, size=(H, W), camera=FAR, style=dict(chain_width=24.0))
    path = str(tmp_path / "w.gif")
    assert tr.generate_together_gif(scenes, 263, mean, std, paths=[path], **kw) == [path]
    idx = tr.generate_together_frames(scenes, 263, mean, std, palette=True, **kw)[0]
    assert tuple(idx.shape) == (16, H, W) and min(int((idx[t] != idx[t - 1]).sum()) for t in range(1, 16)) > 0
    with Image.open(path) as im:
        assert im.n_frames == 16 and im.size == (W, H) and im.info["duration"] == 50
        for t in (0, 8, 15):
            im.seek(t)
            assert np.array_equal(np.asarray(im.convert("RGB")), R.PALETTE[idx[t].cpu().numpy()]), t

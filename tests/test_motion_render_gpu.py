"""GPU: the motion preview (mdm_motion_render) against its restatement tests/render_ref.py.

* parity: t2m and KIT, B = 3, T = 5, lengths 5 / 2 / 1, 48 x 64 (not square, H no multiple of the tile), the default camera and
  one at elev 60, azim 135, dist 3, fov 60;
* T = 300 at 24 x 32 with frames= around the trajectory's chunk boundary; the 40 m clip (floor and trajectory behind the
  camera); two coincident joints; bones through the near plane (dist 0.5); colours and widths that are not the defaults;
* NaN past every length changes no bit and those frames are zero; each sample equals its own run at B = 1, T = n; palette mode
  is the index formula of the RGB output; frames= equals the same frames of a full render; contact_sheet equals tiling by hand;
* through a tiny trainer: generate_frames is render_motion of generate_joints, generate_gif writes m_len frames.

The gate.  Every pixel of every frame within ONE grey level of the fp64 restatement, none left out.  The bound is derived:
coverage and compositing are continuous (slope <= 1 per pixel of distance) in the projected coordinates, whose fp32 error is
about 1e-3 pixel or less, so the only difference is a rounding flip at floor(255 c + 0.5).  The share of pixels that differ at
all is printed next to the fp32 restatement's own share.  tests/test_motion_render_host.py shows that each likely mistake
moves >= 20 pixels by >= 64 levels.
"""
import numpy as np
import pytest
import torch

from conftest import pkg

import render_ref as RR
import test_motion_features_gpu as TF
import test_motion_fk_gpu as TK

pytestmark = pytest.mark.gpu

H, W = 48, 64
CAMERA2 = dict(elev=60.0, azim=135.0, dist=3.0, fov=60.0)
_MEMO = {}


def clips(name):
    """The parity batch of one skeleton: (skeleton, joints (3, 5, J, 3), lengths [5, 2, 1]); computed once, never written."""
    if name not in _MEMO:
        sk = TF.ref_skel(name)
        j, lens = RR.pad([RR.walk(sk, 5, 1), RR.walk(sk, 2, 2), RR.walk(sk, 1, 3)])
        _MEMO[name] = (sk, j, lens)
    return _MEMO[name]


def held(what, got, sk, joints, lens, size, camera=None, style=None, frames=None):
    """The gate: got (B, NF, H, W, 3) uint8 within one grey level of the fp64 restatement on every pixel."""
    w64 = RR.render(sk.chains, joints, lens, size[0], size[1], camera, style, np.float64, frames)
    w32 = RR.render(sk.chains, joints, lens, size[0], size[1], camera, style, np.float32, frames)
    assert got.shape == w64.shape and got.dtype == np.uint8, (what, got.shape, w64.shape)
    d = np.abs(got.astype(np.int32) - w64.astype(np.int32))
    own = np.abs(w32.astype(np.int32) - w64.astype(np.int32))
    print(f"{what}: worst {int(d.max())} level(s), {100 * (d > 0).any(-1).mean():.3f} % of pixels differ; the fp32 restatement: "
          f"worst {int(own.max())}, {100 * (own > 0).any(-1).mean():.3f} %")
    assert int(d.max()) <= 1, (what, int(d.max()), int((d > 1).sum()))
    drawn = (w64 != 255).any(-1).reshape(w64.shape[0], w64.shape[1], -1).sum(-1)
    return w64, drawn


def render(joints, lens=None, name=None, **kw):
    R = pkg("motion_render")
    return R.render_motion(torch.from_numpy(np.asarray(joints)).cuda(), lens, skeleton=name, **kw)


@pytest.mark.parametrize("camera", [None, CAMERA2], ids=["default", "elev60"])
@pytest.mark.parametrize("name", ["t2m", "kit"])
def test_parity(name, camera):
    sk, j, lens = clips(name)
    out = render(j, lens, size=(H, W), camera=camera)  # the skeleton by J
    assert out.shape == (3, 5, H, W, 3) and out.dtype == torch.uint8 and out.is_cuda
    got = out.cpu().numpy()
    w64, drawn = held(f"{name} {'default' if camera is None else 'elev 60'}", got, sk, j, lens, (H, W), camera)
    for b, n in enumerate(lens):
        assert not got[b, n:].any() and drawn[b, :n].min() > 30  # zeros past the length; a figure and a floor before
    if camera is None:  # a Camera is the dict
        R = pkg("motion_render")
        assert torch.equal(render(j, lens, name, size=(H, W), camera=R.Camera()), out)


def test_trajectory_chunks():
    """T = 300: the trajectory of frame 257 and later has more than 256 segments and goes through LDS in two chunks."""
    sk = TF.ref_skel("t2m")
    j = RR.walk(sk, 300, 5)[None]
    pick = [0, 1, 2, 255, 256, 257, 299]
    out = render(j, None, size=(24, 32), frames=pick)
    assert out.shape == (1, 7, 24, 32, 3)
    held("T 300", out.cpu().numpy(), sk, j, None, (24, 32), frames=pick)
    wide = dict(trajectory_width=60.0)  # a stroke a pixel wide: every chunk's segments show
    held("T 300 wide", render(j, None, size=(24, 32), frames=pick, **wide).cpu().numpy(), sk, j, None, (24, 32), style=wide, frames=pick)


def test_floor_and_trajectory_behind_the_camera():
    sk = TF.ref_skel("t2m")
    j = RR.far_clip(sk)[None]
    pick = [0, 1, 2, 7, 12, 18, 23]
    held("40 m", render(j, None, size=(H, W), frames=pick).cpu().numpy(), sk, j, None, (H, W), frames=pick)
    wide = dict(trajectory_width=30.0)
    held("40 m wide", render(j, None, size=(H, W), frames=pick, **wide).cpu().numpy(), sk, j, None, (H, W), style=wide, frames=pick)


def test_coincident_joints():
    sk = TF.ref_skel("t2m")
    j = RR.coincident_clip(sk)[None]
    out = render(j, None, size=(H, W), chain_width=30.0).cpu().numpy()
    held("coincident", out, sk, j, None, (H, W), style=dict(chain_width=30.0))


def test_bones_through_the_near_plane():
    """The camera half a metre from the spine: bones cross the near plane and are cut there."""
    sk = TF.ref_skel("t2m")
    j = RR.walk(sk, 3, 4)[None]
    for cam in (dict(dist=0.5, near=0.2), dict(dist=0.5, near=0.35, azim=80.0, elev=10.0)):
        eye, r, u, f = RR.camera_basis(cam, np.float64)
        p = j[0, 1].astype(np.float64) - [j[0, 1, 0, 0], j[0].reshape(-1, 3)[:, 1].min(), j[0, 1, 0, 2]]
        depth = (p - eye) @ f
        assert any((depth[a] < cam["near"]) != (depth[b] < cam["near"]) for c in sk.chains for a, b in zip(c[:-1], c[1:]))
        held(f"near plane {cam}", render(j, None, size=(H, W), camera=cam).cpu().numpy(), sk, j, None, (H, W), cam)


def test_colours_and_widths():
    sk, j, lens = clips("t2m")
    style = dict(background=(0.1, 0.2, 0.3), floor_color=(0.9, 0.8, 0.1), floor_alpha=0.8, trajectory_color=(0.0, 1.0, 0.0),
                 trajectory_alpha=0.6, trajectory_width=9.0, chain_colors=((1.0, 1.0, 0.0), (0.0, 1.0, 1.0), (1.0, 1.0, 1.0)),
                 chain_alpha=(1.0, 0.5, 0.75, 0.25, 1.0), chain_width=(2.0, 4.0, 8.0, 16.0, 32.0))
    got = render(j, lens, size=(H, W), **style).cpu().numpy()
    held("style", got, sk, j, lens, (H, W), style=style)
    assert not np.array_equal(got, render(j, lens, size=(H, W)).cpu().numpy())


def test_lengths_and_padding():
    """NaN in every frame past a length changes no bit; those frames are zero; a sample equals its own run at B = 1, T = n."""
    sk, j, lens = clips("t2m")
    for kw in (dict(), dict(palette=True), dict(camera=CAMERA2)):
        clean = render(j, lens, size=(H, W), **kw)
        bad = j.copy()
        for b, n in enumerate(lens):
            bad[b, n:] = np.nan
        out = render(bad, lens, size=(H, W), **kw)
        assert torch.equal(out, clean), kw
        for b, n in enumerate(lens):
            assert not out[b, n:].any()
            assert torch.equal(render(j[b:b + 1, :n], None, size=(H, W), **kw)[0], out[b, :n]), (kw, b)


def test_palette_mode_is_the_index_of_the_rgb_output():
    R = pkg("motion_render")
    sk, j, lens = clips("t2m")
    for kw in (dict(), dict(camera=CAMERA2, chain_colors=((0.3, 0.6, 0.9),), background=(0.2, 0.4, 0.5))):
        rgb, idx = render(j, lens, size=(H, W), **kw), render(j, lens, size=(H, W), palette=True, **kw)
        assert idx.shape == (3, 5, H, W) and idx.dtype == torch.uint8
        want = R.palette_index(rgb)
        for b, n in enumerate(lens):  # frames past the length are zero in both modes, not the index of black
            assert torch.equal(idx[b, :n], want[b, :n]) and not idx[b, n:].any()
        assert np.array_equal(want.cpu().numpy(), RR.palette_index(rgb.cpu().numpy()))
        assert len(torch.unique(idx)) > 3


def test_frames_subset_and_contact_sheet():
    R = pkg("motion_render")
    sk = TF.ref_skel("t2m")
    j, lens = RR.pad([RR.walk(sk, 11, 1), RR.walk(sk, 7, 2)])
    full = render(j, lens, size=(H, W))
    for frames, idx in ((slice(2, None, 3), [2, 5, 8]), (4, [0, 4, 8]), ([10, 0, 6, 6], [10, 0, 6, 6])):
        sub = render(j, lens, size=(H, W), frames=frames)
        assert torch.equal(sub, full[:, idx]), frames
    assert not full[1, 7:].any() and not render(j, lens, size=(H, W), frames=[6, 7])[1, 1].any()
    # a sheet of every 3rd frame, 3 to a row: frames 0 3 6 / 9 and two white cells
    sheet = R.contact_sheet(full, cols=3, every=3)
    assert sheet.shape == (2, 2 * H, 3 * W, 3)
    hand = torch.full((2, 2 * H, 3 * W, 3), 255, dtype=torch.uint8, device="cuda")
    for k, t in enumerate([0, 3, 6, 9]):
        hand[:, (k // 3) * H:(k // 3 + 1) * H, (k % 3) * W:(k % 3 + 1) * W] = full[:, t]
    assert torch.equal(sheet, hand)
    assert torch.equal(R.contact_sheet(torch.from_numpy(j).cuda(), cols=3, every=3, lengths=lens, size=(H, W)), hand)
    pal = render(j, lens, size=(H, W), palette=True)
    row = R.contact_sheet(pal, every=5)  # all in one row
    assert row.shape == (2, H, 3 * W) and torch.equal(row, torch.cat([pal[:, 0], pal[:, 5], pal[:, 10]], dim=2))
    assert int(R.contact_sheet(pal, cols=2, every=5)[0, H:, W:].min()) == 251  # the white cell, as an index


def _trainer():
    if "trainer" not in _MEMO:
        _MEMO["trainer"] = TF._tiny_trainer()
    return _MEMO["trainer"]


def test_generate_frames_is_render_of_generate_joints():
    R = pkg("motion_render")
    tr = _trainer()
    mean, std = TK._mean_std(263, 22, 12)
    caps, lens = ["a", "b", "c", "d"], torch.tensor([16, 16, 12, 9])
    opts = dict(seed=0, sampler="ddim", sample_steps=5, batch_size=2)  # batches of 16 and 12 frames: the denoiser takes even T
    for kw in (dict(), dict(from_rotations=True, fix_feet=True)):
        joints = tr.generate_joints(caps, lens, 263, mean, std, **opts, **kw)
        frames = tr.generate_frames(caps, lens, 263, mean, std, size=(H, W), **opts, **kw)
        assert [tuple(f.shape) for f in frames] == [(n, H, W, 3) for n in lens.tolist()]
        for f, jn in zip(frames, joints):
            assert torch.equal(f, R.render_motion(jn[None], size=(H, W))[0])
    styled = tr.generate_frames(caps, lens, 263, mean, std, size=(24, 32), camera=CAMERA2, palette=True,
                                style=dict(chain_width=8.0), **opts)
    for f, jn in zip(styled, tr.generate_joints(caps, lens, 263, mean, std, **opts)):
        assert torch.equal(f, R.render_motion(jn[None], size=(24, 32), camera=CAMERA2, palette=True, chain_width=8.0)[0])


def test_generate_gif_writes_every_frame(tmp_path):
    """The tiny model's motions are not a person's: their joints spread over some 2000 m (its weights are random), so the camera
    stands 8 km away, where every frame shows the whole tangle and differs from the one before.  (PIL stores a frame that
    repeats the one before as a longer delay of that one, so a clip of identical frames would come back shorter.)"""
    Image = pytest.importorskip("PIL.Image")
    R = pkg("motion_render")
    tr = _trainer()
    mean, std = TK._mean_std(263, 22, 12)
    caps, lens = ["a", "b"], [16, 9]
    opts = dict(seed=0, sampler="ddim", sample_steps=5, size=(H, W), camera=dict(dist=8000.0, target=(0.0, 0.0, 0.0)),
                style=dict(chain_width=24.0))
    paths = [str(tmp_path / "a.gif"), str(tmp_path / "b.gif")]
    assert tr.generate_gif(caps, torch.tensor(lens), 263, mean, std, paths=paths, **opts) == paths
    frames = tr.generate_frames(caps, torch.tensor(lens), 263, mean, std, palette=True, **opts)
    for path, n, idx in zip(paths, lens, frames):
        moved = [int((idx[t] != idx[t - 1]).sum()) for t in range(1, n)]
        print(f"{n} frames, pixels that differ from the frame before: {moved}")
        assert tuple(idx.shape) == (n, H, W) and min(moved) > 0  # the inputs: no two neighbouring frames alike
        with Image.open(path) as im:
            assert im.n_frames == n and im.size == (W, H) and im.info["duration"] == 50  # 20 fps
            for t in (0, n // 2, n - 1):
                im.seek(t)
                assert np.array_equal(np.asarray(im.convert("RGB")), R.PALETTE[idx[t].cpu().numpy()]), t
    data = tr.generate_gif(caps, torch.tensor(lens), 263, mean, std, **opts)
    assert [d == open(p, "rb").read() for d, p in zip(data, paths)] == [True, True]
    long = tr.generate_long_gif([[("a", 16), ("b", 16)]], 263, mean, std, overlap=4, seed=4, sampler="ddim", sample_steps=5,
                                size=(24, 32), fps=12.5, paths=[str(tmp_path / "long.gif")], camera=opts["camera"], style=opts["style"])
    with Image.open(long[0]) as im:
        assert im.n_frames == 28 and im.info["duration"] == 80
    with pytest.raises(ValueError, match="paths"):
        tr.generate_gif(caps, torch.tensor(lens), 263, mean, std, paths=paths[:1], **opts)

"""CPU: the motion preview's definition, its restatement tests/render_ref.py, the palette, the GIF writer and
the C entry's argument checks.  No GPU.

* the restatement's own properties on a 48 x 64 image: a lone capsule's coverage sums to its analytic integral, and a group's
  maximum makes a polyline no darker at its joint than its segments are;
* each of eleven likely mistakes moves the image by >= 64 grey levels on >= 20 pixels, with the restatement alone: this is
  what lets the GPU test's gate of one grey level see them;
* PALETTE and the index formula over all 256^3 colours;
* write_gif read back with PIL: frame count, pixels, duration;
* mdm_motion_render returns MDM_ERR_ARG for every bad argument, on the loaded library and without a device.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import pkg

import motion_features_ref as MR
import render_ref as RR

H, W = 48, 64


def ref_skel(name):
    sk = pkg("motion_features").SKELETONS[name]
    return MR.skeleton_from_tables(sk.chains, sk.raw_offsets, sk.face, sk.feet, sk.legs)


def test_a_capsule_sums_to_its_area():
    """Sum over pixels of clamp(0.5 + w - d) against its integral over the plane, 2 L w + pi w^2 + pi / 12 (the capsule's
    area, and pi / 12 that the ramp adds around the two caps).  The sum is a midpoint rule with cell 1 on a function of
    slope <= 1 that is linear in d but for two kinks, d = w -+ 0.5; where the function is smooth the rule's error per cell is
    <= |f''| / 24 <= 1 / (24 (w - 0.5)) (the caps' curvature), and a cell that a kink crosses errs by <= 1 / 8; the kinks are
    curves of length <= P = 2 L + 2 pi (w + 0.5) each and a curve of length P meets <= sqrt(2) P + 4 cells.  That bounds the
    error without counting on any cancellation: under 10 % of the area at w = 6, far below a factor on w or L."""
    X, Y = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    for a, b, w in (((14.3, 12.1), (47.9, 33.6), 6.0), ((20.0, 24.0), (44.0, 24.0), 6.0), ((30.2, 9.7), (31.9, 37.0), 6.0)):
        L = float(np.hypot(b[0] - a[0], b[1] - a[1]))
        cov = RR.capsule(a, b, w, X, Y, np.float64)
        assert cov.min() == 0.0 and cov.max() == 1.0 and not cov[0].any() and not cov[-1].any() and not cov[:, 0].any() and not cov[:, -1].any()
        want = 2 * L * w + np.pi * w * w + np.pi / 12
        P = 2 * L + 2 * np.pi * (w + 0.5)
        bound = 2 * (np.sqrt(2) * P + 4) / 8 + (2 * L * (w + 0.5) + np.pi * (w + 0.5) ** 2) / (24 * (w - 0.5))
        print(f"capsule L {L:.1f} w {w}: sum {cov.sum():.3f} integral {want:.3f} bound {bound:.1f}")
        assert abs(cov.sum() - want) <= bound and bound < 0.1 * want
    disc = RR.capsule((31.3, 22.8), (31.3, 22.8), 5.0, X, Y, np.float64)  # no length: a disc, and no NaN
    assert np.isfinite(disc).all() and abs(disc.sum() - (np.pi * 25 + np.pi / 12)) <= 2 * (np.sqrt(2) * 2 * np.pi * 5.5 + 4) / 8 + 1


def test_a_polyline_is_no_darker_at_its_joint():
    """Three joints, black on white without a floor: the chain 0-1-2 is exactly the darker of its two segments drawn alone,
    pixel by pixel, so nowhere darker than a single stroke; compositing them one after the other would be."""
    clip = np.array([[[-0.5, 0.3, 0.0], [0.1, 1.1, 0.0], [0.6, 0.2, 0.3]]], np.float32)
    style = dict(floor_alpha=0.0, chain_colors=(RR.BLACK,), chain_width=60.0)  # half-width 2 pixels
    one = lambda chains: RR.render_clip(chains, clip, 1, H, W, style=style)[0]  # noqa: E731
    both, a, b = one([[0, 1, 2]]), one([[0, 1]]), one([[1, 2]])
    assert np.array_equal(both, np.minimum(a, b))
    assert (a == 0).any() and (b == 0).any() and (np.minimum(a, b) < 255).sum() > 100
    twice = one([[0, 1], [1, 2]])  # two groups: composited one over the other
    assert np.array_equal(twice, both) is False and (twice <= both).all() and (twice < both).any()


# mistake -> (clip, valid frames, frame drawn, camera, style): chosen here, on the CPU, so that each mistake shows
MISTAKES = {
    "height_kept": ("walk", 24, 12, None, None),
    "traj_absolute": ("far", 24, 23, None, None),
    "traj_at_1": ("walk", 24, 1, None, dict(trajectory_width=64.0)),  # one point under the pelvis: a wide stroke shows it
    "traj_through_t": ("far", 24, 23, None, dict(trajectory_width=16.0)),
    "floor_unclipped": ("far", 24, 12, None, None),
    "chains_reversed": ("walk", 24, 12, dict(azim=90.0), dict(chain_width=16.0)),
    "mirror_x": ("walk", 24, 12, None, None),
    "flip_y": ("walk", 24, 12, None, None),
    "integer_centres": ("walk", 24, 12, None, None),
    "width_pixels": ("walk", 24, 12, None, None),
    "padding_in_extent": ("walk", 16, 12, None, None),  # frames 16 .. 23 are padding (zeros)
}


def test_every_mistake_moves_the_image():
    sk = ref_skel("t2m")
    assert set(MISTAKES) == set(RR.WRONG)
    clips = {"walk": RR.walk(sk, 24), "far": RR.far_clip(sk)}
    span = clips["far"][:, 0].max(0) - clips["far"][:, 0].min(0)
    assert 39.9 < float(np.linalg.norm(span[[0, 2]])) < 40.1  # the 40 m clip
    for name, (clip, n, t, cam, style) in MISTAKES.items():
        j = clips[clip].copy()
        j[n:] = 0.0
        right = RR.render_clip(sk.chains, j, n, 96, 128, cam, style, frames=[t])[0]
        wrong = RR.render_clip(sk.chains, j, n, 96, 128, cam, style, frames=[t], wrong=name)[0]
        count = RR.moved(right, wrong, 64)
        print(f"{name}: {count} pixels move by >= 64 levels")
        assert count >= 20, (name, count)


def test_the_far_floor_passes_behind_the_camera():
    """The 40 m clip is what near-plane clipping is tested on: at its frame 12 floor corners lie on both sides of the plane."""
    sk = ref_skel("t2m")
    j = RR.far_clip(sk)
    eye, r, u, f = RR.camera_basis(None, np.float64)
    lo, hi, root = j.reshape(-1, 3).min(0), j.reshape(-1, 3).max(0), j[12, 0]
    depth = [float(f @ (np.array([x - root[0], 0.0, z - root[2]]) - eye)) for x in (lo[0], hi[0]) for z in (lo[2], hi[2])]
    assert min(depth) < 0.1 < max(depth)
    path = j[:12, 0][:, [0, 2]] - root[[0, 2]]
    assert min(float(f @ (np.array([x, 0.0, z]) - eye)) for x, z in path) < 0.1  # and so does the trajectory


def test_palette_and_index():
    R = pkg("motion_render")
    assert R.PALETTE.shape == (252, 3) and R.PALETTE.dtype == np.uint8
    assert len({tuple(c) for c in R.PALETTE.tolist()}) == 252
    assert tuple(R.PALETTE[0]) == (0, 0, 0) and tuple(R.PALETTE[251]) == (255, 255, 255)
    g, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    half = np.array([255 / 5 / 2, 255 / 6 / 2, 255 / 5 / 2])  # half a step of the cube per channel
    for r in range(256):
        rgb = np.stack([np.full_like(g, r), g, b], -1)
        idx = R.palette_index(rgb)
        assert idx.dtype == np.uint8 and int(idx.max()) < 252
        assert np.array_equal(idx, RR.palette_index(rgb))  # the formula as the issue states it
        err = np.abs(R.PALETTE[idx].astype(np.int32) - rgb)
        assert (err <= half).all(), (r, err.reshape(-1, 3).max(0))
    t = torch.randint(0, 256, (5, 7, 3), generator=torch.Generator().manual_seed(0), dtype=torch.uint8)
    assert np.array_equal(R.palette_index(t).numpy(), R.palette_index(t.numpy()))


def test_gif_round_trip(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    R = pkg("motion_render")
    sk = ref_skel("t2m")
    n = 5
    j, _ = RR.pad([RR.walk(sk, n)], 7)
    rgb = RR.render(sk.chains, j, [n], H, W)[0]
    idx = R.palette_index(rgb)
    assert idx.shape == (7, H, W) and not idx[n:].any()
    for fps, ms in ((20.0, 50), (12.5, 80)):
        path = str(tmp_path / f"clip_{ms}.gif")
        assert R.write_gif(idx, path, fps, lengths=n) == path
        with Image.open(path) as im:
            assert im.n_frames == n and im.size == (W, H)
            for t in range(n):
                im.seek(t)
                assert np.array_equal(np.asarray(im.convert("RGB")), R.PALETTE[idx[t]]), t
                assert im.info["duration"] == ms
    assert R.gif_duration_ms(20) == 50 and R.gif_duration_ms(12.5) == 80 and R.gif_duration_ms(30) == 30 and R.gif_duration_ms(1000) == 10
    data = R.gif_bytes(torch.from_numpy(idx), 20.0, n)
    assert data[:6] in (b"GIF89a", b"GIF87a") and data == open(str(tmp_path / "clip_50.gif"), "rb").read()
    paths = [str(tmp_path / "a.gif"), str(tmp_path / "b.gif")]
    assert R.write_gif(np.stack([idx, idx]), paths, 20.0, lengths=[n, 2]) == paths
    with Image.open(paths[1]) as im:
        assert im.n_frames == 2
    with pytest.raises(ValueError):
        R.write_gif(idx.astype(np.float32), path, 20.0)
    with pytest.raises(ValueError):
        R.write_gif(idx, path, 20.0, lengths=8)
    with pytest.raises(ValueError):
        R.write_gif(idx, path, 0.0)


def test_arguments_are_checked_without_a_device():
    R, L = pkg("motion_render"), pkg("_lib")
    j = torch.zeros(2, 4, 22, 3)
    for kw in (dict(size=(48, 62)), dict(size=(3, 64)), dict(lengths=[4, 5]), dict(lengths=[0, 4]), dict(lengths=[4]),
               dict(skeleton="kit"), dict(camera=dict(elev=89.9)), dict(camera=dict(near=5.0)), dict(camera=dict(dist=0.0)),
               dict(camera=dict(fov=180.0)), dict(camera="front"), dict(frames=[4]), dict(frames=[]), dict(frames=0),
               dict(colour=(1, 0, 0)), dict(background=(2.0, 0, 0)), dict(chain_width=(1.0, 2.0)), dict(chain_width=-1.0),
               dict(floor_alpha=1.5), dict(trajectory_width=float("nan"))):
        with pytest.raises(ValueError):
            R.render_motion(j, **kw)
    with pytest.raises(ValueError):
        R.render_motion(torch.zeros(2, 4, 20, 3))  # no skeleton of 20 joints
    with pytest.raises(L.MdmError):
        R.render_motion(j)  # a CPU tensor: no fallback
    assert R.frame_indices(slice(1, None, 2), 6) == [1, 3, 5] and R.frame_indices(4, 10) == [0, 4, 8] and R.frame_indices([-1, 0], 5) == [4, 0]
    cam = R.as_camera(dict(elev=60, azim=135, dist=3, fov=60))
    assert cam == R.Camera(60, 135, 3, 60) and list(R.Camera().block()) == pytest.approx([30, 0, 5, 40, 0, 0.9, 0, 0.1])
    st = list(R.style_block(5))
    assert len(st) == 3 + 5 * 7 and st[:8] == [1, 1, 1, 0.5, 0.5, 0.5, 0.5, 0] and st[8:13] == [0, 0, 1, 1, 1]
    assert [st[13 + 5 * c:16 + 5 * c] for c in range(5)] == [list(c) for c in (RR.RED, RR.BLUE, RR.BLACK, RR.RED, RR.BLUE)]
    assert {k: v for k, v in R.STYLE.items()} == {k: v for k, v in RR.STYLE.items()}  # the defaults, stated twice


def test_entry_refuses_bad_arguments_before_the_device():
    """mdm_motion_render returns MDM_ERR_ARG for each bad argument without touching a device (B = 0 where it is well formed)."""
    L, MF, R = pkg("_lib"), pkg("motion_features"), pkg("motion_render")
    if not os.path.exists(L.LIB_PATH):
        pkg("build").build(verbose=False)
    lib = L.lib()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    skel = MF._skeleton_struct(MF.SKELETONS["t2m"])
    cam0 = [30.0, 0.0, 5.0, 40.0, 0.0, 0.9, 0.0, 0.1]

    def call(joints=p, skeleton=skel, B=0, T=4, J=22, H=48, W=64, camera=None, style=None, mode=0, frames=None, n_frames=0,
             out=p, scratch=p, no_camera=False, no_style=False, **cam):
        c = list(cam0)
        for k, v in cam.items():
            c[("elev", "azim", "dist", "fov", "tx", "ty", "tz", "near").index(k)] = v
        c = None if no_camera else (C.c_float * 8)(*c)
        s = None if no_style else (R.style_block(5) if style is None else (C.c_float * len(style))(*style))
        return lib.mdm_motion_render(joints, None, C.byref(skeleton) if skeleton is not None else None, B, T, J, H, W, c, s, mode,
                                     frames, n_frames, out, scratch, None)

    assert call() == 0 and call(mode=1) == 0 and call(H=4, W=4) == 0 and call(elev=-89.0) == 0 and call(frames=p, n_frames=3) == 0
    for kw in (dict(joints=None), dict(skeleton=None), dict(no_camera=True), dict(no_style=True), dict(out=None), dict(scratch=None),
               dict(W=62), dict(W=2), dict(H=3), dict(W=0), dict(J=21), dict(J=23), dict(elev=89.9), dict(elev=-90.0),
               dict(near=5.0), dict(near=6.0), dict(near=0.0), dict(dist=0.0), dict(fov=0.0), dict(fov=180.0),
               dict(elev=float("nan")), dict(tx=float("inf")), dict(mode=2), dict(mode=-1), dict(B=-1), dict(T=0),
               dict(frames=p, n_frames=0), dict(out=p + 2)):
        assert call(**kw) == 1, kw
    bad = list(R.style_block(5))
    bad[12] = -1.0  # the trajectory's width
    assert call(style=bad) == 1
    bad[12] = float("nan")
    assert call(style=bad) == 1
    odd = MF._skeleton_struct(MF.SKELETONS["t2m"])
    odd.chain_joints[1] = 99  # a joint outside the skeleton
    assert call(skeleton=odd) == 1
    assert call(skeleton=MF._skeleton_struct(MF.SKELETONS["kit"]), J=21) == 0
    assert call(B=70000) == 3 and call(frames=p, n_frames=70000) == 3  # MDM_ERR_UNSUPPORTED, before any launch
    assert lib.mdm_motion_render_scratch_floats(3, 5) == 3 * 18 and lib.mdm_motion_render_scratch_floats(1, 0) == -1

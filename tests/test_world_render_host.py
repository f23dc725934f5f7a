"""CPU: the world view's definition, its restatement tests/world_render_ref.py, the host side of
``motion_render.render_world`` and the C entries' argument checks.  No GPU.

* mdm_world_extent / mdm_world_render return MDM_ERR_ARG for each bad argument on the loaded library, without a device;
* pack_world, the ground rule, fit_camera (every corner of three extents projects inside the image), the limits (a fifth
  character, 17 primitives, 25 tracks) and the unknown-style error;
* each of eleven likely mistakes moves the 48 x 64 image by >= 64 grey levels on >= 20 pixels, with the restatement alone:
  this is what lets the GPU test's gate of one grey level see them.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import pkg

import render_ref as RR
import world_render_ref as WR

H, W = 48, 64


def test_entries_refuse_bad_arguments_before_the_device():
    L, MF, R = pkg("_lib"), pkg("motion_features"), pkg("motion_render")
    if not os.path.exists(L.LIB_PATH):
        pkg("build").build(verbose=False)
    lib = L.lib()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    skel = MF._skeleton_struct(MF.SKELETONS["t2m"])
    cam0 = [30.0, 0.0, 5.0, 40.0, 0.0, 0.9, 0.0, 0.1]

    def call(joints=p, skeleton=skel, scene=None, K=0, tracks=None, Km=0, B=0, Cn=2, T=4, J=22, H=48, W=64, style=None, ground=p,
             mode=0, frames=None, n_frames=0, out=p, scratch=p, no_camera=False, no_style=False, **cam):
        c = list(cam0)
        for k, v in cam.items():
            c[("elev", "azim", "dist", "fov", "tx", "ty", "tz", "near").index(k)] = v
        c = None if no_camera else (C.c_float * 8)(*c)
        s = None if no_style else (R.world_style_block(Cn if 1 <= Cn <= 4 else 1, 5) if style is None else (C.c_float * len(style))(*style))
        return lib.mdm_world_render(joints, None, C.byref(skeleton) if skeleton is not None else None, scene, K, tracks, Km, B, Cn,
                                    T, J, H, W, c, s, ground, mode, frames, n_frames, out, scratch, None)

    assert call() == 0 and call(mode=1) == 0 and call(H=4, W=4) == 0 and call(Cn=1) == 0 and call(Cn=4) == 0
    assert call(scene=p, K=16, tracks=p, Km=24) == 0 and call(frames=p, n_frames=3) == 0
    for kw in (dict(joints=None), dict(skeleton=None), dict(no_camera=True), dict(no_style=True), dict(ground=None), dict(out=None),
               dict(scratch=None), dict(Cn=0), dict(Cn=5), dict(K=-1), dict(scene=p, K=17), dict(K=1), dict(Km=-1),
               dict(tracks=p, Km=25), dict(Km=1), dict(W=62), dict(W=2), dict(H=3), dict(J=21), dict(elev=89.9), dict(near=5.0),
               dict(dist=0.0), dict(fov=180.0), dict(elev=float("nan")), dict(mode=2), dict(B=-1), dict(T=0),
               dict(frames=p, n_frames=0), dict(out=p + 2)):
        assert call(**kw) == 1, kw
    n = len(R.world_style_block(2, 5))
    assert n == 18 + 5 * 2 * 6
    for at, v in ((14, -1.0), (n - 1, -1.0), (22, -1.0), (16, float("nan")), (n - 2, float("inf"))):  # widths, a shade, an alpha
        bad = list(R.world_style_block(2, 5))
        bad[at] = v
        assert call(style=bad) == 1, (at, v)
    assert call(B=70000) == 3 and call(frames=p, n_frames=70000) == 3  # MDM_ERR_UNSUPPORTED, before any launch

    def extent(joints=p, scene=None, K=0, tracks=None, Km=0, B=0, Cn=2, T=4, J=22, out=p):
        return lib.mdm_world_extent(joints, None, scene, K, tracks, Km, B, Cn, T, J, out, None)

    assert extent() == 0 and extent(scene=p, K=16, tracks=p, Km=24) == 0 and extent(B=70000) == 3
    for kw in (dict(joints=None), dict(out=None), dict(Cn=0), dict(Cn=5), dict(K=17, scene=p), dict(K=2), dict(Km=25, tracks=p),
               dict(Km=3), dict(B=-1), dict(T=0), dict(J=0), dict(J=33)):
        assert extent(**kw) == 1, kw
    floats = lib.mdm_world_render_scratch_floats
    assert floats(2, 2, 5, 3, 0, 0) == 2 * (8 + 2 * 2 * 5 + 3 * (32 + 16 * 320)) and floats(1, 5, 5, 3, 0, 0) == -1
    assert floats(1, 1, 0, 1, 0, 0) == -1 and floats(1, 1, 1, 1, 17, 0) == -1 and floats(1, 1, 1, 1, 0, 25) == -1


def test_pack_world_and_limits():
    R, MS = pkg("motion_render"), pkg("motion_scene")
    a, b, c = torch.randn(5, 22, 3), torch.randn(3, 22, 3), torch.randn(2, 22, 3)
    x, ln = R.pack_world([[a, b], [c]])
    assert tuple(x.shape) == (2, 2, 5, 22, 3) and ln.tolist() == [[5, 3], [2, 0]] and x.dtype == torch.float32
    assert torch.equal(x[0, 1, :3], b) and not x[0, 1, 3:].any() and torch.equal(x[1, 0, :2], c) and not x[1, 1].any()
    y, ly = R.pack_world(x, [[5, 3], [2, 0]])
    assert torch.equal(y, x) and torch.equal(ly, ln) and R.pack_world(x)[1].tolist() == [[5, 5], [5, 5]]
    with pytest.raises(ValueError, match="at most 4"):
        R.pack_world([[a] * 5])
    with pytest.raises(ValueError, match="1 to 4"):
        R.pack_world(torch.zeros(1, 5, 4, 22, 3))
    with pytest.raises(ValueError, match=r"in \[0, 5\]"):
        R.pack_world(x, [[6, 3], [2, 0]])
    with pytest.raises(ValueError, match="one J"):
        R.pack_world([[a, torch.zeros(3, 21, 3)]])
    # the limits are motion_scene's: render_world checks the world before it needs a device
    with pytest.raises(ValueError, match="at most 16"):
        R.render_world(x, ln, scene=[MS.sphere((0, 0, 0), 1.0)] * 17)
    with pytest.raises(ValueError, match="at most 24"):
        R.render_world(x, ln, tracks=[MS.moving_sphere(np.zeros((5, 3)), 1.0)] * 25)
    with pytest.raises(ValueError, match="at most 4"):
        R.render_world([[a] * 5])
    with pytest.raises(ValueError, match="unknown style arguments.*chain_colors"):
        R.world_style_block(2, 5, chain_colors=((1, 0, 0),))
    with pytest.raises(ValueError, match="chain_alpha"):
        R.world_style_block(2, 5, chain_alpha=(1.0, 0.5, 0.2))
    assert len(R.world_style_block(4, 5, chain_alpha=[[1.0] * 5, [0.0] * 5, [0.5] * 5, [1.0] * 5], trajectory_alpha=[1, 0, 1, 0])) == 18 + 120
    assert set(R.WORLD_STYLE) >= {"solid_color", "solid_alpha", "edge_color", "edge_width", "shade", "character_colors"}
    assert R.WORLD_STYLE["character_colors"][0] == R.STYLE["chain_colors"] and len(R.WORLD_STYLE["character_colors"]) == 4


def test_ground_rule():
    R, MS = pkg("motion_render"), pkg("motion_scene")
    wall, tilted = MS.half_space((0, 0, 1), -2.0), MS.half_space((0, 1, 1e-3), 0.3)
    rec = MS.batch_scene([[wall, MS.floor(0.25), MS.floor(0.5)], [tilted, MS.half_space((0, 1, 0), 0.7, inside=True)], []], 3)
    ground, out = R.world_ground(rec)
    assert ground.tolist() == [0.25, 0.0, 0.0]  # the first floor(); a tilted or a keep-in one is not the ground
    assert not out[0, 1].any() and torch.equal(out[0, [0, 2]], rec[0, [0, 2]]) and torch.equal(out[1:], rec[1:])
    assert rec[0, 1, 0] == 4  # the caller's records are not written
    g, pr = WR.ground_of(rec[0].numpy())
    assert g == 0.25 and np.array_equal(pr, out[0].numpy())


def test_fit_camera_shows_the_whole_extent():
    R = pkg("motion_render")
    for ext, kw in (((-1.0, 0.0, -1.0, 1.0, 1.8, 1.0), dict()), ((-6.0, -0.5, 2.0, 9.0, 2.0, 3.0), dict(elev=60.0, azim=135.0, fov=60.0)),
                    ((0.1, 0.0, -20.0, 0.4, 0.3, 25.0), dict(elev=-20.0, azim=-70.0, size=(64, 48)))):
        size = kw.get("size", (H, W))
        cam = R.fit_camera(torch.tensor([ext]), **dict(kw, size=size))
        cam.block()
        assert np.allclose(cam.target, [(ext[i] + ext[i + 3]) / 2 for i in range(3)])
        eye, r, u, f = RR.camera_basis(WR.camera_dict(cam), np.float64)
        F = size[0] / 2 / np.tan(np.deg2rad(cam.fov) / 2)
        for x in ext[0::3]:
            for y in ext[1::3]:
                for z in ext[2::3]:
                    d = np.array([x, y, z]) - eye
                    px, py = size[1] / 2 + F * (r @ d) / (f @ d), size[0] / 2 - F * (u @ d) / (f @ d)
                    assert f @ d > cam.near and 0 <= px <= size[1] and 0 <= py <= size[0], (ext, px, py)
    both = R.fit_camera(np.array([[-1.0, 0, -1, 1, 2, 1], [3.0, 0, 3, 4, 1, 4], [np.inf, np.inf, np.inf, -np.inf, -np.inf, -np.inf]]))
    assert np.allclose(both.target, (1.5, 1.0, 1.5))  # the union of the finite rows
    assert R.fit_camera(np.full((1, 6), np.inf)) == R.Camera()


def _mistake_worlds():
    """name -> (joints (C, T, J, 3), lens, prims, tracks, camera, style): chosen here, on the CPU, so that each mistake shows."""
    MS = pkg("motion_scene")
    sk = WR.skel("t2m")
    _, j, lens, prims = WR.static_world("t2m")
    near = dict(elev=25.0, azim=20.0, dist=4.5, fov=45.0, target=(0.2, 0.6, 0.0))
    front = dict(elev=5.0, azim=0.0, dist=5.0, fov=40.0, target=(0.0, 0.7, 0.0))
    none = np.zeros((5, 0, 12), np.float32)
    static = (j[0], lens[0], prims[0], none, near, None)
    oj, ol, op = WR.order_world(sk)
    order = (oj[0], ol[0], op[0], none, front, dict(chain_width=24.0))
    tj, tl, tt = WR.track_world(sk)
    tracks = (tj[0], tl[0], np.zeros((0, 12), np.float32), tt[0], near, None)
    sunk = MS.pack_scene([MS.floor(0.0), MS.sphere((0.8, -0.6, 0.0), 0.5)]).numpy()
    # the box from nearby, its faces in colours far apart; a second character whose frames go on past its length
    at_box = dict(elev=35.0, azim=30.0, dist=3.0, fov=45.0, target=(0.3, 0.45, -1.2))
    boxy = (j[0], lens[0], prims[0], none, at_box, dict(solid_color=(0.1, 0.2, 0.9), solid_alpha=1.0, shade=(1.0, 0.5, 0.2)))
    full, _ = WR.world([[WR.placed(sk, 5, 1, -0.4, 0.8), WR.placed(sk, 5, 2, 0.7, -0.3)]])
    longer = (full[0], [5, 3], prims[0], none, near, dict(chain_width=16.0))
    return sk, {"index_order": (order, 1), "near_to_far": (order, 3), "yaw_sign": (boxy, 2), "six_faces": (boxy, 2),
                "track_frame0": (tracks, 4), "inactive_drawn": (tracks, 3), "past_length": (longer, 4), "sphere_flat": (static, 2),
                "ground_lowest": ((j[0], lens[0], sunk, none, near, None), 2), "root_relative": (static, 2),
                "halfspace_tangent": (static, 2)}


def test_every_mistake_moves_the_image():
    sk, worlds = _mistake_worlds()
    assert set(worlds) == set(WR.WRONG)
    for name, ((j, lens, prims, tracks, cam, style), t) in worlds.items():
        ground, pr = WR.ground_of(prims)
        right = WR.render_one(sk.chains, j, lens, pr, tracks, H, W, cam, style, ground, frames=[t])[0]
        wrong = WR.render_one(sk.chains, j, lens, pr, tracks, H, W, cam, style, ground, frames=[t], wrong=name)[0]
        count = RR.moved(right, wrong, 64)
        print(f"{name}: {count} pixels move by >= 64 levels")
        assert count >= 20, (name, count)

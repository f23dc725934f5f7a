"""GPU: the body view of the motion preview (mdm_mesh_render) against its restatement (tests/mesh_render_ref.py).

Images are 48 x 64 (24 x 32 where said), B = 3, T = 5, lengths 5 / 2 / 1.  Mesh c (the capsule bodies) is skinned on the device
by ``skin_vertices``, and the restatement runs on those vertices.

Parity gate: every DECISIVE pixel (see tests/mesh_render_ref.py: at least DELTA_E from the winner's edges, every other
candidate's depth key below by DELTA_D, |n.e| >= DELTA_N) within ONE grey level of the fp64 image, none left out; every
non-decisive pixel within one level of the colour of one of its candidates, or of no body; the non-decisive pixels at most
5 % of the covered ones in every image.  Printed: how many pixels differ at all, and the fp32 restatement's count beside it.
Everything else is bit for bit, except ``body_alpha = 0`` against ``render_motion`` (one level: two kernels' floors).
"""
import functools
import io
import os

import numpy as np
import pytest
import torch

from conftest import pkg

import mesh_render_ref as R
import scratch_hygiene as SH

pytestmark = pytest.mark.gpu


def device_skin(mesh, skel, P, Rm, lengths):
    v, n = pkg("motion_mesh").skin_vertices(mesh, torch.from_numpy(P).cuda(), torch.from_numpy(Rm).cuda(), lengths, return_normals=True)
    return v.cpu().numpy(), n.cpu().numpy()


@functools.lru_cache(maxsize=None)
def all_cases():
    return R.cases(device_skin)


@functools.lru_cache(maxsize=None)
def truth(name):
    return R.run(all_cases()[name], detail=True)


def cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def draw(case, **kw):
    """``render_mesh`` of a case; keyword arguments replace the case's."""
    a = dict(vertices=cuda(case.vertices), faces=torch.from_numpy(case.faces), lengths=case.lengths, root=cuda(case.root),
             normals=cuda(case.normals), size=case.size, camera=case.camera)
    a.update(case.style or {})
    a.update(kw)
    return pkg("motion_render").render_mesh(a.pop("vertices"), a.pop("faces"), a.pop("lengths"), **a)


@functools.lru_cache(maxsize=None)
def drawn(name):
    """The device's image of a case, shared and read-only."""
    return draw(all_cases()[name])


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_parity(name):
    case = all_cases()[name]
    im, det = truth(name)
    dec, cov = R.masks(det, im.shape[:4])
    for b in range(len(im)):
        for k in range(im.shape[1]):
            if det[b][k] is not None:                                               # the condition, on the device's own vertices
                assert (~dec[b, k]).sum() <= 0.05 * cov[b, k].sum(), (name, b, k)
    got = drawn(name).cpu().numpy()
    assert got.shape == im.shape and got.dtype == np.uint8
    for b, n in enumerate(case.lengths):
        assert not got[b, n:].any()                                                 # frames past a length are zero
    bad_dec, bad_nd, differ = R.check_against(got, im, det)
    _, _, differ32 = R.check_against(R.run(case, ft=np.float32), im, det)
    print(name, f"covered {int(cov.sum())}, non-decisive {int((~dec).sum())}: decisive pixels off by more than one level {bad_dec}, "
                f"non-decisive pixels unexplained {bad_nd}; pixels that differ at all {differ} (the fp32 restatement: {differ32})")
    assert bad_dec == 0 and bad_nd == 0


def test_crossing_boxes_show_both_orders():
    """Inside both boxes' silhouettes the thin box is in front in one place and the fat one in another: at the centre of each
    such part the device shows that box's own shade, which no painter's order of the two gives."""
    both, thin, fat = R.crossing_boxes()
    (ti, td), (ai, ad), (bi, bd) = (R.run(c, detail=True) for c in (both, thin, fat))
    masks = [R.masks(d, ti.shape[:4]) for d in (td, ad, bd)]
    overlap = masks[1][1] & masks[2][1] & masks[0][0] & masks[1][0] & masks[2][0]   # covered by each alone; decisive in all
    apart = np.abs(ai.astype(np.int32) - bi.astype(np.int32)).max(-1) > 8
    got = drawn("crossing_boxes").cpu().numpy().astype(np.int32)
    for b, k in ((0, 0), (0, 4), (1, 1), (2, 0)):
        for alone, who in ((ai, "thin"), (bi, "fat")):
            part = overlap[b, k] & apart[b, k] & (np.abs(ti[b, k].astype(np.int32) - alone[b, k]).max(-1) == 0)
            ys, xs = np.nonzero(part)
            assert len(ys) >= 5, (who, b, k, len(ys))
            i = np.argmin((ys - ys.mean()) ** 2 + (xs - xs.mean()) ** 2)               # the part's centre
            assert np.abs(got[b, k, ys[i], xs[i]] - alone[b, k, ys[i], xs[i]]).max() <= 1, (who, b, k)
            assert np.abs(got[b, k][part] - alone[b, k][part].astype(np.int32)).max() <= 1


def test_near_plane_and_degenerate_faces():
    """e: the face through the near plane is dropped, its neighbours are drawn.  f: zero-area faces and indices outside
    [0, V) draw nothing: the picture is the octahedron's."""
    case = all_cases()["near_plane"]
    got = drawn("near_plane")
    assert torch.equal(got, draw(case, faces=torch.from_numpy(case.faces[:3])))       # without the dropped face: the same picture
    assert int((got[0, 0] != draw(case, body_alpha=0.0)[0, 0]).any(-1).sum()) > 50      # and the neighbours are there
    assert torch.equal(drawn("degenerate"), drawn("octahedron_flat"))


def test_a_vertex_that_is_not_finite_inside_the_length():
    """NaN and +inf vertices in valid frames: their faces are dropped and they are no part of MINS / MAXS (bit for bit the
    octahedron's picture; an extent that took the +inf in would move the floor and the body)."""
    assert torch.equal(draw(R.nonfinite_case()), drawn("octahedron_flat"))


@pytest.mark.parametrize("shape", ["octahedron", "sphere"])
def test_watertight_on_the_device(shape):
    """Closed convex meshes: every pixel whose centre lies more than 0.5 pixel inside the silhouette shows the body, i.e. differs
    from the ``body_alpha = 0`` picture.  A crack at a shared edge (a fused multiply-add in one face's edge function, an edge
    evaluated in two orders) would show the floor or the background there; the parity gate would let it pass as non-decisive."""
    import test_mesh_render_host as TH
    v, f = {"octahedron": R.octahedron, "sphere": TH.sphere}[shape]()
    vv, root, _ = R._moving(v, B=2, T=4)
    H, W = 48, 64
    red = dict(body_color=(1.0, 0.0, 0.0))                       # no floor, trajectory or background pixel is red
    for cam in (None, R.CAMERA2):
        case = R._case(vv, f, root, camera=cam, lengths=[4, 4], style=red)
        shows = (draw(case) != draw(case, body_alpha=0.0)).any(-1).cpu().numpy()
        c = dict(R.RR.CAMERA, **(cam or {}))
        eye, r, u, fwd = R.RR.camera_basis(c, np.float64)
        F = H / 2 / np.tan(np.deg2rad(c["fov"]) / 2)
        X, Y = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
        for b in range(2):
            lo = case.vertices[b].reshape(-1, 3).min(0).astype(np.float64)
            for t in range(4):
                p = case.vertices[b, t].astype(np.float64) - (case.root[b, t, 0], lo[1], case.root[b, t, 2]) - eye
                h = TH.hull(np.stack([W / 2 + F * (p @ r) / (p @ fwd), H / 2 - F * (p @ u) / (p @ fwd)], -1))
                inside = np.full((H, W), np.inf)
                for a, q in zip(h, np.roll(h, -1, 0)):
                    e = q - a
                    inside = np.minimum(inside, (e[0] * (Y - a[1]) - e[1] * (X - a[0])) / np.hypot(*e))
                deep = inside > 0.5
                assert deep.sum() > 30 and shows[b, t][deep].all(), (shape, cam, b, t, int((deep & ~shows[b, t]).sum()))


def test_lengths_batches_and_reruns():
    for name in ("body_t2m_high_smooth", "octahedron_flat"):
        case = all_cases()[name]
        out = drawn(name)
        v, nr, root = case.vertices.copy(), None if case.normals is None else case.normals.copy(), case.root.copy()
        for b, n in enumerate(case.lengths):
            v[b, n:], root[b, n:] = np.nan, np.nan
            if nr is not None:
                nr[b, n:] = np.nan
        assert torch.equal(draw(case, vertices=cuda(v), normals=cuda(nr), root=cuda(root)), out)   # nothing past a length is read
        assert torch.equal(draw(case), out)                                                      # two runs of the same call
        for b, n in enumerate(case.lengths):
            one = draw(case, vertices=cuda(case.vertices[b:b + 1, :n]), root=cuda(case.root[b:b + 1, :n]), lengths=None,
                       normals=None if nr is None else cuda(case.normals[b:b + 1, :n]))
            assert torch.equal(one[0], out[b, :n]), (name, b)                                    # a sample against its own run
        pal = draw(case, palette=True)
        assert pal.shape == out.shape[:4] and torch.equal(pal, pkg("motion_render").palette_index(out))
        for frames, idx in (([4, 0, 1], [4, 0, 1]), (2, [0, 2, 4]), (slice(1, 4), [1, 2, 3])):
            assert torch.equal(draw(case, frames=frames), out[:, idx]), frames
            assert torch.equal(draw(case, frames=frames, palette=True), pal[:, idx])
    one = all_cases()["octahedron_flat"]
    clip = draw(one, vertices=cuda(one.vertices[0]), root=cuda(one.root[0]), lengths=None)   # one clip without the batch dim
    assert torch.equal(clip[0], drawn("octahedron_flat")[0])


@pytest.mark.parametrize("smooth", [False, True], ids=["flat", "smooth"])
def test_face_chunks(smooth):
    """Undrawn faces (zero area, a vertex index past V) in front of, between and behind the faces change nothing, at face
    counts around the chunk of 256.  Mesh c has 1044 faces, more than a chunk, so the counts 255 / 256 / 257 / 3 x 256 + 1 are
    reached from its first five capsules (228 faces), and the whole body goes to 5 x 256 and 5 x 256 + 1."""
    case = all_cases()["body_t2m_high_smooth" if smooth else "body_t2m_high_flat"]
    V = case.vertices.shape[2]
    for faces, counts in ((case.faces[:228], (255, 256, 257, 3 * 256 + 1)), (case.faces, (5 * 256, 5 * 256 + 1))):
        want = draw(case, faces=torch.from_numpy(faces))
        assert int((want != draw(case, body_alpha=0.0)).any(-1).sum()) > 60   # the faces show: 8 frames of them
        for F in counts:
            extra = F - len(faces)
            junk = np.array([(0, 0, 0), (1, 2, V), (3, 3, 4)], np.int32)[np.arange(extra) % 3]
            cut = [0, extra // 3, 2 * extra // 3, extra]
            mixed = np.concatenate([junk[cut[0]:cut[1]], faces[:100], junk[cut[1]:cut[2]], faces[100:], junk[cut[2]:cut[3]]])
            assert len(mixed) == F and torch.equal(draw(case, faces=torch.from_numpy(mixed)), want), F


def test_long_clip_around_the_trajectory_chunk():
    """T = 300 at 24 x 32: frames either side of the 256 segments a trajectory chunk holds, against the restatement."""
    tri = np.array([[-0.5, -0.3, 0.0], [0.6, -0.2, 0.1], [0.0, 0.55, -0.1], [0.1, 0.1, 0.5]])
    faces = np.array([(0, 1, 2), (0, 1, 3), (1, 2, 3), (2, 0, 3)])
    t = np.arange(300)[:, None]
    root = np.concatenate([0.8 * np.sin(t / 40.0), 0.9 + 0 * t, 0.8 * np.cos(t / 25.0) - 0.8], 1)[None]
    case = R._case(tri[None, None] + root[:, :, None], faces, root, lengths=[300], size=(24, 32))
    frames = [2, 255, 256, 257, 258, 299]
    im, det = R.run(case, detail=True, frames=frames)
    got = draw(case, frames=frames).cpu().numpy()
    bad_dec, bad_nd, differ = R.check_against(got, im, det)
    print(f"T = 300: decisive off {bad_dec}, non-decisive unexplained {bad_nd}, pixels that differ at all {differ}")
    assert bad_dec == 0 and bad_nd == 0
    assert torch.equal(draw(case)[:, frames], torch.from_numpy(got).cuda())


def test_no_body_is_the_stick_figure_view_without_sticks():
    """``body_alpha = 0`` leaves §21's floor and trajectory: ``render_motion`` of a figure whose joints span the vertices'
    extent (joint 0 the root, joints 1 and 2 at MINS and MAXS, the rest on the root) with ``chain_alpha = 0``, to one level."""
    MRn = pkg("motion_render")
    for name in ("body_t2m_high_flat", "octahedron_flat"):
        case = all_cases()[name]
        B, T = case.vertices.shape[:2]
        joints = np.repeat(case.root[:, :, None], 22, 2).copy()
        for b, n in enumerate(case.lengths):
            lo, hi = case.vertices[b, :n].reshape(-1, 3).min(0), case.vertices[b, :n].reshape(-1, 3).max(0)
            assert (case.root[b, :n] >= lo).all() and (case.root[b, :n] <= hi).all()   # the root lies inside the body's extent
            joints[b, :, 1], joints[b, :, 2] = lo, hi
        sticks = MRn.render_motion(cuda(joints), case.lengths, size=case.size, camera=case.camera, chain_alpha=0.0)
        bare = draw(case, body_alpha=0.0)
        diff = (sticks.int() - bare.int()).abs()
        print(name, f"body_alpha = 0 against render_motion: {int((diff > 0).any(-1).sum())} pixels differ, at most {int(diff.max())} level")
        assert int(diff.max()) <= 1
        assert int((bare != drawn(name)).any(-1).sum()) > 100                          # and the body was there


def test_scratch_and_output_bounds():
    """The C entry in guarded windows: poisoned scratch changes nothing (all that is read was written by the call), and the
    guard words past ``mdm_mesh_render_scratch_floats`` and past the output are intact."""
    L, MRn = pkg("_lib"), pkg("motion_render")
    lib = L.lib()
    for name, frames in (("body_kit_default_smooth", None), ("body_kit_default_flat", [3, 1]), ("triangle", None)):
        case = all_cases()[name]
        v, root, f = cuda(case.vertices), cuda(case.root), cuda(case.faces)
        nr, ln = cuda(case.normals), torch.tensor(case.lengths, dtype=torch.int32).cuda()
        fr = None if frames is None else torch.tensor(frames, dtype=torch.int32).cuda()
        B, T, V = v.shape[:3]
        NF, (H, W) = (T if frames is None else len(frames)), case.size
        floats = int(lib.mdm_mesh_render_scratch_floats(B, T, NF, V, len(f), int(nr is not None)))
        cam, st = MRn.as_camera(case.camera).block(), MRn.mesh_style_block()
        outs = []
        for palette in (0, 1):
            for how in ("Z", "P"):
                scratch = SH.guarded(4 * floats)
                SH.fill_float_scratch(scratch.win, how)
                guard, out = SH.guarded_like((B, NF, H, W) + (() if palette else (3,)), torch.uint8, fill=7)
                status = lib.mdm_mesh_render(v.data_ptr(), L.ptr(nr), f.data_ptr(), root.data_ptr(), ln.data_ptr(), B, T, V, len(f), H, W,
                                             cam, st, palette | (2 if nr is not None else 0), L.ptr(fr), NF, out.data_ptr(),
                                             scratch.ptr(), L.stream_ptr())
                torch.cuda.synchronize()
                assert status == 0 and scratch.guards_untouched() and guard.guards_untouched(), (name, palette, how)
                outs.append(out.clone())
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[2], outs[3]), name
        want = drawn(name) if frames is None else drawn(name)[:, frames]
        assert torch.equal(outs[0], want) and torch.equal(outs[2], MRn.palette_index(want))
    assert lib.mdm_mesh_render(v.data_ptr(), None, f.data_ptr(), root.data_ptr(), None, 0, T, V, len(f), H, W, cam, st, 0, None, 0,
                               out.data_ptr(), scratch.ptr(), L.stream_ptr()) == 0      # B = 0: a no-op


def test_through_a_tiny_trainer(tmp_path):
    import test_motion_features_gpu as TF
    import test_motion_fk_gpu as TK
    from PIL import Image
    MRn, MO = pkg("motion_render"), pkg("motion_outputs")
    tr = TF._tiny_trainer()
    mean, std = TK._mean_std(263, 22, 12)
    caps, lens = ["a", "b", "c", "d"], [16, 16, 12, 9]
    opts = dict(seed=0, sampler="ddim", sample_steps=5, batch_size=2, fix_feet=True)
    meshes = tr.generate_mesh(caps, torch.tensor(lens), 263, mean, std, normals=True, **opts)
    rots = tr.generate_rotations(caps, torch.tensor(lens), 263, mean, std, **opts)
    extent = []                                                                          # of each sample as the view places it
    for (v, _, _), (j, _, _) in zip(meshes, rots):
        p = (v - j[:, :1] * torch.tensor([1.0, 0.0, 1.0], device=v.device)).reshape(-1, 3)
        p[:, 1] -= p[:, 1].min()
        extent.append(torch.cat([p.min(0).values, p.max(0).values]))
    view = dict(size=(48, 64), camera=MRn.fit_camera(torch.stack(extent), elev=20.0, azim=30.0, size=(48, 64)))
    frames = tr.generate_frames(caps, torch.tensor(lens), 263, mean, std, view="body", **view, **opts)
    for i, n in enumerate(lens):
        v, nr, faces = meshes[i]
        want = MRn.render_mesh(v, faces, root=rots[i][0], normals=nr, **view)             # the body in the .glb is the body drawn
        assert frames[i].shape == (n, 48, 64, 3) and torch.equal(frames[i], want[0]), i
        assert int((frames[i][0] != MRn.render_mesh(v, faces, root=rots[i][0], body_alpha=0.0, **view)[0, 0]).any(-1).sum()) > 30
    paths = [str(tmp_path / "a.gif"), None, None, None]
    gifs = tr.generate_gif(caps, torch.tensor(lens), 263, mean, std, view="body", paths=paths, **view, **opts)
    assert gifs[0] == paths[0] and os.path.exists(paths[0])
    pal = tr.generate_frames(caps, torch.tensor(lens), 263, mean, std, view="body", palette=True, **view, **opts)
    for i, n in enumerate(lens):
        assert torch.equal(pal[i], MRn.palette_index(frames[i]))
        im = Image.open(paths[0] if i == 0 else io.BytesIO(gifs[i]))
        kept = 1 + sum(int(not torch.equal(pal[i][t], pal[i][t - 1])) for t in range(1, n))   # PIL folds a repeated frame
        shown = 0
        for t in range(im.n_frames):
            im.seek(t)
            shown += im.info["duration"]
        assert im.n_frames == kept and shown == 50 * n and im.size == (64, 48), (i, im.n_frames, kept, shown)
    # the other views take the code they took
    root_view = tr.generate_frames(caps, torch.tensor(lens), 263, mean, std, size=(48, 64), **opts)
    joints = tr.generate_joints(caps, torch.tensor(lens), 263, mean, std, **opts)
    for got, want in zip(root_view, MO.to_frames(joints, (48, 64), None, False, None)):
        assert torch.equal(got, want)
    for bad in (dict(view="sky"), dict(view="root", mesh=object())):
        with pytest.raises(ValueError):
            tr.generate_frames(caps, torch.tensor(lens), 263, mean, std, **bad, **opts)
    scripts = [[("a", 16), ("b", 16)]]
    (gif,) = tr.generate_long_gif(scripts, 263, mean, std, view="body", size=(24, 32), overlap=4, seed=4, sampler="ddim", sample_steps=5)
    im, shown = Image.open(io.BytesIO(gif)), 0
    for t in range(im.n_frames):
        im.seek(t)
        shown += im.info["duration"]
    assert shown == 50 * 28 and im.size == (32, 24)
    mesh = pkg("motion_mesh").capsule_body(rots[0][2].cpu(), "t2m", segments=6, rings=2)   # a mesh of the caller's
    own = tr.generate_frames(caps[:2], torch.tensor(lens[:2]), 263, mean, std, view="body", mesh=mesh, **view, **opts)
    assert own[0].shape == frames[0].shape and not torch.equal(own[0], frames[0])

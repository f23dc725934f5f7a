"""GPU: linear blend skinning on the device (mdm_skin_vertices) and what is built on it.

* the kernel against the fp64 restatement (tests/mesh_ref.py) on the cases of tests/golden/motion_fk.npz through
  motion_to_joints_fk: both skeletons; 1, 255 and 257 vertices (one vertex tile is 256); frame counts below, at and above the
  frame tile of 16; shared and per-sample vertices and bind joints; Q null and given; 1 to 4 live influences, dead slots holding
  index 0 and J - 1; normals on and off;
* lengths: zeros past a length, nothing past it is read, every sample equals its run alone, T = 1;
* ties to the skeleton: a vertex at bind joint c on bone c lands on joint c, one on bone 0 at the root lands on the root, identity
  rotations with P = G give the rest vertices bit for bit;
* through the file: device quaternions -> glb_bytes -> the fp64 glTF evaluator against the device's vertices; after the
  foot-skate clean-up the ankles' vertices follow the pinned joints;
* through the trainer: generate_mesh, generate_glb, generate_long_mesh, generate_long_glb; argument errors.

Tolerances.  GATE = 4 x a yardstick, as tests/test_motion_rig_gpu.py has it: the yardstick of a launch is how far the all-fp32
restatement lies from what the launch is compared with (the fp64 restatement, or the joints themselves), on the same inputs and
over the whole batch, for vertices and normals separately.  Nothing is gated against the kernel's output.
tests/test_motion_mesh_host.py shows that each of seven mistakes lies >= 8e4 gates away.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, pkg

import mesh_ref as MR
import rig_ref as RR

pytestmark = pytest.mark.gpu

GATE = 4.0
FRAME_TILE, VERTEX_TILE = 16, 256  # of csrc/motion_skin.hip
SHAPES = [(5, [5, 2, 1]), (FRAME_TILE - 1, [5, 2, 1]), (FRAME_TILE, [5, 2, 1]), (FRAME_TILE + 1, [5, 2, 1]),
          (FRAME_TILE + 1, [FRAME_TILE + 1, FRAME_TILE, 1])]


def golden():
    return np.load(os.path.join(GOLDEN, "motion_fk.npz"))


def parents_of(skel):
    return list(pkg("motion_features").get_skeleton(skel).parents)


@functools.lru_cache(maxsize=None)
def fk(skel, T, lens):
    """The noisy golden case through motion_to_joints_fk on the shared offsets: (joints, rotations) on the device; read-only."""
    z = golden()
    rows = torch.from_numpy(np.ascontiguousarray(z[f"{skel}_noisy_rows"][:, :T])).cuda()
    return pkg("postprocess").motion_to_joints_fk(rows, z[f"{skel}_mean"], z[f"{skel}_std"], list(lens),
                                                  torch.from_numpy(z[f"{skel}_offsets"]), skeleton=skel, sigma=0.0,
                                                  return_rotations=True)


@functools.lru_cache(maxsize=None)
def random_mesh(skel, V, per_sample, with_q, seed=3):
    """A mesh by construction: vertices about the bind joints, 1 to 4 live influences per vertex in turn, the dead slots
    holding index 0 and J - 1 in turn, random unit normals; bind joints off our rest pose, per sample or shared."""
    MM = pkg("motion_mesh")
    rs = np.random.RandomState(seed + V)
    J = len(parents_of(skel))
    rest = MM.rest_pose(golden()[f"{skel}_offsets"], skel)
    G = np.stack([s * rest + 0.02 * rs.randn(J, 3) for s in (1.0, 1.1, 0.9)]) if per_sample else rest + 0.02 * rs.randn(J, 3)
    idx, w = rs.randint(0, J, (V, 4)), rs.uniform(0.1, 1.0, (V, 4))
    dead = np.arange(4)[None, :] > (np.arange(V) % 4)[:, None]
    w[dead] = 0.0
    idx[dead] = np.broadcast_to(np.where(np.arange(V) % 2 == 0, 0, J - 1)[:, None], (V, 4))[dead]
    v = G[..., idx[:, 0], :] + 0.1 * rs.randn(*G.shape[:-2], V, 3)
    n = rs.randn(*v.shape)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    Q = None
    if with_q:
        axis = rs.randn(J, 3)
        Q = RR.rodrigues(axis / np.linalg.norm(axis, axis=-1, keepdims=True), np.deg2rad(rs.uniform(5, 40, J)))
    faces = np.zeros((1, 3), int)
    mesh = MM.Mesh(v, faces, idx, w, G, Q, n, skel)
    if V >= 8:
        lost = mesh.bone_index[mesh.bone_weight == 0]
        assert (lost == 0).any() and (lost == J - 1).any() and sorted(set((mesh.bone_weight > 0).sum(1))) == [1, 2, 3, 4]
    return mesh


def restated(mesh, skel, j, r, lens, dtype):
    """The restatement over a batch: per sample (vertices, normals) of its first lens[b] frames."""
    P, R = j.cpu().numpy(), r.cpu().numpy()
    out = []
    for b, n in enumerate(lens):
        one = mesh.sample(b)
        out.append(MR.skin(parents_of(skel), P[b, :n], R[b, :n], one.vertices, one.normals, one.bind_joints, one.bind_rotations,
                           one.bone_index, one.bone_weight, dtype))
    return out


def worst(got, want, k):
    return max(float(np.abs(np.asarray(g[k], np.float64) - w[k]).max()) for g, w in zip(got, want))


@pytest.mark.parametrize("per_sample", [False, True], ids=["shared", "per_sample"])
@pytest.mark.parametrize("V", [1, VERTEX_TILE - 1, VERTEX_TILE + 1])
@pytest.mark.parametrize("skel", ["t2m", "kit"])
def test_kernel_against_the_restatement(skel, V, per_sample):
    MM = pkg("motion_mesh")
    for with_q in (False, True):
        mesh = random_mesh(skel, V, per_sample, with_q)
        for T, lens in SHAPES:
            j, r = fk(skel, T, tuple(lens))
            truth, fp32 = restated(mesh, skel, j, r, lens, np.float64), restated(mesh, skel, j, r, lens, np.float32)
            yv, yn = worst(fp32, truth, 0), worst(fp32, truth, 1)
            out, nout = MM.skin_vertices(mesh, j, r, lens, return_normals=True)
            plain = MM.skin_vertices(mesh, j, r, lens)
            assert out.shape == (3, T, V, 3) and nout.shape == (3, T, V, 3) and torch.equal(plain, out)  # normals on and off
            got = [(out[b, :n].cpu().numpy(), nout[b, :n].cpu().numpy()) for b, n in enumerate(lens)]
            ev, en = worst(got, truth, 0), worst(got, truth, 1)
            print(skel, V, "per-sample" if per_sample else "shared", "Q" if with_q else "-", T, lens,
                  f"vertices {ev:.3g} (yardstick {yv:.3g})  normals {en:.3g} (yardstick {yn:.3g})")
            assert ev <= GATE * yv and en <= GATE * yn, (with_q, T, lens, ev, yv, en, yn)
            for b, n in enumerate(lens):
                assert not out[b, n:].any() and not nout[b, n:].any()


def test_lengths():
    MM = pkg("motion_mesh")
    T, lens = FRAME_TILE + 1, [FRAME_TILE + 1, FRAME_TILE, 1]
    j, r = fk("t2m", T, tuple(lens))
    for per_sample in (False, True):
        mesh = random_mesh("t2m", VERTEX_TILE + 1, per_sample, True)
        out, nout = MM.skin_vertices(mesh, j, r, lens, return_normals=True)
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(nout).all())
        jn, rn = j.clone(), r.clone()
        for b, n in enumerate(lens):
            jn[b, n:], rn[b, n:] = float("nan"), float("nan")
        out2, nout2 = MM.skin_vertices(mesh, jn, rn, lens, return_normals=True)
        assert torch.equal(out2, out) and torch.equal(nout2, nout)                        # nothing past a length is read
        for b, n in enumerate(lens):
            assert not out[b, n:].any() and not nout[b, n:].any()                          # zeros past the length
            one, n1 = MM.skin_vertices(mesh.sample(b), j[b:b + 1, :n], r[b:b + 1, :n], None, return_normals=True)
            assert one.shape == (1, n, VERTEX_TILE + 1, 3)                                 # T = 1 among them
            assert torch.equal(one[0], out[b, :n]) and torch.equal(n1[0], nout[b, :n]), (per_sample, b)
    full = MM.skin_vertices(mesh, j, r)                                                   # no lengths: every frame counts
    assert torch.equal(full[0], out[0]) and full.shape == out.shape


@pytest.mark.parametrize("skel", ["t2m", "kit"])
def test_ties_to_the_skeleton(skel):
    """A vertex at bind joint c, bound wholly to bone c, is joint c; bound to bone 0 at the root it is the root.  Yardstick: the
    fp32 restatement of the same vertices against the joints."""
    MM = pkg("motion_mesh")
    lens = [5, 2, 1]
    j, r = fk(skel, 5, tuple(lens))
    off = golden()[f"{skel}_offsets"]
    rest = MM.rest_pose(off, skel).astype(np.float32)
    J = len(rest)
    idx, w = np.zeros((J, 4), int), np.zeros((J, 4))
    idx[:, 0], w[:, 0] = np.arange(J), 1.0
    mesh = MM.Mesh(rest, np.zeros((1, 3), int), idx, w, rest, None, None, skel)
    out = MM.skin_vertices(mesh, j, r, lens)
    want = [(j[b, :n].cpu().numpy().astype(np.float64),) for b, n in enumerate(lens)]
    yard = worst(restated(mesh, skel, j, r, lens, np.float32), want, 0)
    err = worst([(out[b, :n].cpu().numpy(),) for b, n in enumerate(lens)], want, 0)
    print(skel, f"vertices at the joints {err:.3g} (yardstick {yard:.3g})")
    assert err <= GATE * yard, (err, yard)
    assert torch.equal(out[:, :, 0], j[:, :, 0])                                         # the root, to the bit
    # identity rotations and P = G: the rest vertices bit for bit, whatever the weights
    for per_sample in (False, True):
        for with_q in (False, True):
            mesh = random_mesh(skel, VERTEX_TILE + 1, per_sample, False)
            if with_q:
                mesh = MM.Mesh(mesh.vertices, mesh.faces, mesh.bone_index, mesh.bone_weight, mesh.bind_joints,
                               np.tile(np.eye(3), (J, 1, 1)), mesh.normals, skel)
            G = torch.from_numpy(np.broadcast_to(mesh.bind_joints, (3, J, 3)).copy()).cuda()
            P = G[:, None].expand(3, FRAME_TILE + 1, J, 3).contiguous()
            R = torch.eye(3, device="cuda").expand(3, FRAME_TILE + 1, J, 3, 3).contiguous()
            still, nrm = MM.skin_vertices(mesh, P, R, None, return_normals=True)
            v = torch.from_numpy(np.broadcast_to(mesh.vertices, (3, VERTEX_TILE + 1, 3)).copy()).cuda()
            assert torch.equal(still, v[:, None].expand_as(still)), (per_sample, with_q)
            n = torch.from_numpy(np.broadcast_to(mesh.normals, (3, VERTEX_TILE + 1, 3)).copy()).cuda()
            # the normals: sum_k w_k n, four roundings of at most eps / 2 each and a weight sum within 2 eps of 1, then the
            # normalisation's own 3 eps: within 8 eps of the unit normal
            assert float((nrm - n[:, None]).abs().max()) <= 8 * np.finfo(np.float32).eps


def test_through_the_file():
    """Device quaternions -> glb_bytes -> the fp64 evaluator, against the device's vertices at the same frames.  Yardstick:
    the same chain in the fp32 restatements (rig keys -> file -> evaluator, against the fp32 skinning)."""
    MM, MRig = pkg("motion_mesh"), pkg("motion_rig")
    lens = [5, 2, 1]
    j, r = fk("t2m", 5, tuple(lens))
    off = golden()["t2m_offsets"]
    rig = MRig.rig_of("t2m")
    mesh = MM.capsule_body(off, "t2m")
    chan, lens_out, quat = MRig.rotations_to_rig(j, r, lens, return_quaternions=True)
    out = MM.skin_vertices(mesh, j, r, lens).cpu().numpy()
    fp32 = restated(mesh, "t2m", j, r, lens, np.float32)
    P, R = j.cpu().numpy(), r.cpu().numpy()
    err = yard = 0.0
    for b, n in enumerate(lens):
        assert int(lens_out[b]) == n
        glb = MR.read_glb(MM.glb_bytes(mesh, rig, off, chan[b, :, :3], quat[b], n, 0.05))
        c32, q32 = RR.rig_channels(rig, P[b, :n], R[b, :n], dtype=np.float32)
        ref = MR.read_glb(MM.glb_bytes(mesh, rig, off, c32[:, :3], q32, n, 0.05))
        for k in range(n):
            err = max(err, float(np.abs(MR.gltf_vertices(glb, k) - out[b, k]).max()))
            yard = max(yard, float(np.abs(MR.gltf_vertices(ref, k) - fp32[b][0][k]).max()))
    print(f"through the file {err:.3g} (yardstick {yard:.3g})")
    assert err <= GATE * yard, (err, yard)


def test_after_the_foot_skate_clean_up():
    """The vertices at the ankles and toes follow the pinned joints.  Yardstick: the fp32 restatement on the pinned joints and
    turned rotations, against those joints."""
    MM, P = pkg("motion_mesh"), pkg("postprocess")
    z = golden()
    T, lens = 24, [24, 2, 1]
    j, r = fk("t2m", T, tuple(lens))
    rows = torch.from_numpy(z["t2m_noisy_rows"]).cuda()
    j2, r2 = P.remove_foot_skate(j, lens, (rows, z["t2m_mean"], z["t2m_std"]), rotations=r)
    assert not torch.equal(j2, j)
    rest = MM.rest_pose(z["t2m_offsets"], "t2m").astype(np.float32)
    feet = list(pkg("motion_features").get_skeleton("t2m").feet)
    idx, w = np.zeros((len(feet), 4), int), np.zeros((len(feet), 4))
    idx[:, 0], w[:, 0] = feet, 1.0
    mesh = MM.Mesh(rest[feet], np.zeros((1, 3), int), idx, w, rest, None, None, "t2m")
    out = MM.skin_vertices(mesh, j2, r2, lens)
    want = [(j2[b, :n][:, feet].cpu().numpy().astype(np.float64),) for b, n in enumerate(lens)]
    yard = worst(restated(mesh, "t2m", j2, r2, lens, np.float32), want, 0)
    err = worst([(out[b, :n].cpu().numpy(),) for b, n in enumerate(lens)], want, 0)
    print(f"pinned feet {err:.3g} (yardstick {yard:.3g})")
    assert err <= GATE * yard, (err, yard)


def first_key(glb, mesh, rig, off, j, r, vertices):
    """-> (how far the file's key 0, evaluated in fp64, lies from the device's ``vertices`` of frame 0; the yardstick: the same
    chain in the fp32 restatements, rig keys -> file -> evaluator against the fp32 skinning).  One motion (n, J, ...)."""
    MM = pkg("motion_mesh")
    P, R, off = j[:1].cpu().numpy(), r[:1].cpu().numpy(), off.cpu().numpy()
    c32, q32 = RR.rig_channels(rig, P, R, dtype=np.float32)
    ref = MR.read_glb(MM.glb_bytes(mesh, rig, off, c32[:, :3], q32, 1, 0.05))
    fp32 = MR.skin(parents_of("t2m"), P, R, mesh.vertices, None, mesh.bind_joints, None, mesh.bone_index, mesh.bone_weight, np.float32)[0]
    return (float(np.abs(MR.gltf_vertices(glb, 0) - vertices[0].cpu().numpy()).max()),
            float(np.abs(MR.gltf_vertices(ref, 0) - fp32[0]).max()))


def test_through_the_trainer(tmp_path):
    import test_motion_features_gpu as TF
    import test_motion_fk_gpu as TK
    MM, MRig = pkg("motion_mesh"), pkg("motion_rig")
    tr = TF._tiny_trainer()
    mean, std = TK._mean_std(263, 22, 12)
    caps, lens = ["a", "b", "c", "d"], [16, 16, 12, 9]   # batches of two: the denoiser takes even T
    opts = dict(seed=0, sampler="ddim", sample_steps=5, batch_size=2, fix_feet=True)
    res = tr.generate_mesh(caps, torch.tensor(lens), 263, mean, std, normals=True, **opts)
    rot = tr.generate_rotations(caps, torch.tensor(lens), 263, mean, std, **opts)
    V = MM.capsule_body(rot[0][2].cpu(), "t2m").n_vertices
    assert len(res) == 4
    for i, n in enumerate(lens):
        v, nr, faces = res[i]
        assert v.shape == (n, V, 3) and nr.shape == (n, V, 3) and v.is_cuda and faces is res[0][2] and faces.shape[1] == 3
        assert float((nr.norm(dim=-1) - 1).abs().max()) < 1e-5
        jo, ro, of = rot[i]
        body = MM.capsule_body(of.cpu(), "t2m")                                 # the body of the offsets used
        again = MM.skin_vertices(body, jo[None], ro[None])
        assert torch.equal(again[0], v), i
    plain = tr.generate_mesh(caps, torch.tensor(lens), 263, mean, std, **opts)
    assert len(plain[0]) == 2 and torch.equal(plain[2][0], res[2][0])
    paths = [str(tmp_path / "a.glb"), None, str(tmp_path / "c.glb"), None]
    blobs = tr.generate_glb(caps, torch.tensor(lens), 263, mean, std, fps_out=30, paths=paths, **opts)
    assert sorted(os.listdir(tmp_path)) == ["a.glb", "c.glb"] and open(paths[0], "rb").read() == blobs[0]
    rig = MRig.rig_of("t2m")
    for i, n in enumerate(lens):
        glb = MR.read_glb(blobs[i])
        m = (n - 1) * 3 // 2 + 1                                                 # lengths_out at 20 -> 30
        times = glb.accessor(glb.doc["animations"][0]["samplers"][0]["input"])
        assert len(times) == m and abs(float(times[1]) - 1 / 30) < 1e-7 and len(glb.doc["nodes"]) == rig.n_nodes + 1
        jo, ro, of = rot[i]
        err, yard = first_key(glb, MM.capsule_body(of.cpu(), "t2m"), rig, of, jo, ro, res[i][0])   # key 0 is frame 0
        print("generate_glb", i, f"key 0 {err:.3g} (yardstick {yard:.3g})")
        assert err <= GATE * yard, (i, err, yard)
    scripts = [[("a", 16), ("b", 16)]]
    lopts = dict(overlap=4, seed=4, sampler="ddim", sample_steps=5)
    path = str(tmp_path / "long.glb")
    (blob,) = tr.generate_long_glb(scripts, 263, mean, std, fps_out=30, paths=[path], **lopts)
    glb = MR.read_glb(blob)
    assert open(path, "rb").read() == blob
    assert glb.doc["accessors"][glb.doc["animations"][0]["samplers"][0]["input"]]["count"] == (28 - 1) * 3 // 2 + 1
    ((lv, lf),) = tr.generate_long_mesh(scripts, 263, mean, std, **lopts)
    canvases = tr.generate_long(scripts, 263, **lopts)
    ((lj, lr, lo),) = pkg("motion_outputs").to_joints(canvases, [28], 263, mean, std, 22, 0.0, True, None, True)
    err, yard = first_key(glb, MM.capsule_body(lo.cpu(), "t2m"), rig, lo, lj, lr, lv)
    print(f"generate_long_glb key 0 {err:.3g} (yardstick {yard:.3g})")
    assert lv.shape == (28, V, 3) and lf.shape[1] == 3 and err <= GATE * yard, (err, yard)
    with pytest.raises(ValueError):
        tr.generate_glb(caps, torch.tensor(lens), 263, mean, std, paths=paths[:2], **opts)


def test_bad_arguments_on_the_device_path():
    MM, L = pkg("motion_mesh"), pkg("_lib")
    off = golden()["t2m_offsets"]
    mesh = MM.capsule_body(off, "t2m")
    j, r = torch.zeros(2, 8, 22, 3, device="cuda"), torch.zeros(2, 8, 22, 3, 3, device="cuda")
    assert MM.skin_vertices(mesh, j, r).shape == (2, 8, mesh.n_vertices, 3)
    with pytest.raises(ValueError):
        MM.skin_vertices(MM.capsule_body(golden()["kit_offsets"], "kit"), j, r)          # wrong J for the skeleton
    with pytest.raises(ValueError):
        MM.skin_vertices(mesh, j, r[:, :7])
    with pytest.raises(ValueError):
        MM.skin_vertices(mesh, j, r, [8, 9])
    with pytest.raises(ValueError):
        MM.skin_vertices(MM.capsule_body(np.stack([off] * 3), "t2m"), j, r)               # (B', V, 3) with B' != B
    with pytest.raises(ValueError):
        MM.skin_vertices("t2m", j, r)
    for a, b in ((j, r.cpu()), (j.cpu(), r), (j.cpu(), r.cpu())):
        with pytest.raises((L.MdmError, ValueError)):
            MM.skin_vertices(mesh, a, b)                                                  # no eager fallback
    with pytest.raises(L.MdmError):
        MM.skin_vertices(mesh, j.cpu(), r.cpu())
    lib = L.lib()
    p = j.data_ptr()
    args = lambda J, V, T: (p, p, None, 1, T, J, (ctypes.c_int32 * 33)(*([-1] + [0] * 32)), p, None, V, 0, p, 0, None, p, p, p, None, None)
    assert lib.mdm_skin_vertices(*args(33, 1, 1)) == 3                                    # MDM_ERR_UNSUPPORTED
    assert lib.mdm_skin_vertices(*args(22, 0, 1)) == 1 and lib.mdm_skin_vertices(*args(22, 1, 0)) == 1   # MDM_ERR_ARG

"""CPU: the skinned body output without a device: the capsule body, ``Mesh`` and its helpers, the glTF binary's
structure, and its meaning: the file read back by an independent reader and evaluated in float64 (tests/mesh_ref.py) against
the float64 restatement of linear blend skinning from the global rotations.

Tolerances.  GATE = 4 x a yardstick (the convention of tests/test_motion_rig_gpu.py).  For the restatement the yardstick is how
far the all-fp32 restatement lies from the fp64 one on the same inputs; for the file it is how far the file written from the
fp32 rig restatement's keys (tests/rig_ref.py) evaluates from the fp64 skinning.  ``test_selectivity`` shows that each of seven
mistakes lies more than 100 gates away (measured: 8e4 gates at the least, see its printout and DESIGN.md §30).
"""
import functools
import os
import struct

import numpy as np
import pytest

from conftest import GOLDEN, pkg

import mesh_ref as MR
import rig_ref as RR

GATE = 4.0
T = 24


@functools.lru_cache(maxsize=None)
def case(skel):
    """A golden case of tests/golden/motion_fk.npz, sample 0: fp32-valued joints and rotations (the inputs of every
    restatement), the offsets they were made on, the rig, and the fp64 / fp32 keys of the rig restatement."""
    z = np.load(os.path.join(GOLDEN, "motion_fk.npz"))
    P, R = z[f"{skel}_clean_joints64"][:T].astype(np.float32), z[f"{skel}_clean_rotations64"][:T].astype(np.float32)
    off = z[f"{skel}_clean_offsets64"][0]
    rig = pkg("motion_rig").rig_of(skel)
    parents = list(pkg("motion_features").get_skeleton(skel).parents)
    for c in range(1, len(parents)):  # the joints are the forward kinematics of the rotations on these offsets
        assert np.abs(P[:, c] - P[:, parents[c]] - R[:, c].astype(np.float64) @ off[c]).max() < 1e-5
    keys = {dt: RR.rig_channels(rig, P, R, dtype=dt) for dt in (np.float64, np.float32)}
    return P, R, off, rig, parents, keys


def distorted(skel, seed=5):
    """A mesh whose bind pose is not our rest pose: other bone lengths (x 0.7 .. 1.4) and directions tilted by 10 to 30
    degrees, a capsule body about those bind joints, ``bind_rotations`` from the helper."""
    MM = pkg("motion_mesh")
    _, _, off, _, parents, _ = case(skel)
    rs = np.random.RandomState(seed)
    tilted = np.zeros_like(off)
    for c in range(1, len(off)):
        axis = np.cross(off[c], rs.randn(3))  # across the bone: the whole angle tilts it
        tilted[c] = rs.uniform(0.7, 1.4) * RR.rodrigues(axis / np.linalg.norm(axis), np.deg2rad(rs.uniform(10, 30))) @ off[c]
    body = MM.capsule_body(tilted, skel)
    return MM.Mesh(body.vertices, body.faces, body.bone_index, body.bone_weight, body.bind_joints,
                   MM.bind_rotations(body.bind_joints, off, skel), body.normals, skel)


def file_vertices(mesh, skel, dtype, scale, frames, **kw):
    """glb_bytes from the rig restatement's keys in ``dtype`` -> the fp64 evaluator's vertices at ``frames``."""
    MM = pkg("motion_mesh")
    _, _, off, rig, _, keys = case(skel)
    chan, quat = keys[dtype]
    glb = MR.read_glb(MM.glb_bytes(mesh, rig, off, chan[:, :3], quat, T, 0.05, scale))
    return np.stack([MR.gltf_vertices(glb, k, **kw) for k in frames])


def truth(mesh, skel, dtype=np.float64, variant=None, weights=None):
    P, R, _, _, parents, _ = case(skel)
    return MR.skin(parents, P, R, mesh.vertices, mesh.normals, mesh.bind_joints, mesh.bind_rotations, mesh.bone_index,
                   mesh.bone_weight if weights is None else weights, dtype, variant)


# ---- the capsule body ----

@pytest.mark.parametrize("skel", ["t2m", "kit"])
def test_capsule_body(skel):
    MM = pkg("motion_mesh")
    _, _, off, _, parents, _ = case(skel)
    S, Rg = 12, 4
    body = MM.capsule_body(off, skel, segments=S, rings=Rg)
    J = len(parents)
    sizes = [2 + (2 * Rg - 1) * S] + [2 + 2 * Rg * S] * (J - 1)
    assert body.vertices.shape == (sum(sizes), 3) and body.faces.shape == (4 * S * Rg * J - 2 * S, 3)
    assert body.bind_rotations is None and body.normals.shape == body.vertices.shape
    # closed and oriented: every directed edge once, its reverse once
    f = body.faces.astype(np.int64)
    directed = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    code = directed[:, 0] * len(body.vertices) + directed[:, 1]
    assert len(np.unique(code)) == len(code)
    assert np.array_equal(np.sort(code), np.sort(directed[:, 1] * len(body.vertices) + directed[:, 0]))
    rest = MM.rest_pose(off, skel)
    assert np.array_equal(body.bind_joints, rest.astype(np.float32))
    height = rest[:, 1].max() - rest[:, 1].min()
    rho = np.cos(np.pi / S) * np.cos(np.pi / (4 * Rg))  # the inscribed polyhedron holds the capsule of radius rho r
    v = body.vertices.astype(np.float64)
    start = 0
    for c, n in enumerate(sizes):
        r = MM.BODY_RADII[skel][c] * height
        a, e = (rest[0], rest[0]) if c == 0 else (rest[parents[c]], rest[c])
        own = (f[:, 0] >= start) & (f[:, 0] < start + n)
        assert ((f[own] >= start) & (f[own] < start + n)).all()  # a component of its own
        tri = v[f[own]]
        volume = np.einsum("fi,fi->f", tri[:, 0], np.cross(tri[:, 1], tri[:, 2])).sum() / 6
        length = np.linalg.norm(e - a)
        analytic = np.pi * r * r * length + 4 / 3 * np.pi * r ** 3
        assert rho ** 3 * analytic * (1 - 1e-5) <= volume <= analytic * (1 + 1e-5), (c, volume, analytic)
        p = v[start:start + n]
        s = np.clip((p - a) @ (e - a) / max(length ** 2, 1e-30), 0, 1)
        dist = np.linalg.norm(p - (a + s[:, None] * (e - a)), axis=1)
        assert np.abs(dist - r).max() <= 8 * np.finfo(np.float32).eps * np.abs(p).max(), (c, np.abs(dist - r).max())
        # the normals are the capsule's own: unit, along the offset from the segment
        assert np.abs(body.normals[start:start + n] * r - (p - (a + s[:, None] * (e - a)))).max() < 1e-5
        # weights: at most two, on bone c and bone parent(c)
        idx, w = body.bone_index[start:start + n], body.bone_weight[start:start + n]
        assert np.abs(w.sum(1, dtype=np.float64) - 1).max() <= 2 ** -23 and (w[:, 2:] == 0).all()
        assert (idx[:, 0] == c).all() and (w[:, 0] >= 0.5).all()
        assert (idx[:, 1][w[:, 1] > 0] == (parents[c] if c else 0)).all()
        axial = (p - a) @ (e - a) / max(length ** 2, 1e-30)
        want = np.zeros(n) if c == 0 else np.maximum(0, 0.5 * (1 - np.maximum(axial, 0) / 0.25))
        assert np.abs(w[:, 1] - want).max() < 1e-6, c
        start += n
    again = MM.capsule_body(off, skel, segments=S, rings=Rg)
    for name in ("vertices", "faces", "bone_index", "bone_weight", "bind_joints", "normals"):
        assert np.array_equal(getattr(again, name), getattr(body, name)), name


def test_capsule_body_per_sample():
    MM = pkg("motion_mesh")
    _, _, off, _, _, _ = case("t2m")
    batch = np.stack([off, 1.1 * off, off * np.array([1.0, 0.9, 1.0])])
    body = MM.capsule_body(batch, "t2m")
    assert body.batch == 3 and body.vertices.ndim == 3 and body.bind_joints.shape == (3, 22, 3)
    for b in range(3):
        one = MM.capsule_body(batch[b], "t2m")
        assert one.batch is None
        part = body.sample(b)
        for name in ("vertices", "faces", "bone_index", "bone_weight", "bind_joints", "normals"):
            assert np.array_equal(getattr(part, name), getattr(one, name)), (b, name)
    with pytest.raises(ValueError):
        MM.capsule_body(off[:5], "t2m")
    with pytest.raises(ValueError):
        MM.capsule_body(off, "t2m", segments=2)
    with pytest.raises(ValueError):
        MM.capsule_body(off, "t2m", radii=np.zeros(22))


# ---- Mesh, from_dense_weights, bind_rotations, vertex_normals ----

def _tetrahedron():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64)
    f = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])
    return v, f


def test_mesh_validation():
    MM = pkg("motion_mesh")
    v, f = _tetrahedron()
    idx, w = np.zeros((4, 4), int), np.tile([2.0, 1.0, 1.0, 0.0], (4, 1))
    idx[:, 1], idx[:, 2], idx[:, 3] = 3, 5, 21
    G = np.zeros((22, 3))
    m = MM.Mesh(v, f, idx, w, G)
    assert m.bone_weight.dtype == np.float32 and np.array_equal(m.bone_weight[0], np.float32([0.5, 0.25, 0.25, 0]))
    assert m.bone_index.tolist()[0] == [0, 3, 5, 21] and m.faces.dtype == np.int32 and m.batch is None
    third = MM.Mesh(v, f, idx, np.tile([1.0, 1.0, 1.0, 0.0], (4, 1)), G).bone_weight
    assert np.array_equal(third[0, :3], np.float32([1 / 3] * 3))           # normalised in float64, then rounded
    bad = lambda **kw: pytest.raises(ValueError)
    cases = [dict(vertices=np.where(np.eye(4, 3) > 0, np.nan, v)), dict(bind_joints=np.full((22, 3), np.inf)),
             dict(bone_index=np.where(idx == 21, 22, idx)), dict(bone_index=np.where(idx == 0, -1, idx)),
             dict(bone_weight=np.where(w == 2, -1.0, w)), dict(bone_weight=np.where(np.arange(4)[:, None] == 2, 0.0, w)),
             dict(faces=np.where(f == 3, 4, f)), dict(faces=f.astype(np.float64)), dict(bind_joints=np.zeros((21, 3))),
             dict(normals=np.zeros((3, 3))), dict(bind_rotations=np.zeros((22, 3))), dict(vertices=np.zeros((0, 3)))]
    for kw in cases:
        args = dict(vertices=v, faces=f, bone_index=idx, bone_weight=w, bind_joints=G)
        args.update(kw)
        with pytest.raises(ValueError):
            MM.Mesh(**args)
    with pytest.raises(ValueError):  # per-sample bind joints need per-sample vertices
        MM.Mesh(v, f, idx, w, np.zeros((2, 22, 3)))


def test_from_dense_weights():
    MM = pkg("motion_mesh")
    v, f = _tetrahedron()
    dense = np.zeros((4, 22))
    dense[:, [1, 4, 7, 10, 20]] = [0.1, 0.3, 0.2, 0.3, 0.1]
    dense[1] = 0
    dense[1, 6] = 5.0
    m = MM.from_dense_weights(v, f, dense, np.zeros((22, 3)))
    assert m.bone_index[0].tolist() == [4, 10, 7, 1]                          # the lower index first among equal weights
    assert np.array_equal(m.bone_weight[0], (np.array([0.3, 0.3, 0.2, 0.1]) / 0.9).astype(np.float32))
    assert m.bone_index[1, 0] == 6 and m.bone_weight[1].tolist() == [1, 0, 0, 0]
    two = MM.from_dense_weights(v, f, dense, np.zeros((22, 3)), top=2)
    assert np.array_equal(two.bone_weight[0], np.float32([0.5, 0.5, 0, 0])) and two.bone_index[0, :2].tolist() == [4, 10]
    for wrong in (dict(weights=-dense), dict(weights=dense[:, :21]), dict(weights=dense * 0), dict(top=5), dict(top=0)):
        args = dict(weights=dense)
        args.update(wrong)
        with pytest.raises(ValueError):
            MM.from_dense_weights(v, f, args.pop("weights"), np.zeros((22, 3)), **args)


@pytest.mark.parametrize("skel", ["t2m", "kit"])
def test_bind_rotations(skel):
    MM = pkg("motion_mesh")
    _, _, off, _, parents, _ = case(skel)
    rest = MM.rest_pose(off, skel)
    assert np.array_equal(MM.bind_rotations(rest, off, skel), np.tile(np.eye(3), (len(off), 1, 1)))  # our own rest pose
    m = distorted(skel)
    G, Q = m.bind_joints.astype(np.float64), MM.bind_rotations(m.bind_joints, off, skel)
    assert np.array_equal(Q[0], np.eye(3))
    for c in range(1, len(off)):
        d, u = G[c] - G[parents[c]], off[c] / np.linalg.norm(off[c])
        assert np.abs(Q[c] @ u - d / np.linalg.norm(d)).max() < 1e-6 and np.abs(Q[c].T @ Q[c] - np.eye(3)).max() < 1e-12
        assert not np.allclose(Q[c], np.eye(3), atol=0.05)
    flat = rest.copy()
    flat[5] = flat[parents[5]]                                                # a bone without length: the identity
    assert np.array_equal(MM.bind_rotations(flat, off, skel)[5], np.eye(3))


def test_vertex_normals_and_obj(tmp_path):
    MM = pkg("motion_mesh")
    body = MM.capsule_body(case("t2m")[2], "t2m", segments=24, rings=8)
    n = MM.vertex_normals(body.vertices, body.faces)
    assert n.dtype == np.float32 and np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-6
    assert (n * body.normals).sum(1).min() > 0.97                             # the faces' normals follow the capsules' own
    v, f = _tetrahedron()
    loose = MM.vertex_normals(np.concatenate([v, [[5, 5, 5]]]), f)
    assert not loose[4].any() and np.allclose(loose[0], -np.ones(3) / np.sqrt(3))
    text = MM.write_obj(tmp_path / "a.obj", v, f, MM.vertex_normals(v, f))
    lines = text.splitlines()
    assert open(tmp_path / "a.obj").read() == text and len(lines) == 12 and lines[0] == "v 0 0 0" and lines[-1] == "f 2//2 3//3 4//4"
    assert MM.write_obj(tmp_path / "b.obj", v, f).splitlines()[-1] == "f 2 3 4"


# ---- the glTF binary ----

def test_glb_structure():
    MM = pkg("motion_mesh")
    _, _, off, rig, _, keys = case("t2m")
    chan, quat = keys[np.float32]
    quat = quat.copy()
    quat[7:, 3] *= -1                                                          # a key on the far hemisphere: the writer flips it back
    mesh = MM.capsule_body(off, "t2m")
    data = MM.glb_bytes(mesh, rig, off, chan[:, :3], quat, T, 0.05, scale=100.0)
    magic, version, total = struct.unpack_from("<4sII", data, 0)
    n_json, k_json = struct.unpack_from("<I4s", data, 12)
    n_bin, k_bin = struct.unpack_from("<I4s", data, 20 + n_json)
    assert (magic, version, total) == (b"glTF", 2, len(data)) and k_json == b"JSON" and k_bin == b"BIN\0"
    assert n_json % 4 == 0 and n_bin % 4 == 0 and 28 + n_json + n_bin == len(data)
    text = data[20:20 + n_json]
    assert text.rstrip(b" ").endswith(b"}") and len(text) - len(text.rstrip(b" ")) < 4
    glb = MR.read_glb(data)
    doc = glb.doc
    N, V = rig.n_nodes, mesh.n_vertices
    assert doc["asset"]["version"] == "2.0" and doc["buffers"] == [dict(byteLength=n_bin)]
    ends = sorted((v["byteOffset"], v["byteOffset"] + v["byteLength"]) for v in doc["bufferViews"])
    assert all(a % 4 == 0 for a, _ in ends) and all(e0 <= a1 for (_, e0), (a1, _) in zip(ends[:-1], ends[1:])) and ends[-1][1] <= n_bin
    for (_, e0), (a1, _) in zip(ends, ends[1:] + [(n_bin, 0)]):
        assert not any(glb.bin[e0:a1]) and a1 - e0 < 4                        # zeros pad a view to 4 bytes
    arrays = [glb.accessor(i) for i in range(len(doc["accessors"]))]           # every accessor inside its view and buffer
    assert len(doc["nodes"]) == N + 1 and [n["name"] for n in doc["nodes"][:N]] == list(rig.names)
    assert doc["skins"][0]["joints"] == list(range(N)) and doc["nodes"][N] == dict(name="body", mesh=0, skin=0)
    assert doc["scenes"][0]["nodes"] == [0, N]
    prim = doc["meshes"][0]["primitives"][0]
    pos, a_pos = arrays[prim["attributes"]["POSITION"]], doc["accessors"][prim["attributes"]["POSITION"]]
    assert np.array_equal(pos, np.float32(100.0) * mesh.vertices)
    assert a_pos["min"] == pos.min(0).tolist() and a_pos["max"] == pos.max(0).tolist() and a_pos["count"] == V
    assert np.array_equal(arrays[prim["attributes"]["NORMAL"]], mesh.normals)
    j0, w0 = arrays[prim["attributes"]["JOINTS_0"]], arrays[prim["attributes"]["WEIGHTS_0"]]
    assert j0.dtype == np.uint8 and w0.dtype == np.float32 and np.array_equal(w0, mesh.bone_weight) and not j0[w0 == 0].any()
    node_of, at = MM.skin_nodes(rig, "t2m")
    pivots = MR.pivots(pkg("motion_features").get_skeleton("t2m").parents)
    for c, n in enumerate(node_of):                                            # the node at pivot(c) that carries R[c]
        assert n >= 0 and rig.carried[n] == c and at[n] == pivots[c]
    assert np.array_equal(j0[w0 > 0], np.asarray(node_of)[mesh.bone_index[w0 > 0]])
    idx = arrays[prim["indices"]]
    assert idx.dtype == np.uint32 and np.array_equal(idx.reshape(-1, 3), mesh.faces)
    for n in range(1, N):
        want = (100.0 * off[rig.joint_of[n]]).astype(np.float32).tolist() if rig.has_offset[n] else None
        assert doc["nodes"][n].get("translation") == want, n
    anim = doc["animations"][0]
    assert len(anim["channels"]) == N + 1 and anim["channels"][0]["target"] == dict(node=0, path="translation")
    assert [c["target"] for c in anim["channels"][1:]] == [dict(node=n, path="rotation") for n in range(N)]
    a_time = doc["accessors"][anim["samplers"][0]["input"]]
    times = arrays[anim["samplers"][0]["input"]]
    assert all(s["input"] == anim["samplers"][0]["input"] and s["interpolation"] == "LINEAR" for s in anim["samplers"])
    assert np.array_equal(times, (np.arange(T) * 0.05).astype(np.float32))
    assert a_time["min"] == [0.0] and a_time["max"] == [float(times[-1])]
    assert np.array_equal(arrays[anim["samplers"][0]["output"]], np.float32(100.0) * chan[:, :3])
    for n in range(N):
        q = arrays[anim["samplers"][n + 1]["output"]]
        assert q.shape == (T, 4) and np.abs(np.linalg.norm(q.astype(np.float64), axis=1) - 1).max() <= 4 * np.finfo(np.float32).eps
        assert ((q[1:] * q[:-1]).sum(1) >= 0).all(), n                         # neighbouring keys on one hemisphere
        same = np.all(q == quat[:, n][:, [1, 2, 3, 0]], axis=1) | np.all(q == -quat[:, n][:, [1, 2, 3, 0]], axis=1)
        assert same.all()                                                      # reordered and at most negated, bit for bit
    with pytest.raises(ValueError):
        MM.glb_bytes(mesh, rig, off, chan[:, :3], quat, T + 1, 0.05)
    with pytest.raises(ValueError):
        MM.glb_bytes(mesh, rig, off, chan[:, :3], quat[:, :-1], T, 0.05)
    with pytest.raises(ValueError):
        MM.glb_bytes(MM.capsule_body(np.stack([off, off]), "t2m"), rig, off, chan[:, :3], quat, T, 0.05)
    # a weighted bone that no node carries at its pivot
    lame = pkg("motion_rig").rig_of("t2m")
    lame = type(lame)(**{**vars(lame), "carried": [c if c != 4 else -1 for c in lame.carried]})
    with pytest.raises(ValueError, match=r"\[4\]"):
        MM.glb_bytes(mesh, lame, off, chan[:, :3], quat, T, 0.05)


FRAMES = (0, 7, 23)
SEMANTICS = [("t2m", "capsule", 1.0), ("kit", "capsule", 1.0), ("t2m", "distorted", 100.0), ("kit", "distorted", 100.0)]


def _mesh(skel, which):
    return pkg("motion_mesh").capsule_body(case(skel)[2], skel) if which == "capsule" else distorted(skel)


@pytest.mark.parametrize("skel,which,scale", SEMANTICS)
def test_glb_semantics(skel, which, scale):
    """The file, written from the fp64 rig restatement's keys, read back and evaluated in fp64, gives the fp64 skinning."""
    mesh = _mesh(skel, which)
    want = scale * truth(mesh, skel)[0][list(FRAMES)]
    yard = float(np.abs(file_vertices(mesh, skel, np.float32, scale, FRAMES) - want).max())
    err = float(np.abs(file_vertices(mesh, skel, np.float64, scale, FRAMES) - want).max())
    print(skel, which, f"scale {scale:g}: file {err:.3g} (yardstick {yard:.3g})")
    assert 0 < yard < 1e-5 * scale and err <= GATE * yard, (err, yard)


@pytest.mark.parametrize("skel", ["t2m", "kit"])
def test_selectivity(skel):
    """Each mistake lies more than 100 gates from the truth, on the restatements alone."""
    mesh = distorted(skel)
    _, _, _, rig, parents, _ = case(skel)
    want_v, want_n = truth(mesh, skel)
    fp32_v, fp32_n = truth(mesh, skel, np.float32)
    gate_v, gate_n = GATE * float(np.abs(fp32_v - want_v).max()), GATE * float(np.abs(fp32_n - want_n).max())
    print(skel, f"restatement gates: vertices {gate_v:.3g} normals {gate_n:.3g}")
    multiples = {}
    for variant in ("pivot_child", "R_transposed", "Q_not_transposed"):
        v, n = truth(mesh, skel, variant=variant)
        multiples[variant] = float(np.abs(v - want_v).max()) / gate_v
        if variant != "pivot_child":
            multiples[variant + " (normals)"] = float(np.abs(n - want_n).max()) / gate_n
    raw = mesh.bone_weight * np.float32(1.25)
    multiples["weights not normalised"] = float(np.abs(truth(mesh, skel, weights=raw)[0] - want_v).max()) / gate_v
    scale = 100.0
    want = scale * want_v[list(FRAMES)]
    gate_f = GATE * float(np.abs(file_vertices(mesh, skel, np.float32, scale, FRAMES) - want).max())
    node_of, _ = pkg("motion_mesh").skin_nodes(rig, skel)
    at_child = {node_of[c]: rig.joint_of.index(c) for c in range(len(parents))}
    for name, kw in (("quaternion order", dict(variant="wxyz")), ("row-major inverse bind matrix", dict(variant="row_major_ibm")),
                     ("weights on the node at c", dict(rebind=at_child))):
        multiples[name] = float(np.abs(file_vertices(mesh, skel, np.float64, scale, FRAMES, **kw) - want).max()) / gate_f
    for name, m in multiples.items():
        print(skel, f"{name}: {m:.3g} gates")
        assert m > 100, (name, m)

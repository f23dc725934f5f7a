"""Numpy restatement of the skinned body output, shared by tests/test_motion_mesh_host.py and
tests/test_motion_mesh_gpu.py.

Independent of motion_mesh.py and csrc/motion_skin.hip but for the tables that are data (a skeleton's parents, ``rig_of``'s
node tree):

* ``skin``: the formulas of linear blend skinning as the issue states them, in the dtype asked for (float64: the truth;
  float32: the yardstick), A_c(x) = P[pivot(c)] + R[c] Q[c]^T (x - G[pivot(c)]), v' = sum_k w_k A_{idx_k}(v), n' =
  normalise(sum_k w_k R Q^T n);
* ``read_glb``: a GLB reader made of ``struct`` and ``json`` that knows nothing of the writer: header and chunks, accessors to
  arrays;
* ``gltf_vertices``: what a glTF player computes at key k, in float64: node TRS -> global matrices down the tree -> G IBM ->
  skinned vertices.

``variant`` builds the mistakes an implementation most easily makes (tests/test_motion_mesh_host.py measures how far each lies
from the truth).  In ``skin``: "pivot_child" (bone c turns about joint c), "R_transposed", "Q_not_transposed".  In
``gltf_vertices``, each the reading that undoes nothing of a writer's mistake, so the same wrong vertices: "wxyz" (the keys not
reordered to x, y, z, w), "row_major_ibm" (the inverse bind matrices written by rows), and ``rebind`` (a map from skin joint
to skin joint: the weights bound to the node at joint c instead of the node at pivot(c))."""
import json
import struct
from types import SimpleNamespace

import numpy as np


def pivots(parents):
    return [0] + [int(p) for p in parents[1:]]


def skin(parents, P, R, v, n, G, Q, idx, w, dtype=np.float64, variant=None):
    """One sample.  P (T, J, 3), R (T, J, 3, 3), v (V, 3), n (V, 3) or None, G (J, 3), Q (J, 3, 3) or None, idx / w (V, 4)
    -> (vertices (T, V, 3), normals (T, V, 3) or None), every operation in ``dtype``."""
    dtype = np.dtype(dtype)
    P, R, v, G, w = (np.asarray(a).astype(dtype) for a in (P, R, v, G, w))
    J = len(parents)
    piv = np.arange(J) if variant == "pivot_child" else np.asarray(pivots(parents))
    Q = np.broadcast_to(np.eye(3, dtype=dtype), (J, 3, 3)) if Q is None else np.asarray(Q).astype(dtype)
    if variant == "R_transposed":
        R = np.swapaxes(R, -1, -2)
    M = R @ (Q if variant == "Q_not_transposed" else np.swapaxes(Q, -1, -2))  # (T, J, 3, 3)
    out = np.zeros((len(P), len(v), 3), dtype)
    nout = None if n is None else np.zeros((len(P), len(v), 3), dtype)
    n = None if n is None else np.asarray(n).astype(dtype)
    for k in range(idx.shape[1]):
        c = np.asarray(idx[:, k])
        live = (w[:, k] != 0)[None, :, None]
        y = v - G[piv[c]]                                                   # (V, 3)
        A = P[:, piv[c]] + np.einsum("tvij,vj->tvi", M[:, c], y)            # (T, V, 3)
        out = out + np.where(live, w[None, :, k, None] * A, dtype.type(0))  # a slot of weight 0 contributes nothing
        if n is not None:
            nout = nout + np.where(live, w[None, :, k, None] * np.einsum("tvij,vj->tvi", M[:, c], n), dtype.type(0))
    if n is not None:
        length = np.sqrt((nout * nout).sum(-1, keepdims=True))
        nout = nout / np.where(length > 0, length, dtype.type(1))
        assert nout.dtype == dtype
    assert out.dtype == dtype
    return out, nout


_COMPONENT = {5120: np.int8, 5121: np.uint8, 5122: np.int16, 5123: np.uint16, 5125: np.uint32, 5126: np.float32}
_WIDTH = {"SCALAR": 1, "VEC2": 2, "VEC3": 3, "VEC4": 4, "MAT4": 16}


def read_glb(data):
    """GLB bytes -> a namespace: ``doc`` (the JSON), ``bin`` (the BIN chunk's bytes as the chunk header counts them),
    ``json_bytes``, ``total`` (the header's length) and ``accessor(i)`` -> the array (count, width) (count,) for SCALAR.
    Asserts the container's structure on the way."""
    magic, version, total = struct.unpack_from("<4sII", data, 0)
    assert magic == b"glTF" and version == 2 and total == len(data)
    n_json, kind = struct.unpack_from("<I4s", data, 12)
    assert kind == b"JSON" and n_json % 4 == 0
    text = data[20:20 + n_json]
    n_bin, kind = struct.unpack_from("<I4s", data, 20 + n_json)
    assert kind == b"BIN\0" and n_bin % 4 == 0 and 28 + n_json + n_bin == total
    blob = data[28 + n_json:]
    doc = json.loads(text.decode("ascii"))

    def accessor(i):
        a = doc["accessors"][i]
        view = doc["bufferViews"][a["bufferView"]]
        dt, width = np.dtype(_COMPONENT[a["componentType"]]), _WIDTH[a["type"]]
        start = view["byteOffset"] + a.get("byteOffset", 0)
        size = a["count"] * width * dt.itemsize
        assert view["byteOffset"] % 4 == 0 and start % dt.itemsize == 0 and "byteStride" not in view
        assert a.get("byteOffset", 0) + size <= view["byteLength"] and view["byteOffset"] + view["byteLength"] <= len(blob)
        arr = np.frombuffer(blob, dt, a["count"] * width, start)
        return arr if width == 1 else arr.reshape(a["count"], width)

    return SimpleNamespace(doc=doc, bin=blob, json_bytes=text, total=total, accessor=accessor)


def quaternion_matrix_xyzw(q):
    x, y, z, w = (q[..., i] for i in range(4))
    rows = [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
            [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
            [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]
    return np.stack([np.stack(r, -1) for r in rows], -2)


def gltf_vertices(glb, k, variant=None, rebind=None):
    """The skinned vertices (V, 3) float64 of the file's one mesh at animation key k, as a player computes them: the animated
    translations and rotations at that key (the node's own where no channel targets it), global matrices down the tree, joint
    matrices ``G[joint] IBM[joint]``, ``v' = sum_k w_k (joint matrix of JOINTS_0[k]) v``."""
    doc = glb.doc
    nodes = doc["nodes"]
    trans = {i: np.asarray(n.get("translation", (0, 0, 0)), np.float64) for i, n in enumerate(nodes)}
    rot = {i: np.asarray(n.get("rotation", (0, 0, 0, 1)), np.float64) for i, n in enumerate(nodes)}
    anim = doc["animations"][0]
    for ch in anim["channels"]:
        s = anim["samplers"][ch["sampler"]]
        value = glb.accessor(s["output"])[k].astype(np.float64)
        (trans if ch["target"]["path"] == "translation" else rot)[ch["target"]["node"]] = value
    world = {}

    def walk(i, above):
        q = rot[i]
        if variant == "wxyz":
            q = q[[3, 0, 1, 2]]  # the four numbers taken as (w, x, y, z) were written unordered
        m = np.eye(4)
        m[:3, :3], m[:3, 3] = quaternion_matrix_xyzw(q / np.linalg.norm(q)), trans[i]
        world[i] = above @ m
        for c in nodes[i].get("children", []):
            walk(c, world[i])

    for r in doc["scenes"][doc["scene"]]["nodes"]:
        walk(r, np.eye(4))
    (mesh_node,) = [n for n in nodes if "mesh" in n]
    sk = doc["skins"][mesh_node["skin"]]
    ibm = glb.accessor(sk["inverseBindMatrices"]).astype(np.float64).reshape(-1, 4, 4)
    if variant != "row_major_ibm":
        ibm = ibm.transpose(0, 2, 1)  # column-major in the file
    joint = np.stack([world[j] @ ibm[s] for s, j in enumerate(sk["joints"])])
    prim = doc["meshes"][mesh_node["mesh"]]["primitives"][0]["attributes"]
    v = glb.accessor(prim["POSITION"]).astype(np.float64)
    j0, w0 = glb.accessor(prim["JOINTS_0"]).astype(np.int64), glb.accessor(prim["WEIGHTS_0"]).astype(np.float64)
    if rebind is not None:
        j0 = np.vectorize(lambda s: rebind.get(int(s), int(s)))(j0)
    vh = np.concatenate([v, np.ones((len(v), 1))], 1)
    out = np.zeros((len(v), 3))
    for s in range(4):
        out += w0[:, s, None] * np.einsum("vij,vj->vi", joint[j0[:, s]], vh)[:, :3]
    return out

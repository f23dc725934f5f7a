"""Skinned body output: the joints and global rotations of ``postprocess.motion_to_joints_fk`` /
``remove_foot_skate`` / ``pin_limbs`` move the vertices of a mesh, and the mesh, its skin and the animation leave as one
glTF 2.0 binary.

Bones.  A skeleton of J joints has J bones: bone 0 is the root (rotation ``R[0]``, pivot joint 0); bone c >= 1 is the segment
``parent(c) -> c`` (rotation ``R[c]``, pivot joint ``parent(c)``), the convention of csrc/motion_fk.hip.  With the mesh's bind
joints ``G`` and bind rotations ``Q`` (how each bone lies in the mesh's bind pose relative to our rest pose; None: identity):

    A_c(x) = P[t, pivot(c)] + R[t, c] Q[c]^T (x - G[pivot(c)])          v'[t, i] = sum_k w[i, k] A_{idx[i, k]}(v[i])

The arithmetic is in ``mdm_skin_vertices`` (csrc/motion_skin.hip); no eager fallback.  ``Mesh`` holds a user's mesh
(``from_dense_weights`` for one with a (V, J) weight matrix, ``bind_rotations`` for one whose bind pose is not our rest pose),
``capsule_body`` makes a body where the user brings none.  ``glb_bytes`` / ``write_glb`` / ``write_obj`` are host code that moves
and prints numbers and does no arithmetic on the motion beyond ``scale``, a reordering and a sign flip."""
from __future__ import annotations

import ctypes as C
import json
import struct

import numpy as np
import torch

from . import _lib as L
from .motion_features import get_skeleton
from .motion_rig import across, rig_of, shortest_arc

MAX_JOINTS = 32     # of mdm_skin_vertices
INFLUENCES = 4

# Capsule radii per bone as fractions of the rest pose's height (HumanML3D and KIT differ in units).  Bone c >= 1 is the
# segment parent(c) -> c, so "right_knee" is the thigh; bone 0 is the sphere at the pelvis.  A look, not a measurement.
_T2M_RADII = {"pelvis": 0.065, "left_hip": 0.055, "right_hip": 0.055, "spine1": 0.075, "left_knee": 0.05, "right_knee": 0.05,
              "spine2": 0.08, "left_ankle": 0.035, "right_ankle": 0.035, "spine3": 0.085, "left_foot": 0.028, "right_foot": 0.028,
              "neck": 0.04, "left_collar": 0.045, "right_collar": 0.045, "head": 0.06, "left_shoulder": 0.04,
              "right_shoulder": 0.04, "left_elbow": 0.032, "right_elbow": 0.032, "left_wrist": 0.026, "right_wrist": 0.026}


def _t2m_radii():
    from .motion_edit import SMPL_JOINTS
    return tuple(_T2M_RADII[n] for n in SMPL_JOINTS)


BODY_RADII = {
    "t2m": _t2m_radii(),
    # KIT: 0 root, 1-3 spine, 4 head, 5-7 / 8-10 arms (shoulder, upper arm, forearm), 11-15 / 16-20 legs (hip, thigh, shin, feet)
    "kit": (0.065, 0.075, 0.08, 0.085, 0.06, 0.045, 0.032, 0.026, 0.045, 0.032, 0.026,
            0.055, 0.05, 0.035, 0.028, 0.028, 0.055, 0.05, 0.035, 0.028, 0.028),
}


def _np(a, dtype=None):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return a if dtype is None else a.astype(dtype)


def pivots_of(skeleton):
    """-> (parents, pivots) of a skeleton (a name or a namespace of ``motion_features``), as its chains give them: the joint a
    bone turns about is 0 for bone 0 and ``parent(c)`` for bone c."""
    parents = [int(p) for p in get_skeleton(skeleton).parents]
    return parents, [0] + parents[1:]


def rest_pose(offsets, skeleton):
    """Bone offsets (J, 3) or (B, J, 3) -> the joints of the rest pose (every rotation the identity, the root at the origin),
    float64: ``joint[c] = joint[parent(c)] + offset[c]``."""
    off = _np(offsets, np.float64)
    sk = get_skeleton(skeleton)
    out = np.zeros_like(off)
    for chain in sk.chains:  # parents come first along a chain, and a chain starts at a joint that an earlier one reached
        for a, b in zip(chain[:-1], chain[1:]):
            out[..., b, :] = out[..., a, :] + off[..., b, :]
    return out


class Mesh:
    """A skinned mesh, validated, as host arrays: ``vertices`` (V, 3) float32, or (B, V, 3) one body per sample; ``faces``
    (F, 3) int32; ``bone_index`` / ``bone_weight`` (V, 4), the weights normalised to sum 1 in float64 and stored as float32,
    the live slots first in descending weight (a dead slot keeps its index, which nothing reads); ``bind_joints`` (J, 3) or
    (B, J, 3): where the joints sit in the mesh's bind pose; ``bind_rotations`` (J, 3, 3) or None (the identity), see
    ``bind_rotations``; ``normals`` like the vertices, or None; ``skeleton``.  Raises ValueError for shapes that do not fit, non-finite values, an index outside [0, J),
    a negative weight, a vertex whose weights sum to 0, a face that indexes past V, and a skeleton of more than ``MAX_JOINTS``
    joints."""

    def __init__(self, vertices, faces, bone_index, bone_weight, bind_joints, bind_rotations=None, normals=None, skeleton="t2m"):
        sk = get_skeleton(skeleton)
        J = int(sk.joints)
        if J > MAX_JOINTS:
            raise ValueError(f"a skeleton of {J} joints: skinning takes at most {MAX_JOINTS}")
        v = _np(vertices, np.float64)
        if v.ndim not in (2, 3) or v.shape[-1] != 3 or v.shape[-2] < 1 or (v.ndim == 3 and v.shape[0] < 1):
            raise ValueError(f"vertices of shape {v.shape} must be (V, 3) or (B, V, 3)")
        V = v.shape[-2]
        f = _np(faces)
        if f.ndim != 2 or f.shape[1] != 3 or not np.issubdtype(f.dtype, np.integer):
            raise ValueError(f"faces of shape {f.shape} and dtype {f.dtype} must be integer (F, 3)")
        if f.size and (f.min() < 0 or f.max() >= V):
            raise ValueError(f"faces index outside the {V} vertices")
        idx, w = _np(bone_index), _np(bone_weight, np.float64)
        if idx.shape != (V, INFLUENCES) or w.shape != (V, INFLUENCES) or not np.issubdtype(idx.dtype, np.integer):
            raise ValueError(f"bone_index {idx.shape} (integer) and bone_weight {w.shape} must be ({V}, {INFLUENCES})")
        g = _np(bind_joints, np.float64)
        if g.shape[-2:] != (J, 3) or g.ndim not in (2, 3) or (g.ndim == 3 and (v.ndim != 3 or g.shape[0] != v.shape[0])):
            raise ValueError(f"bind_joints of shape {g.shape} must be ({J}, 3), or (B, {J}, 3) beside (B, V, 3) vertices")
        q = None if bind_rotations is None else _np(bind_rotations, np.float64)
        if q is not None and q.shape != (J, 3, 3):
            raise ValueError(f"bind_rotations of shape {q.shape} must be ({J}, 3, 3)")
        n = None if normals is None else _np(normals, np.float64)
        if n is not None and n.shape != v.shape:
            raise ValueError(f"normals of shape {n.shape} must have the vertices' shape {v.shape}")
        for name, a in (("vertices", v), ("bone_weight", w), ("bind_joints", g), ("bind_rotations", q), ("normals", n)):
            if a is not None and not np.isfinite(a).all():
                raise ValueError(f"{name} has non-finite values")
        if (w < 0).any():
            raise ValueError("bone_weight has negative entries")
        total = w.sum(1)
        if not (total > 0).all():
            raise ValueError(f"vertex {int(np.argmin(total > 0))} has weights that sum to 0")
        if ((idx < 0) | (idx >= J)).any():
            raise ValueError(f"bone_index outside [0, {J})")
        w = w / total[:, None]
        order = np.argsort(-w, axis=1, kind="stable")  # live slots first, in descending weight
        w = np.take_along_axis(w, order, 1).astype(np.float32)
        idx = np.take_along_axis(idx, order, 1).astype(np.int32)
        self.vertices, self.faces = v.astype(np.float32), np.ascontiguousarray(f, dtype=np.int32)
        self.bone_index, self.bone_weight = np.ascontiguousarray(idx), np.ascontiguousarray(w)
        self.bind_joints = g.astype(np.float32)
        self.bind_rotations = None if q is None else q.astype(np.float32)
        self.normals = None if n is None else n.astype(np.float32)
        self.skeleton = skeleton
        self._device = {}

    @property
    def n_vertices(self):
        return self.vertices.shape[-2]

    @property
    def batch(self):
        """The number of per-sample bodies, or None for a mesh that the batch shares."""
        return self.vertices.shape[0] if self.vertices.ndim == 3 else None

    def _with(self, **fields):
        """A copy with some fields replaced, as they are: the weights are not normalised a second time (which would move
        them by an ulp), so that a sample taken out of a batch is skinned as it is inside it, bit for bit."""
        other = object.__new__(Mesh)
        other.__dict__.update(self.__dict__)
        other.__dict__.update(fields, _device={})
        return other

    def sample(self, b):
        """The mesh of sample ``b`` alone (the mesh itself where the batch shares it)."""
        if self.batch is None:
            return self
        if not 0 <= int(b) < self.batch:
            raise ValueError(f"sample {b} of a mesh that holds {self.batch}")
        g = self.bind_joints
        return self._with(vertices=self.vertices[b], bind_joints=g[b] if g.ndim == 3 else g,
                          normals=None if self.normals is None else self.normals[b])

    def with_normals(self):
        """The mesh itself where it has normals, else a copy with ``vertex_normals``."""
        if self.normals is not None:
            return self
        v, f = self.vertices, self.faces
        return self._with(normals=vertex_normals(v, f) if v.ndim == 2 else np.stack([vertex_normals(x, f) for x in v]))

    def on(self, device):
        """The arrays ``mdm_skin_vertices`` reads as tensors on ``device``, uploaded once per device."""
        key = str(device)
        if key not in self._device:
            put = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)
            self._device[key] = tuple(put(a) for a in (self.vertices, self.normals, self.bind_joints, self.bind_rotations,
                                                       self.bone_index, self.bone_weight))
        return self._device[key]


def from_dense_weights(vertices, faces, weights, bind_joints, top=INFLUENCES, *, bind_rotations=None, normals=None,
                       skeleton="t2m"):
    """A ``Mesh`` from a user's own skinned mesh with one weight per (vertex, joint): ``weights`` (V, J), column c the weight
    of bone c.  The ``top`` (1 .. 4) largest weights of every vertex are kept, the lower bone index first among equal ones,
    and renormalised to sum 1."""
    w = _np(weights, np.float64)
    J = int(get_skeleton(skeleton).joints)
    if w.ndim != 2 or w.shape[1] != J or not 1 <= int(top) <= INFLUENCES:
        raise ValueError(f"weights of shape {w.shape} must be (V, {J}) and top in [1, {INFLUENCES}]")
    if not np.isfinite(w).all() or (w < 0).any():
        raise ValueError("weights must be finite and not negative")
    keep = min(int(top), w.shape[1])
    order = np.argsort(-w, axis=1, kind="stable")[:, :keep]
    idx, val = np.zeros((len(w), INFLUENCES), np.int64), np.zeros((len(w), INFLUENCES))
    idx[:, :keep], val[:, :keep] = order, np.take_along_axis(w, order, 1)
    return Mesh(vertices, faces, idx, val, bind_joints, bind_rotations, normals, skeleton)


def bind_rotations(bind_joints, offsets, skeleton="t2m"):
    """``Q`` (J, 3, 3) float64 for a mesh whose bind pose is not our rest pose: per bone c >= 1 the shortest-arc rotation
    (``motion_rig.shortest_arc``) from our rest bone direction ``offsets[c]`` to the mesh's, ``bind_joints[c] -
    bind_joints[parent(c)]``; the identity for bone 0 and where either has no length.  The twist about the bone stays
    undetermined: two directions fix two of a rotation's three degrees of freedom, and the shortest arc picks the rotation
    without twist, so a mesh whose limbs are rolled about their own axes in its bind pose needs its own ``Q``."""
    g, off = _np(bind_joints, np.float64), _np(offsets, np.float64)
    parents, _ = pivots_of(skeleton)
    if g.shape != (len(parents), 3) or off.shape != g.shape:
        raise ValueError(f"bind_joints {g.shape} and offsets {off.shape} must be ({len(parents)}, 3)")
    Q = np.tile(np.eye(3), (len(parents), 1, 1))
    for c in range(1, len(parents)):
        u, v = off[c], g[c] - g[parents[c]]
        lu, lv = np.linalg.norm(u), np.linalg.norm(v)
        if lu > 0 and lv > 0:
            Q[c] = shortest_arc(u / lu, v / lv)
    return Q


def vertex_normals(vertices, faces):
    """Area-weighted vertex normals (V, 3) float32 of one mesh, on the host: the sum of the cross products of the faces at a
    vertex, normalised; zero where no face with area touches it."""
    v, f = _np(vertices, np.float64), _np(faces).astype(np.int64)
    if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
        raise ValueError(f"vertices {v.shape} must be (V, 3) and faces {f.shape} (F, 3)")
    cross = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    n = np.zeros_like(v)
    for k in range(3):
        np.add.at(n, f[:, k], cross)
    length = np.linalg.norm(n, axis=1, keepdims=True)
    return (n / np.where(length > 0, length, 1.0)).astype(np.float32)


def _capsule_template(segments, rings, sphere):
    """The tessellation that every capsule shares: per vertex (side, cos, sin, phi) -- the end it belongs to (0 parent, 1
    child), the polar angle from that end's pole and the angle around the axis -- and the faces, outward.  Poles first and
    last; ``rings`` rings per hemisphere down to the equator; a sphere drops the second equator."""
    S, Rg = int(segments), int(rings)
    rows = [(0, 0.0)] + [(0, 0.5 * np.pi * i / Rg) for i in range(1, Rg + 1)]
    rows += [(1, 0.5 * np.pi * i / Rg) for i in range(Rg - 1 if sphere else Rg, 0, -1)] + [(1, 0.0)]
    side, polar, phi, start = [], [], [], []
    for r, (sd, th) in enumerate(rows):
        n = 1 if r in (0, len(rows) - 1) else S
        start.append(len(side))
        side += [sd] * n
        polar += [th] * n
        phi += [2.0 * np.pi * k / S for k in range(n)]
    faces = []
    for r in range(len(rows) - 1):
        a, b = start[r], start[r + 1]
        for k in range(S):
            k1 = (k + 1) % S
            if r == 0:
                faces.append((a, b + k1, b + k))
            elif r == len(rows) - 2:
                faces.append((a + k, a + k1, b))
            else:
                faces += [(a + k, a + k1, b + k1), (a + k, b + k1, b + k)]
    return np.array(side), np.array(polar), np.array(phi), np.array(faces, np.int32)


def capsule_body(offsets, skeleton="t2m", radii=None, segments=12, rings=4, blend=0.25):
    """A body for users who bring none: one closed capsule per bone c >= 1 along its rest segment ``parent(c) -> c`` and a
    sphere at the root for bone 0.  ``offsets`` (J, 3) -> a ``Mesh``; (B, J, 3) -> one with per-sample ``vertices``, ``normals``
    and ``bind_joints`` (B, ...) and shared faces and weights.  ``radii``: per bone, in the offsets' units; default
    ``BODY_RADII[skeleton]`` times the height of the rest pose (its extent along Y).  ``segments`` (>= 3) vertices around a
    capsule, ``rings`` (>= 1) per hemisphere.  A vertex of capsule c at axial parameter s -- 0 at the parent end, 1 at the child
    end, below 0 on the parent's cap -- has weight ``max(0, (1 - max(s, 0) / blend) / 2)`` on bone ``parent(c)`` and the rest on
    bone c: at most two influences, and at the joint, where both bones put a point in the same place, half each.
    ``blend`` lies in (0, 1], a fraction of the bone.  The frame across the bone is ``motion_rig.across``; a bone without length
    gets a sphere about Y.  ``bind_joints`` is the rest pose of the offsets, ``bind_rotations`` None, the normals are the
    capsules' own.  Deterministic."""
    off = _np(offsets, np.float64)
    sk = get_skeleton(skeleton)
    J = int(sk.joints)
    if off.shape[-2:] != (J, 3) or off.ndim not in (2, 3) or not np.isfinite(off).all():
        raise ValueError(f"offsets of shape {off.shape} must be finite ({J}, 3) or (B, {J}, 3)")
    if int(segments) < 3 or int(rings) < 1 or not 0 < float(blend) <= 1:
        raise ValueError("segments must be >= 3, rings >= 1 and blend in (0, 1]")
    if radii is None:
        name = skeleton if isinstance(skeleton, str) else next((k for k in BODY_RADII if get_skeleton(k) is sk), None)
        if name not in BODY_RADII:
            raise ValueError("radii are required for a skeleton that BODY_RADII does not list")
        fractions = np.asarray(BODY_RADII[name], np.float64)
    else:
        fractions = None
        radii = _np(radii, np.float64)
        if radii.shape != (J,) or not (np.isfinite(radii).all() and (radii > 0).all()):
            raise ValueError(f"radii must be {J} positive numbers")
    parents, _ = pivots_of(sk)
    batch = off[None] if off.ndim == 2 else off
    rest = rest_pose(batch, sk)
    parts = [_capsule_template(segments, rings, sphere=True)] + [_capsule_template(segments, rings, sphere=False)] * (J - 1)
    verts, norms = [], []
    for b in range(len(batch)):
        r = radii if fractions is None else fractions * (rest[b, :, 1].max() - rest[b, :, 1].min())
        vb, nb = [], []
        for c, (side, polar, phi, _) in enumerate(parts):
            a, e = (rest[b, 0], rest[b, 0]) if c == 0 else (rest[b, parents[c]], rest[b, c])
            length = np.linalg.norm(e - a)
            u = (e - a) / length if length > 0 else np.array([0.0, 1.0, 0.0])
            e1 = across(u)
            e2 = np.cross(u, e1)
            sign = np.where(side == 0, -1.0, 1.0)
            n = (sign * np.cos(polar))[:, None] * u + (np.sin(polar) * np.cos(phi))[:, None] * e1 + \
                (np.sin(polar) * np.sin(phi))[:, None] * e2
            vb.append(np.where(side[:, None] == 0, a, e) + r[c] * n)
            nb.append(n)
        verts.append(np.concatenate(vb)), norms.append(np.concatenate(nb))
    faces, idx, w, base = [], [], [], 0
    for c, (side, polar, phi, f) in enumerate(parts):
        faces.append(f + base)
        base += len(side)
        # the same for every sample: max(s, 0) is 0 on the parent's cap and equator; the child's equator and cap have s >= 1 >=
        # blend, where the weight is 0 whatever s is, so 1 stands for it
        s = np.where(side == 0, 0.0, 1.0)
        wp = np.zeros(len(side)) if c == 0 else np.maximum(0.0, 0.5 * (1.0 - s / float(blend)))
        k, zero = len(side), np.zeros(len(side), int)
        idx.append(np.stack([np.full(k, c), np.full(k, parents[c] if c else 0), zero, zero], 1))
        w.append(np.stack([1.0 - wp, wp, np.zeros(len(side)), np.zeros(len(side))], 1))
    verts, norms = np.stack(verts), np.stack(norms)
    if off.ndim == 2:
        verts, norms, rest = verts[0], norms[0], rest[0]
    return Mesh(verts, np.concatenate(faces), np.concatenate(idx), np.concatenate(w), rest, None, norms, skeleton)


def check_skin(mesh, joints, rotations, lengths=None, return_normals=False):
    """Argument checks of ``skin_vertices`` that need no device: -> (joints (B, T, J, 3), rotations (B, T, J, 3, 3), lengths
    (B,) int64 or None).  Raises ValueError."""
    if not isinstance(mesh, Mesh):
        raise ValueError("mesh must be a motion_mesh.Mesh")
    J = int(get_skeleton(mesh.skeleton).joints)
    x, r = torch.as_tensor(joints), torch.as_tensor(rotations)
    if x.dim() == 3:
        x = x[None]
    if r.dim() == 4:
        r = r[None]
    if x.dim() != 4 or tuple(x.shape[2:]) != (J, 3):
        raise ValueError(f"joints of shape {tuple(x.shape)} must be (B, T, {J}, 3) for the mesh's skeleton")
    B, T = x.shape[:2]
    if tuple(r.shape) != (B, T, J, 3, 3):
        raise ValueError(f"rotations of shape {tuple(r.shape)} must be ({B}, {T}, {J}, 3, 3)")
    if T < 1:
        raise ValueError("a motion needs at least 1 frame")
    if mesh.batch is not None and mesh.batch != B:
        raise ValueError(f"the mesh holds {mesh.batch} per-sample bodies, the batch has {B} motions")
    if B * T * mesh.n_vertices * 3 >= 2 ** 40 or B > 65535:
        raise ValueError("the batch is too large for one launch")
    if lengths is not None:
        lengths = L.check_lengths(lengths, B, T)
    return x, r, lengths


@torch.no_grad()
def skin_vertices(mesh, joints, rotations, lengths=None, return_normals=False):
    """joints (B, T, J, 3) and global rotations (B, T, J, 3, 3) on a GPU, as ``motion_to_joints_fk(..., sigma=0,
    return_rotations=True)``, ``remove_foot_skate(..., rotations=)`` or ``pin_limbs(..., rotations=)`` return them -> the
    mesh's vertices under that motion, (B, T, V, 3) on the device, by linear blend skinning (the module's formula); with
    ``return_normals`` ``(vertices, normals)``, the normals turned with the bones and normalised (from the mesh's own, or
    ``vertex_normals`` of its bind pose).  Frames at or past a length are zero and are never read.  A mesh with per-sample
    bodies (``capsule_body`` of (B, J, 3) offsets) must hold one per motion.  No eager fallback: without a GPU this raises."""
    x, r, lengths = check_skin(mesh, joints, rotations, lengths, return_normals)
    L.require_cuda(x, r)
    dev = x.device
    if r.device != dev:
        raise ValueError("rotations must be on the joints' device")
    x, r = x.detach().to(torch.float32).contiguous(), r.detach().to(torch.float32).contiguous()
    B, T, J = x.shape[:3]
    if return_normals:
        mesh = mesh.with_normals()
    v, n, g, q, idx, w = mesh.on(dev)
    V = mesh.n_vertices
    ln = None if lengths is None else lengths.to(dev, torch.int32).contiguous()
    out = torch.empty(B, T, V, 3, device=dev)
    nout = torch.empty(B, T, V, 3, device=dev) if return_normals else None
    parents, _ = pivots_of(mesh.skeleton)
    parent = (C.c_int32 * J)(*parents)
    with torch.cuda.device(dev):
        L.check(L.lib().mdm_skin_vertices(
            x.data_ptr(), r.data_ptr(), L.ptr(ln), B, T, J, parent, v.data_ptr(), L.ptr(n if return_normals else None), V,
            int(v.dim() == 3), g.data_ptr(), int(g.dim() == 3), L.ptr(q), idx.data_ptr(), w.data_ptr(), out.data_ptr(),
            L.ptr(nout), L.stream_ptr()), "mdm_skin_vertices")
    return (out, nout) if return_normals else out


def skin_nodes(rig, skeleton):
    """Per bone the rig node that takes its weights in a glTF skin, or -1: the node that carries the bone's rotation
    (``carried[n] == c``) and sits at joint ``pivot(c)``; and per node the joint it sits at (a helper sits at its parent's)."""
    rig = rig_of(rig)
    _, pivots = pivots_of(skeleton)
    at = [j if j >= 0 else rig.joint_of[rig.parent[n]] for n, j in enumerate(rig.joint_of)]
    node = [-1] * len(pivots)
    for n, c in enumerate(rig.carried):
        if c >= 0 and node[c] < 0 and at[n] == pivots[c]:
            node[c] = n
    return node, at


def _pad4(b, fill):
    return b + fill * (-len(b) % 4)


def glb_bytes(mesh, rig, offsets, root, quaternions, n_frames, frame_time, scale=1.0):
    """One glTF 2.0 binary (``bytes``) of one sample: the mesh, its skin and the animation.  ``mesh``: a ``Mesh`` with (V, 3)
    vertices (``Mesh.sample`` of a per-sample one); ``rig``: ``rig_of``'s tree or a skeleton name; ``offsets`` (J, 3): the bone
    offsets the motion was generated on; ``root`` (T, 3) and ``quaternions`` (T, N, 4) as (w, x, y, z): the root positions and
    local rotations of ``rotations_to_rig(..., return_quaternions=True)`` at scale 1, of which the first ``n_frames`` (>= 1) are
    written, ``frame_time`` seconds apart; ``scale``: of every length (100 for centimetres).

    Nodes: the N nodes of the rig in its order, each with the translation ``scale * offset[joint_of]`` where ``has_offset``
    (the root: its first key), and a mesh node that carries the skin.  ``skin.joints`` lists all N nodes; bone c's weights go
    to ``skin_nodes``' node, which sits at joint ``pivot(c)`` and carries ``R[c]`` (ValueError where a weighted bone has none);
    ``inverseBindMatrices`` is ``(T(scale G[joint at node]) Q[carried])^-1``, column-major.  The primitive holds POSITION
    (``scale * vertices``, with min / max), NORMAL, JOINTS_0 (unsigned byte), WEIGHTS_0 (float) and uint32 indices.  The
    animation: one input of times ``k * frame_time``, a translation channel on the root (``scale * root``) and one rotation
    channel per node, keys reordered to (x, y, z, w) and negated where the dot product with the key before is negative (the
    same rotation), so that LINEAR players go the short way.  Container: 12-byte header, a JSON chunk padded with spaces, a BIN
    chunk padded with zeros, every bufferView 4-byte aligned."""
    rig = rig_of(rig)
    N, J = rig.n_nodes, rig.joints
    if not isinstance(mesh, Mesh) or mesh.batch is not None:
        raise ValueError("glb_bytes takes a Mesh with (V, 3) vertices: Mesh.sample(b) of a per-sample one")
    if int(get_skeleton(mesh.skeleton).joints) != J:
        raise ValueError(f"the mesh's skeleton has {get_skeleton(mesh.skeleton).joints} joints, the rig {J}")
    mesh = mesh.with_normals()
    off = _np(offsets, np.float64)
    if off.shape != (J, 3):
        raise ValueError(f"offsets of shape {off.shape} must be ({J}, 3)")
    pos, quat = _np(root, np.float32), _np(quaternions, np.float32)
    n_frames = int(n_frames)
    if pos.ndim != 2 or pos.shape[1] != 3 or quat.shape != (pos.shape[0], N, 4):
        raise ValueError(f"root {pos.shape} must be (T, 3) and quaternions {quat.shape} (T, {N}, 4)")
    if not 1 <= n_frames <= pos.shape[0]:
        raise ValueError(f"n_frames must lie in [1, {pos.shape[0]}]")
    if not (np.isfinite(float(frame_time)) and float(frame_time) > 0 and np.isfinite(float(scale))):
        raise ValueError("frame_time must be > 0 and scale finite")
    node_of, at = skin_nodes(rig, mesh.skeleton)
    live = mesh.bone_weight > 0
    orphans = sorted({int(c) for c in mesh.bone_index[live] if node_of[c] < 0})
    if orphans:
        raise ValueError(f"the bones {orphans} carry weights but no rig node sits at their pivot and carries their rotation")
    sc = np.float32(scale)
    G = mesh.bind_joints.astype(np.float64)
    ibm = np.zeros((N, 4, 4))
    for n in range(N):
        c = rig.carried[n]
        Q = np.eye(3) if mesh.bind_rotations is None or c < 0 else mesh.bind_rotations[c].astype(np.float64)
        ibm[n, :3, :3], ibm[n, :3, 3], ibm[n, 3, 3] = Q.T, -Q.T @ (float(scale) * G[at[n]]), 1.0  # (T(s g) Q)^-1 = Q^T T(-s g)
    joints0 = np.where(live, np.asarray(node_of)[mesh.bone_index], 0).astype(np.uint8)
    keys = quat[:n_frames][:, :, [1, 2, 3, 0]].copy()
    for k in range(1, n_frames):  # against the key as written, so a flip carries on
        flip = (keys[k] * keys[k - 1]).sum(-1) < 0
        keys[k][flip] = -keys[k][flip]
    times = (np.arange(n_frames, dtype=np.float64) * float(frame_time)).astype(np.float32)
    position = sc * mesh.vertices
    blobs, views, accessors = [], [], []

    def add(array, kind, component, target=None, bounds=False, count=None, split=1):
        """One bufferView of ``array``'s bytes, and ``split`` accessors that share it in equal parts -> the first's index."""
        data = np.ascontiguousarray(array).tobytes()
        start = sum(len(b) for b in blobs)
        blobs.append(_pad4(data, b"\0"))
        view = dict(buffer=0, byteOffset=start, byteLength=len(data))
        if target is not None:
            view["target"] = target
        views.append(view)
        count = (len(array) if count is None else count)
        for part in range(split):
            acc = dict(bufferView=len(views) - 1, byteOffset=part * (len(data) // split), componentType=component, count=count,
                       type=kind)
            if bounds:
                flat = np.asarray(array).reshape(len(array), -1)
                acc["min"], acc["max"] = [float(x) for x in flat.min(0)], [float(x) for x in flat.max(0)]
            accessors.append(acc)
        return len(accessors) - split

    FLOAT, UBYTE, UINT = 5126, 5121, 5125
    a_pos = add(position, "VEC3", FLOAT, 34962, bounds=True)
    a_nrm = add(mesh.normals, "VEC3", FLOAT, 34962)
    a_jnt = add(joints0, "VEC4", UBYTE, 34962)
    a_wgt = add(mesh.bone_weight, "VEC4", FLOAT, 34962)
    a_idx = add(mesh.faces.astype(np.uint32).reshape(-1), "SCALAR", UINT, 34963)
    a_ibm = add(np.ascontiguousarray(ibm.transpose(0, 2, 1)).astype(np.float32).reshape(N, 16), "MAT4", FLOAT)
    a_time = add(times, "SCALAR", FLOAT, bounds=True)
    a_root = add(sc * pos[:n_frames], "VEC3", FLOAT)
    a_rot = add(np.ascontiguousarray(keys.transpose(1, 0, 2)).reshape(N * n_frames, 4), "VEC4", FLOAT, count=n_frames, split=N)
    kids = [[] for _ in range(N)]
    for n in range(1, N):
        kids[rig.parent[n]].append(n)
    nodes = []
    for n in range(N):
        node = dict(name=rig.names[n])
        if n == 0:
            node["translation"] = [float(x) for x in sc * pos[0]]
        elif rig.has_offset[n]:
            node["translation"] = [float(x) for x in (float(scale) * off[rig.joint_of[n]]).astype(np.float32)]
        node["rotation"] = [float(x) for x in keys[0, n]]
        if kids[n]:
            node["children"] = kids[n]
        nodes.append(node)
    nodes.append(dict(name="body", mesh=0, skin=0))
    samplers = [dict(input=a_time, output=a_root, interpolation="LINEAR")]
    channels = [dict(sampler=0, target=dict(node=0, path="translation"))]
    for n in range(N):
        samplers.append(dict(input=a_time, output=a_rot + n, interpolation="LINEAR"))
        channels.append(dict(sampler=n + 1, target=dict(node=n, path="rotation")))
    binary = b"".join(blobs)
    doc = dict(
        asset=dict(version="2.0", generator="motiondiffusion-moe_amd motion_mesh"), scene=0, scenes=[dict(nodes=[0, N])],
        nodes=nodes,
        meshes=[dict(primitives=[dict(attributes=dict(POSITION=a_pos, NORMAL=a_nrm, JOINTS_0=a_jnt, WEIGHTS_0=a_wgt),
                                      indices=a_idx, mode=4)])],
        skins=[dict(joints=list(range(N)), inverseBindMatrices=a_ibm, skeleton=0)],
        animations=[dict(name="motion", samplers=samplers, channels=channels)],
        accessors=accessors, bufferViews=views, buffers=[dict(byteLength=len(binary))])
    text = _pad4(json.dumps(doc, separators=(",", ":")).encode("ascii"), b" ")
    total = 12 + 8 + len(text) + 8 + len(binary)
    return b"".join([struct.pack("<4sII", b"glTF", 2, total), struct.pack("<I4s", len(text), b"JSON"), text,
                     struct.pack("<I4s", len(binary), b"BIN\0"), binary])


def write_glb(path, mesh, rig, offsets, root, quaternions, n_frames, frame_time, scale=1.0):
    """``glb_bytes`` written to ``path``; returns the bytes."""
    data = glb_bytes(mesh, rig, offsets, root, quaternions, n_frames, frame_time, scale)
    with open(path, "wb") as f:
        f.write(data)
    return data


def write_obj(path, vertices, faces, normals=None):
    """One frame as a Wavefront OBJ, for a quick look: ``vertices`` (V, 3), ``faces`` (F, 3) from 0, ``normals`` (V, 3) or
    None.  Returns the text."""
    v, f = _np(vertices, np.float64), _np(faces).astype(np.int64)
    if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
        raise ValueError(f"vertices {v.shape} must be (V, 3) and faces {f.shape} (F, 3)")
    lines = ["v %.9g %.9g %.9g" % tuple(p) for p in v.tolist()]
    if normals is not None:
        n = _np(normals, np.float64)
        if n.shape != v.shape:
            raise ValueError(f"normals of shape {n.shape} must be {v.shape}")
        lines += ["vn %.9g %.9g %.9g" % tuple(p) for p in n.tolist()]
        lines += ["f %d//%d %d//%d %d//%d" % (a, a, b, b, c, c) for a, b, c in (f + 1).tolist()]
    else:
        lines += ["f %d %d %d" % tuple(t) for t in (f + 1).tolist()]
    text = "\n".join(lines) + "\n"
    with open(path, "w") as out:
        out.write(text)
    return text

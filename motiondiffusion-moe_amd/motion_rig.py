"""Rig export: the joints and global rotations of ``postprocess.motion_to_joints_fk`` /
``remove_foot_skate`` -> a node tree with Euler channels at the frame rate a tool works at -> BVH text.

``R[c]`` of the forward kinematics orients the bone ``parent(c) -> c`` and every chain starts from the root matrix, so a joint
with several children (pelvis, spine3) has a different rotation for each outgoing bone: loaded into a skeleton as "the joint's
global rotation" it gives a broken pose.  ``rig_of`` builds the node tree in which it is one: zero-offset helper nodes below
every branching joint (the ``LHipJoint`` / ``LowerBack`` nodes of the CMU files), one per outgoing bone.  On that tree the
existing rotations are a lossless animation, no IK fit.  The arithmetic (local rotations, quaternions, slerp retiming, Euler
angles) is in ``mdm_rig_channels`` (csrc/motion_rig.hip); no eager fallback.  ``bvh_text`` / ``write_bvh`` are host code that
prints numbers and does no arithmetic on the motion."""
from __future__ import annotations

import ctypes as C
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib as L

MAX_NODES = 64  # of mdm_rig_channels
EULER_ORDERS = ("XYZ", "XZY", "YXZ", "YZX", "ZXY", "ZYX")
DEFAULT_FPS = {"t2m": 20.0, "kit": 12.5}


def rig_of(skeleton):
    """The node tree of a skeleton ("t2m", "kit" or a skeleton namespace of ``motion_features``): a namespace of ``names``,
    ``parent`` (node index, -1 at the root; parents come first), ``carried`` (the joint whose ``R`` is the node's global
    rotation, or -1: the node turns with its parent), ``joint_of`` (the joint that sits at the node, or -1 for a helper),
    ``has_offset`` (the node's OFFSET is ``offset[joint_of]``; zero for the root and the helpers), ``joints`` and ``n_nodes``.
    Depth-first in chain order.  A joint with one child carries the child's ``R``; one with several carries its own and gets a
    zero-offset helper ``"<p>_to_<c>"`` per child that carries the child's; a leaf carries nothing.  Raises ValueError for a
    skeleton that needs more than ``MAX_NODES`` nodes."""
    if isinstance(skeleton, SimpleNamespace) and hasattr(skeleton, "joint_of"):
        return skeleton
    from .motion_edit import SMPL_JOINTS
    from .motion_features import SKELETONS, get_skeleton
    sk = get_skeleton(skeleton)
    J = int(sk.joints)
    children = [[] for _ in range(J)]
    for chain in sk.chains:
        for a, b in zip(chain[:-1], chain[1:]):
            if b not in children[a]:
                children[a].append(b)
    if sorted(c for cs in children for c in cs) != list(range(1, J)):
        raise ValueError("the skeleton's chains must reach every joint but the root exactly once")
    n_nodes = J + sum(len(cs) for cs in children if len(cs) > 1)
    if n_nodes > MAX_NODES:
        raise ValueError(f"the skeleton needs {n_nodes} rig nodes: at most {MAX_NODES}")
    jname = getattr(sk, "names", None) or (SMPL_JOINTS if sk is SKELETONS["t2m"] else [f"joint_{j:02d}" for j in range(J)])
    rig = SimpleNamespace(names=[], parent=[], carried=[], joint_of=[], has_offset=[], joints=J, n_nodes=n_nodes)

    def add(name, parent, carried, joint, has_offset):
        for k, v in (("names", name), ("parent", parent), ("carried", carried), ("joint_of", joint), ("has_offset", has_offset)):
            getattr(rig, k).append(v)
        return len(rig.names) - 1

    def walk(p, above):
        cs = children[p]
        node = add(jname[p], above, cs[0] if len(cs) == 1 else (p if cs else -1), p, above >= 0)
        for c in cs:
            walk(c, add(f"{jname[p]}_to_{jname[c]}", node, c, -1, False) if len(cs) > 1 else node)

    walk(0, -1)
    return rig


def _axes(euler):
    if not isinstance(euler, str) or euler.upper() not in EULER_ORDERS:
        raise ValueError(f"euler must be one of {EULER_ORDERS}, not {euler!r}")
    return tuple("XYZ".index(ch) for ch in euler.upper())


def retime_ratio(skeleton, fps=None, fps_out=None):
    """-> (num, den, fps) with output frame k at source frame k den / num: ``Fraction(fps_out).limit_denominator(1000) /
    Fraction(fps).limit_denominator(1000)``.  ``fps`` defaults by skeleton name (t2m 20, KIT 12.5); without ``fps_out`` 1 / 1."""
    if fps is None and isinstance(skeleton, str):
        fps = DEFAULT_FPS.get(skeleton)
    if fps is not None and not (np.isfinite(float(fps)) and float(fps) > 0):
        raise ValueError("fps must be > 0")
    if fps_out is None:
        return 1, 1, fps
    if not (np.isfinite(float(fps_out)) and float(fps_out) > 0):
        raise ValueError("fps_out must be > 0")
    if fps is None:
        raise ValueError("fps is required with fps_out for a skeleton that has no default frame rate")
    src, dst = Fraction(float(fps)).limit_denominator(1000), Fraction(float(fps_out)).limit_denominator(1000)
    if src <= 0 or dst <= 0:
        raise ValueError("fps and fps_out must be at least 0.001")
    r = dst / src
    return r.numerator, r.denominator, fps


def check_rig(joints, rotations, lengths, skeleton, euler="ZXY", fps=None, fps_out=None, scale=1.0):
    """Argument checks of ``rotations_to_rig`` that need no device: -> (joints (B, T, J, 3), rotations (B, T, J, 3, 3), lengths
    (B,) int64 or None, rig, the three axis indices, num, den, lengths_out (B,) int64).  Raises ValueError."""
    rig = rig_of(skeleton)
    J = rig.joints
    axes = _axes(euler)
    x, r = torch.as_tensor(joints), torch.as_tensor(rotations)
    if x.dim() == 3:
        x = x[None]
    if r.dim() == 4:
        r = r[None]
    if x.dim() != 4 or tuple(x.shape[2:]) != (J, 3):
        raise ValueError(f"joints of shape {tuple(x.shape)} must be (B, T, {J}, 3) for this skeleton")
    B, T = x.shape[:2]
    if tuple(r.shape) != (B, T, J, 3, 3):
        raise ValueError(f"rotations of shape {tuple(r.shape)} must be ({B}, {T}, {J}, 3, 3)")
    if T < 1:
        raise ValueError("a motion needs at least 1 frame")
    if not np.isfinite(float(scale)):
        raise ValueError("scale must be finite")
    num, den, _ = retime_ratio(skeleton, fps, fps_out)
    if lengths is not None:
        lengths = torch.as_tensor(lengths).flatten().to(torch.int64).cpu()
        if lengths.numel() != B:
            raise ValueError(f"lengths must have {B} entries")
        if B and (int(lengths.min()) < 1 or int(lengths.max()) > T):
            raise ValueError(f"every length must lie in [1, {T}]")
    n = torch.full((B,), T, dtype=torch.int64) if lengths is None else lengths
    lengths_out = (n - 1) * num // den + 1
    if B and int(lengths_out.max()) * (3 + 3 * rig.n_nodes) >= 2 ** 31:
        raise ValueError("the retimed motion is too long")
    return x, r, lengths, rig, axes, num, den, lengths_out


@torch.no_grad()
def rotations_to_rig(joints, rotations, lengths=None, *, skeleton="t2m", euler="ZXY", fps=None, fps_out=None, scale=1.0,
                     return_quaternions=False):
    """joints (B, T, J, 3) and global rotations (B, T, J, 3, 3) on a GPU, as ``motion_to_joints_fk(..., sigma=0,
    return_rotations=True)`` or ``remove_foot_skate(..., rotations=)`` return them -> ``(channels (B, T_out, 3 + 3 N),
    lengths_out (B,))`` for the N nodes of ``rig_of(skeleton)``: the root's X Y Z times ``scale``, then three angles in degrees
    per node in node order, of ``L = R_A(a) R_B(b) R_C(c)`` for ``euler`` "ABC", which is what a BVH reader computes from
    ``CHANNELS Arotation Brotation Crotation``.  ``fps_out``: retimed from ``fps`` (default 20 for "t2m", 12.5 for "kit") by
    slerp of the local rotations and lerp of the root, ``lengths_out = (length - 1) num // den + 1`` with ``num / den`` of
    ``retime_ratio``; frames at or past it are zero.  ``return_quaternions``: also the local unit quaternions
    (B, T_out, N, 4) as (w, x, y, z), w >= 0."""
    x, r, lengths, rig, axes, num, den, lengths_out = check_rig(joints, rotations, lengths, skeleton, euler, fps, fps_out, scale)
    L.require_cuda(x, r)
    dev = x.device
    if r.device != dev:
        raise ValueError("rotations must be on the joints' device")
    x, r = x.detach().to(torch.float32).contiguous(), r.detach().to(torch.float32).contiguous()
    B, T, J = x.shape[:3]
    N = rig.n_nodes
    T_out = int(lengths_out.max()) if B else 1
    ln = None if lengths is None else lengths.to(dev, torch.int32).contiguous()
    ln_out = lengths_out.to(dev, torch.int32).contiguous()
    chan = torch.empty(B, T_out, 3 + 3 * N, device=dev)
    quat = torch.empty(B, T_out, N, 4, device=dev) if return_quaternions else None
    parent, carried = (C.c_int32 * N)(*rig.parent), (C.c_int32 * N)(*rig.carried)
    with torch.cuda.device(dev):
        L.check(L.lib().mdm_rig_channels(
            x.data_ptr(), r.data_ptr(), L.ptr(ln), B, T, J, N, parent, carried, axes[0], axes[1], axes[2], float(scale), num, den,
            T_out, ln_out.data_ptr(), chan.data_ptr(), L.ptr(quat), L.stream_ptr()), "mdm_rig_channels")
    return (chan, lengths_out, quat) if return_quaternions else (chan, lengths_out)


def bvh_text(rig, offsets, channels, n_frames, frame_time, *, euler="ZXY", scale=1.0, end_site=0.05):
    """The BVH file of one sample as a ``str``.  ``rig``: ``rig_of``'s tree (or a skeleton name); ``offsets`` (J, 3) bone
    offsets; ``channels`` (T, 3 + 3 N) from ``rotations_to_rig`` with the same ``euler`` and ``scale``, of which the first
    ``n_frames`` rows are written; ``frame_time`` in seconds.  HIERARCHY: every node with ``scale * offset`` of its joint
    (zero at the root and the helpers) and ``CHANNELS`` in the Euler order, the root's led by its position; a leaf gets an
    End Site that continues its own bone for ``end_site * scale``, or (0, end_site * scale, 0) where that bone is zero.
    Numbers, offsets included, are printed with ``%.9g`` (``%.17g`` for float64 channels): parsed back to the channels' dtype
    they are the channels bit for bit."""
    rig = rig_of(rig)
    axes = _axes(euler)
    N = rig.n_nodes
    ch = channels.detach().cpu().numpy() if torch.is_tensor(channels) else np.asarray(channels)
    if ch.dtype not in (np.float32, np.float64):
        ch = ch.astype(np.float32)
    if ch.ndim != 2 or ch.shape[1] != 3 + 3 * N:
        raise ValueError(f"channels of shape {ch.shape} must be (T, {3 + 3 * N}) for this rig")
    n_frames = int(n_frames)
    if not 0 <= n_frames <= ch.shape[0]:
        raise ValueError(f"n_frames must lie in [0, {ch.shape[0]}]")
    if not (np.isfinite(float(frame_time)) and float(frame_time) > 0):
        raise ValueError("frame_time must be > 0")
    off = (offsets.detach().cpu().numpy() if torch.is_tensor(offsets) else np.asarray(offsets)).astype(np.float64)
    if off.shape != (rig.joints, 3):
        raise ValueError(f"offsets of shape {off.shape} must be ({rig.joints}, 3)")
    fmt = "%.17g" if ch.dtype == np.float64 else "%.9g"
    off = float(scale) * off
    reach = float(end_site) * float(scale)
    kids = [[] for _ in range(N)]
    for n in range(1, N):
        kids[rig.parent[n]].append(n)
    rot = " ".join("XYZ"[a] + "rotation" for a in axes)
    out = ["HIERARCHY"]

    def vec(v):
        return " ".join(fmt % float(e) for e in v)

    def node(n, depth):
        pad = "  " * depth
        o = off[rig.joint_of[n]] if rig.has_offset[n] else np.zeros(3)
        out.append(f"{pad}{'ROOT' if n == 0 else 'JOINT'} {rig.names[n]}")
        out.append(pad + "{")
        out.append(f"{pad}  OFFSET {vec(o)}")
        out.append(f"{pad}  CHANNELS 6 Xposition Yposition Zposition {rot}" if n == 0 else f"{pad}  CHANNELS 3 {rot}")
        for k in kids[n]:
            node(k, depth + 1)
        if not kids[n]:
            length = float(np.linalg.norm(o))
            end = o / length * reach if length > 0 else np.array([0.0, reach, 0.0])
            out.extend([f"{pad}  End Site", pad + "  {", f"{pad}    OFFSET {vec(end)}", pad + "  }"])
        out.append(pad + "}")

    node(0, 0)
    out.extend(["MOTION", f"Frames: {n_frames}", "Frame Time: %.9g" % float(frame_time)])
    out.extend(" ".join([fmt % v for v in row]) for row in ch[:n_frames].tolist())
    return "\n".join(out) + "\n"


def write_bvh(path, rig, offsets, channels, n_frames, frame_time, **kw):
    """``bvh_text`` written to ``path``; returns the text."""
    text = bvh_text(rig, offsets, channels, n_frames, frame_time, **kw)
    with open(path, "w") as f:
        f.write(text)
    return text

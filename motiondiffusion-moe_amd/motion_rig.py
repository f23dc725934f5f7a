"""Rig export: the joints and global rotations of ``postprocess.motion_to_joints_fk`` /
``remove_foot_skate`` -> a node tree with Euler channels at the frame rate a tool works at -> BVH text.

``R[c]`` of the forward kinematics orients the bone ``parent(c) -> c`` and every chain starts from the root matrix, so a joint
with several children (pelvis, spine3) has a different rotation for each outgoing bone: loaded into a skeleton as "the joint's
global rotation" it gives a broken pose.  ``rig_of`` builds the node tree in which it is one: zero-offset helper nodes below
every branching joint (the ``LHipJoint`` / ``LowerBack`` nodes of the CMU files), one per outgoing bone.  On that tree the
existing rotations are a lossless animation, no IK fit.  The arithmetic (local rotations, quaternions, slerp retiming, Euler
angles) is in ``mdm_rig_channels`` (csrc/motion_rig.hip); no eager fallback.  ``bvh_text`` / ``write_bvh`` are host code that
prints numbers and does no arithmetic on the motion.

Rig import is the way back, for any hierarchy: ``parse_bvh`` / ``read_bvh`` (host, no arithmetic) ->
``resolve_joint_map`` (which node stands for which joint: ``JOINT_MAPS``) -> ``bvh_to_joints``, whose arithmetic (local
rotations from the channels, slerp retiming, the walk from a node up to the root) is in ``mdm_rig_joints``
(csrc/motion_rig_import.hip); ``bvh_to_motion`` goes on to feature rows.  No eager fallback either.

Rig retargeting writes a motion onto a given hierarchy, a character's own: ``target_rig`` (host, float64: which
node copies which bone's rotation with which rest-pose correction, which is fitted, the legs) -> ``retarget_to_rig``, whose
arithmetic is in ``mdm_retarget_channels`` (csrc/motion_retarget.hip) -> ``target_bvh_text``.  No eager fallback either."""
from __future__ import annotations

import ctypes as C
import os
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib as L

MAX_NODES = 64  # of mdm_rig_channels
EULER_ORDERS = ("XYZ", "XZY", "YXZ", "YZX", "ZXY", "ZYX")
DEFAULT_FPS = {"t2m": 20.0, "kit": 12.5}
MAX_IMPORT_NODES = 128  # of mdm_rig_joints


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
        lengths = L.check_lengths(lengths, B, T)
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


# ---- rig import ----

_KEYWORDS = ("ROOT", "JOINT", "END", "{", "}", "OFFSET", "CHANNELS", "MOTION")
_CHANNELS = {a.lower() + k: (a + k, i, k == "rotation") for i, a in enumerate("XYZ") for k in ("position", "rotation")}


def parse_bvh(text):
    """BVH text -> a namespace: ``names``, ``parent`` (node index, -1 at the root; parents come first), ``offsets`` (N, 3)
    float64, ``channels`` (per node its channel names, spelled ``Xposition`` ... ``Zrotation``), ``end_sites`` {node: offset},
    ``rot_col`` / ``rot_axis`` (N, 3) int32: per node the column of ``values`` and the axis (0 / 1 / 2) of each rotation
    channel in the order the file lists them, column -1 (axis 0) where the node has fewer than three; ``pos_col`` (3,): the
    columns of the root's X, Y, Z position, or -1; ``frames``, ``frame_time`` and ``values`` (frames, C) float32.  Host code
    that reads numbers and does no arithmetic on the motion.

    A node has 0 to 3 rotation channels, on any axes and in its own order.  Position channels on a node other than the root
    count towards the column numbering and are otherwise ignored: the node's OFFSET is used and bones stay rigid (files that
    write six channels per joint repeat the offset there).  An ``End Site`` owns no channels.  Any whitespace, CRLF line ends,
    keywords in any letter case, names with ``:`` and a missing final newline are taken; the hierarchy is read token by token
    (a CHANNELS list may wrap), a MOTION row is a line.  Raises ValueError, with the line number, for a second ROOT, a CHANNELS count that disagrees
    with its list, an unknown channel name, more than 3 rotation channels on a node, a MOTION row of the wrong width, a row
    count other than ``Frames:``, a number that does not parse or is not finite, ``Frame Time`` <= 0, more than
    ``MAX_IMPORT_NODES`` nodes, and a hierarchy that does not parse."""
    lines = text.splitlines()
    toks = [(w, i + 1, k == len(ws) - 1) for i, ws in enumerate(ln.split() for ln in lines) for k, w in enumerate(ws)]
    pos = 0

    def bad(line, what):
        return ValueError(f"BVH line {line}: {what}")

    def take(what):
        nonlocal pos
        if pos >= len(toks):
            raise bad(len(lines), f"the text ends where {what} is expected")
        pos += 1
        return toks[pos - 1]

    def number(what, kind=float):
        w, line, _ = take(what)
        try:
            v = kind(w)
        except ValueError:
            raise bad(line, f"{w!r} is not {what}") from None
        if not np.isfinite(v):
            raise bad(line, f"{what} {w!r} is not finite")
        return v, line

    w, line, _ = take("HIERARCHY")
    if w.upper() != "HIERARCHY":
        raise bad(line, f"HIERARCHY expected, not {w!r}")
    names, parent, offsets, channels, ends, rot_col, rot_axis = [], [], [], [], {}, [], []
    pos_col, stack, pending, width, listed = [-1, -1, -1], [], None, 0, set()
    while True:
        w, line, last = take("MOTION")
        key = w.upper()
        if key == "MOTION":
            break
        if key in ("ROOT", "JOINT"):
            if key == "ROOT" and names:
                raise bad(line, "a second ROOT")
            if key == "JOINT" and not stack:
                raise bad(line, "JOINT outside the ROOT")
            if pending is not None or (stack and stack[-1] == "end"):
                raise bad(line, f"{w!r} where a node cannot start")
            if len(names) == MAX_IMPORT_NODES:
                raise bad(line, f"more than {MAX_IMPORT_NODES} nodes")
            names.append(take("a node's name")[0]), parent.append(stack[-1] if stack else -1), offsets.append(None)
            channels.append([]), rot_col.append([-1, -1, -1]), rot_axis.append([0, 0, 0])
            pending = len(names) - 1
        elif key == "END":
            if take("Site")[0].upper() != "SITE" or not stack or stack[-1] == "end" or pending is not None:
                raise bad(line, "a misplaced End Site")
            pending = "end"
        elif key == "{":
            if pending is None:
                raise bad(line, "'{' without a node")
            stack.append(pending)
            pending = None
        elif key == "}":
            if not stack or pending is not None:
                raise bad(line, "'}' without its '{'")
            if stack[-1] != "end" and offsets[stack[-1]] is None:
                raise bad(line, f"node {names[stack[-1]]!r} has no OFFSET")
            stack.pop()
        elif key == "OFFSET":
            if not stack or pending is not None:
                raise bad(line, "OFFSET outside a node")
            v = np.array([number("an offset")[0] for _ in range(3)], np.float64)
            if stack[-1] == "end":
                ends[stack[-2]] = v
            else:
                offsets[stack[-1]] = v
        elif key == "CHANNELS":
            if not stack or stack[-1] == "end" or pending is not None or stack[-1] in listed:
                raise bad(line, "CHANNELS outside a node, in an End Site or given twice")
            node = stack[-1]
            listed.add(node)
            count = number("a channel count", int)[0]
            while pos < len(toks) and (len(channels[node]) < count or toks[pos][0].lower() in _CHANNELS):
                c = toks[pos][0]
                if c.lower() not in _CHANNELS:  # the list is over before its count: a keyword, or a name that is no channel
                    if c.upper() in _KEYWORDS:
                        break
                    raise bad(toks[pos][1], f"unknown channel {c!r}")
                pos += 1
                name, axis, turns = _CHANNELS[c.lower()]
                if turns:
                    k = sum(col >= 0 for col in rot_col[node])
                    if k == 3:
                        raise bad(line, f"more than 3 rotation channels on node {names[node]!r}")
                    rot_col[node][k], rot_axis[node][k] = width, axis
                elif node == 0:
                    pos_col[axis] = width
                channels[node].append(name)
                width += 1
            if len(channels[node]) != count:
                raise bad(line, f"CHANNELS {count} lists {len(channels[node])} channels")
        else:
            raise bad(line, f"unexpected {w!r} in the hierarchy")
    if stack or pending is not None or not names:
        raise bad(line, "MOTION inside an open node" if names else "MOTION before a ROOT")
    w, line, _ = take("Frames:")
    if w.upper() != "FRAMES:":
        raise bad(line, f"Frames: expected, not {w!r}")
    frames, line = number("a frame count", int)
    if frames < 0:
        raise bad(line, "a negative frame count")
    w, line, _ = take("Frame Time:")
    if w.upper() != "FRAME" or take("Time:")[0].upper() != "TIME:":
        raise bad(line, "Frame Time: expected")
    frame_time, line = number("a frame time")
    if not frame_time > 0:
        raise bad(line, "Frame Time must be > 0")
    values = np.zeros((frames, width), np.float32)
    n = 0
    for i in range(line, len(lines)):  # a row is a line
        ws = lines[i].split()
        if not ws:
            continue
        if n == frames:
            raise bad(i + 1, f"more rows than Frames: {frames}")
        try:
            row = np.array(ws, dtype=np.float64)
        except ValueError:
            raise bad(i + 1, "a MOTION row holds something that is not a number") from None
        if len(row) != width:
            raise bad(i + 1, f"a MOTION row of {len(row)} numbers, the hierarchy has {width} channels")
        if not np.isfinite(row).all():
            raise bad(i + 1, "a MOTION row holds a number that is not finite")
        values[n] = row
        n += 1
    if n != frames:
        raise bad(len(lines), f"{n} MOTION rows, Frames: says {frames}")
    return SimpleNamespace(names=names, parent=parent, offsets=np.stack(offsets), channels=channels, end_sites=ends,
                           rot_col=np.array(rot_col, np.int32), rot_axis=np.array(rot_axis, np.int32),
                           pos_col=np.array(pos_col, np.int32), frames=frames, frame_time=frame_time, values=values)


def read_bvh(path):
    """``parse_bvh`` of the file at ``path``."""
    with open(path, newline="") as f:
        return parse_bvh(f.read())


def _cmu(side):
    return [side + n for n in ("UpLeg", "Leg", "Foot", "ToeBase", "Shoulder", "Arm", "ForeArm", "Hand")]


def _humanoid(spine):
    """The 22 joints in ``SMPL_JOINTS`` order on the Left / Right naming that the CMU and the Mixamo files share."""
    l, r = _cmu("Left"), _cmu("Right")
    return ("Hips", l[0], r[0], spine[0], l[1], r[1], spine[1], l[2], r[2], spine[2], l[3], r[3], spine[3], l[4], r[4],
            spine[4], l[5], r[5], l[6], r[6], l[7], r[7])


def _smpl_names():
    from .motion_edit import SMPL_JOINTS
    return tuple(SMPL_JOINTS)


# Per preset, the node at which each joint sits, in joint order: "smpl" and "kit" are the names ``rig_of`` gives its own export
# (22 HumanML3D joints / 21 KIT joints); "cmu" and "mixamo" place the 22 HumanML3D joints on those files' nodes.  ``X/End`` is
# the End Site of node X.  The CMU files have LowerBack, Neck and the Shoulder nodes at zero offset below Hips and Spine1 (as
# ``rig_of`` has its helpers), so their spine has five distinct node positions for the six joints pelvis .. head: the preset
# takes Spine, Spine1, Neck1, Head and Head's End Site, which leaves no bone of the skeleton without length (the collars, at
# Spine1's position, hang off spine3 at Neck1).
JOINT_MAPS = {
    "smpl": _smpl_names(),
    "kit": tuple(f"joint_{j:02d}" for j in range(21)),
    "cmu": _humanoid(("Spine", "Spine1", "Neck1", "Head", "Head/End")),
    "mixamo": _humanoid(("Spine", "Spine1", "Spine2", "Neck", "Head")),
}


def _bare(name):
    return str(name).rsplit(":", 1)[-1].lower()


def resolve_joint_map(bvh, joint_map=None):
    """-> per joint the index of the node of ``bvh`` (``parse_bvh``'s namespace) it sits at; ``N + n`` stands for the End Site
    of node n, named ``<node>/End``.  Names match without letter case and with anything up to the last ``:`` stripped
    (``mixamorig:Hips`` is ``hips``); of nodes that then share a name the first counts.  ``joint_map``: None (the first preset
    of ``JOINT_MAPS`` whose names are all present), a preset's name, a sequence of node names in joint order, or a dict from
    joint index or HumanML3D joint name to node name that covers the joints 0 .. J - 1.  Raises ValueError listing the names
    that the file lacks."""
    at, N = {}, len(bvh.names)
    for n, name in enumerate(bvh.names):
        at.setdefault(_bare(name), n)
    for n in getattr(bvh, "end_sites", {}):
        at.setdefault(_bare(bvh.names[n]) + "/end", N + n)
    if joint_map is None:
        for wanted in JOINT_MAPS.values():
            if all(_bare(w) in at for w in wanted):
                return [at[_bare(w)] for w in wanted]
        lacks = {k: [w for w in wanted if _bare(w) not in at] for k, wanted in JOINT_MAPS.items()}
        raise ValueError("no preset of JOINT_MAPS fits the file's nodes: " + "; ".join(f"{k!r} lacks {v}" for k, v in lacks.items()))
    if isinstance(joint_map, str):
        if joint_map not in JOINT_MAPS:
            raise ValueError(f"joint_map must be one of {sorted(JOINT_MAPS)}, a sequence or a dict, not {joint_map!r}")
        wanted = JOINT_MAPS[joint_map]
    elif isinstance(joint_map, dict):
        smpl = {n: i for i, n in enumerate(JOINT_MAPS["smpl"])}
        by_index = {}
        for k, v in joint_map.items():
            if isinstance(k, str) and k not in smpl:
                raise ValueError(f"joint_map names the joint {k!r}: not one of {JOINT_MAPS['smpl']}")
            by_index[smpl[k] if isinstance(k, str) else int(k)] = v
        if sorted(by_index) != list(range(len(by_index))) or not by_index:
            raise ValueError(f"joint_map must cover the joints 0 .. J - 1, not {sorted(by_index)}")
        wanted = [by_index[j] for j in range(len(by_index))]
    else:
        wanted = list(joint_map)
    missing = [w for w in wanted if _bare(w) not in at]
    if missing or not wanted:
        raise ValueError(f"the file has no node named {missing}" if missing else "joint_map names no joint")
    return [at[_bare(w)] for w in wanted]


def import_tables(bvh, pick):
    """The node tables ``mdm_rig_joints`` takes for ``pick`` (``resolve_joint_map``'s indices): -> (parent, offsets, rot_col,
    rot_axis, pick).  A picked End Site becomes a node of its own behind the file's N nodes: its parent the node it ends,
    its OFFSET the End Site's, no channels.  Raises ValueError for an index that is neither, and beyond ``MAX_IMPORT_NODES``."""
    N = len(bvh.names)
    parent, offsets = list(bvh.parent), [np.asarray(o, np.float64) for o in bvh.offsets]
    extra, out = {}, []
    for p in pick:
        p = int(p)
        if not 0 <= p < 2 * N or (p >= N and p - N not in bvh.end_sites):
            raise ValueError(f"pick {p}: not a node of the file (0 .. {N - 1}) or N + a node that has an End Site")
        if p >= N and p not in extra:
            extra[p] = len(parent)
            parent.append(p - N), offsets.append(np.asarray(bvh.end_sites[p - N], np.float64))
        out.append(extra.get(p, p))
    if len(parent) > MAX_IMPORT_NODES or len(out) > MAX_IMPORT_NODES:
        raise ValueError(f"{len(parent)} nodes and {len(out)} picked joints: at most {MAX_IMPORT_NODES} of each")
    pad = len(parent) - N
    rot_col = np.concatenate([np.asarray(bvh.rot_col, np.int32).reshape(N, 3), np.full((pad, 3), -1, np.int32)])
    rot_axis = np.concatenate([np.asarray(bvh.rot_axis, np.int32).reshape(N, 3), np.zeros((pad, 3), np.int32)])
    return np.asarray(parent, np.int32), np.stack(offsets), rot_col, rot_axis, np.asarray(out, np.int32)


def zero_length_bones(bvh, pick, skeleton):
    """The bones (parent joint, joint) of ``skeleton`` that have no length in any frame under ``pick``: both joints sit at the
    same point of the rig, which a node at zero OFFSET shares with its parent.  ``joints_to_motion`` divides by a bone's
    length."""
    from .motion_features import get_skeleton
    parent, offsets, _, _, at = import_tables(bvh, pick)

    def point(n):  # the highest node that n always coincides with
        while parent[n] >= 0 and not np.any(offsets[n]):
            n = int(parent[n])
        return n

    return [(p, c) for c, p in enumerate(get_skeleton(skeleton).parents) if p >= 0 and point(at[p]) == point(at[c])]


UP_BASIS = {"Y": ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)),
            "Z": ((1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, -1.0, 0.0))}  # Z-up right-handed -> Y-up: (x, y, z) -> (x, z, -y)


def _as_bvh(source):
    if isinstance(source, SimpleNamespace):
        return source
    if isinstance(source, os.PathLike) or (isinstance(source, str) and "\n" not in source and "\r" not in source
                                           and not source.lstrip().upper().startswith("HIERARCHY")):
        return read_bvh(source)
    if isinstance(source, str):
        return parse_bvh(source)
    raise ValueError(f"a source must be BVH text, a path or parse_bvh's namespace, not {type(source).__name__}")


def check_import(sources, joint_map=None, fps_out=20.0, scale=1.0, up="Y", basis=None):
    """Argument checks of ``bvh_to_joints`` that need no device: -> (the parsed files, per file its picked nodes, its (num, den)
    and its output length, the basis as a (3, 3) float32 array).  Raises ValueError, also where 22 or 21 joints are picked and
    a bone of that skeleton has no length (``zero_length_bones``)."""
    if isinstance(sources, (str, os.PathLike, SimpleNamespace)):
        raise ValueError("sources is a list of texts, paths or parsed files")
    files = [_as_bvh(s) for s in sources]
    if not files:
        raise ValueError("no sources given")
    if not np.isfinite(float(scale)):
        raise ValueError("scale must be finite")
    if basis is None:
        if up not in UP_BASIS:
            raise ValueError(f"up must be one of {sorted(UP_BASIS)}, not {up!r}")
        basis = UP_BASIS[up]
    basis = np.asarray(basis.detach().cpu() if torch.is_tensor(basis) else basis, dtype=np.float32)
    if basis.shape != (3, 3) or not np.isfinite(basis).all():
        raise ValueError("basis must be a finite 3 x 3 matrix")
    picks, ratios, lengths_out = [], [], []
    for i, f in enumerate(files):
        if f.frames < 1 or f.values.shape[1] < 1:
            raise ValueError(f"source {i} has no {'frames' if f.frames < 1 else 'channels'}")
        if len(f.names) > MAX_IMPORT_NODES:
            raise ValueError(f"source {i} has {len(f.names)} nodes: at most {MAX_IMPORT_NODES}")
        picks.append(resolve_joint_map(f, joint_map))
        skeleton = {22: "t2m", 21: "kit"}.get(len(picks[-1]))  # the joint counts of the skeletons that feature rows are made for
        flat = zero_length_bones(f, picks[-1], skeleton) if skeleton else []
        if flat:
            raise ValueError(f"source {i}: under this joint_map the {skeleton} bones {flat} (parent joint, joint) have no length, "
                             f"the joints sit at one point of the rig ({[(f.names[picks[-1][a] % len(f.names)], f.names[picks[-1][b] % len(f.names)]) for a, b in flat]}): "
                             "feature rows divide by a bone's length.  Give a joint_map that puts them at different nodes")
        num, den, _ = retime_ratio(None, 1.0 / float(f.frame_time), fps_out)
        ratios.append((num, den)), lengths_out.append((f.frames - 1) * num // den + 1)
    return files, picks, ratios, lengths_out, basis


@torch.no_grad()
def rig_joints(values, lengths, bvh, pick, num=1, den=1, *, scale=1.0, basis=UP_BASIS["Y"], return_quaternions=False):
    """One launch of ``mdm_rig_joints``: ``values`` (B, T, C) float32 on a GPU, the MOTION rows of B files that share the
    tables of ``bvh`` (``parse_bvh``'s namespace), zero-padded to T frames, with ``lengths`` (B,) or None -> ``(joints
    (B, T_out, len(pick), 3), lengths_out (B,) int64, quaternions (B, T_out, N, 4) or None)``, ``lengths_out = (length - 1)
    num // den + 1`` and ``T_out`` its largest; frames at or past it are zero, values at or past a length are never read.
    ``pick``: ``resolve_joint_map``'s indices (``import_tables`` makes a node of a picked End Site; the quaternions are those of
    the file's own N nodes).  Raises ValueError where the launch has 2^31 work items or more."""
    L.require_cuda(values)
    if values.dim() != 3 or values.dtype != torch.float32:
        raise ValueError(f"values must be float32 (B, T, C), not {values.dtype} {tuple(values.shape)}")
    values = values.contiguous()
    dev = values.device
    B, T, width = values.shape
    n = torch.full((B,), T, dtype=torch.int64) if lengths is None else \
        L.check_lengths(lengths, B, T, message=f"lengths must have {B} entries in [1, {T}]")
    lengths_out = (n - 1) * num // den + 1
    parent, offsets, rot_col, rot_axis, pick = import_tables(bvh, pick)
    N, n_pick = len(parent), len(pick)
    T_out = int(lengths_out.max()) if B else 1
    if B * T_out * (n_pick + N) >= 2 ** 31 or (T_out - 1) * int(den) >= 2 ** 31:
        raise ValueError(f"{B} files of up to {T_out} output frames at {num} / {den}: too long for one launch")
    ln, ln_out = n.to(dev, torch.int32), lengths_out.to(dev, torch.int32)
    out = torch.empty(B, T_out, n_pick, 3, device=dev)
    quat = torch.empty(B, T_out, N, 4, device=dev) if return_quaternions else None
    tables = [np.ascontiguousarray(a, dtype=t) for a, t in ((parent, np.int32), (offsets, np.float32), (rot_col, np.int32),
              (rot_axis, np.int32), (bvh.pos_col, np.int32), (pick, np.int32), (basis, np.float32))]
    with torch.cuda.device(dev):
        L.check(L.lib().mdm_rig_joints(
            values.data_ptr(), ln.data_ptr(), B, T, width, N, *(a.ctypes.data_as(C.c_void_p) for a in tables[:6]), n_pick,
            tables[6].ctypes.data_as(C.c_void_p), float(scale), int(num), int(den), T_out, ln_out.data_ptr(), out.data_ptr(),
            L.ptr(quat), L.stream_ptr()), "mdm_rig_joints")
    return out, lengths_out, None if quat is None else quat[:, :, :len(bvh.names)]


@torch.no_grad()
def bvh_to_joints(sources, *, joint_map=None, fps_out=20.0, scale=1.0, up="Y", basis=None, return_quaternions=False,
                  device=None):
    """``sources``, a list of BVH texts, paths or ``parse_bvh`` namespaces -> a list of joint positions (n_i, J, 3) on the
    GPU ``device`` (default the current one) at ``fps_out`` frames a second: the positions, by the file's own hierarchy,
    channel orders and OFFSETs, of the nodes that ``resolve_joint_map(file, joint_map)`` picks, times ``scale`` (0.01 for
    centimetres) and turned by ``basis`` (3 x 3; default by ``up``: "Y" as it is, "Z" the fixed turn of a Z-up right-handed
    file onto Y-up), ``out = scale * basis @ p``.  The source rate is ``1 / frame_time``: with ``num / den`` of
    ``retime_ratio`` output frame k lies at source frame k den / num, the local rotations slerped and the root lerped where
    that is no whole frame, and ``n_i = (frames - 1) num // den + 1``; ``fps_out=None`` keeps the file's frames.  Files
    whose tables and ratio agree share one launch of ``mdm_rig_joints``, padded and with their lengths.
    ``return_quaternions``: ``(joints, quaternions)``, the second a list of the retimed local unit quaternions (n_i, N, 4)
    of every node as (w, x, y, z), w >= 0.  No eager fallback: without a GPU this raises."""
    files, picks, ratios, lengths_out, basis = check_import(sources, joint_map, fps_out, scale, up, basis)
    dev = torch.device("cuda" if device is None else device)
    groups = {}
    for i, f in enumerate(files):  # files that one launch can take together
        key = (tuple(f.parent), np.asarray(f.offsets, np.float32).tobytes(), f.rot_col.tobytes(), f.rot_axis.tobytes(),
               f.pos_col.tobytes(), tuple(picks[i]), ratios[i], f.values.shape[1],
               tuple((n, np.asarray(v, np.float32).tobytes()) for n, v in sorted(f.end_sites.items())))
        groups.setdefault(key, []).append(i)
    joints, quats = [None] * len(files), [None] * len(files)
    for idx in groups.values():
        host = np.zeros((len(idx), max(files[i].frames for i in idx), files[idx[0]].values.shape[1]), np.float32)
        for b, i in enumerate(idx):
            host[b, :files[i].frames] = files[i].values
        out, _, quat = rig_joints(torch.from_numpy(host).to(dev), [files[i].frames for i in idx], files[idx[0]], picks[idx[0]],
                                      *ratios[idx[0]], scale=scale, basis=basis, return_quaternions=return_quaternions)
        for b, i in enumerate(idx):
            joints[i] = out[b, :lengths_out[i]]
            if return_quaternions:
                quats[i] = quat[b, :lengths_out[i]]
    return (joints, quats) if return_quaternions else joints


@torch.no_grad()
def bvh_to_motion(sources, mean, std, *, target_offsets=None, skeleton="t2m", **kw):
    """``bvh_to_joints(sources, **kw)`` followed by ``motion_features.joints_to_motion`` with ``mean`` / ``std`` and, when
    given, ``target_offsets`` (the retargeting of §16): -> (rows (B, max n_i - 1, F), normalised and zero past each clip, and
    the row counts n_i - 1 as an int64 tensor).  A file of n_i frames at the output rate gives n_i - 1 rows."""
    from .motion_features import joints_to_motion
    if kw.get("return_quaternions"):
        raise ValueError("bvh_to_motion returns rows: ask bvh_to_joints for the quaternions")
    clips = bvh_to_joints(sources, **kw)
    rows = joints_to_motion(clips, None, mean, std, skeleton=skeleton, target_offsets=target_offsets)
    return rows, torch.tensor([int(c.shape[0]) - 1 for c in clips], dtype=torch.int64)


# ---- rig retargeting ----

MAX_TARGET_JOINTS = 32  # mapped joints of mdm_retarget_channels
MAX_FIT_CHILDREN = 8    # children summed into b at a fitted node
RT_NONE, RT_COPY, RT_FIT = 0, 1, 2
_RT_I_HEAD, _RT_I_NODE, _RT_F_HEAD, _RT_F_NODE = 16, 16, 32, 12
_RT_F_BASE = _RT_I_HEAD + _RT_I_NODE * MAX_IMPORT_NODES
RT_WORDS = _RT_F_BASE + _RT_F_HEAD + _RT_F_NODE * MAX_IMPORT_NODES  # mdm_retarget_table_words()


def _unit(v):
    return v / np.linalg.norm(v)


def across(u):
    """The fixed unit vector across the unit vector ``u``: unit(u x e_m), m the axis of u's smallest component in absolute
    value, the lowest index on ties.  Half a turn about it is the rule for the shortest arc between opposite directions."""
    m = int(np.argmin(np.abs(u)))  # argmin takes the first of equal entries
    return _unit(np.cross(u, np.eye(3)[m]))


def shortest_arc(u, v):
    """The rotation (3, 3) float64 that takes the unit vector ``u`` onto the unit vector ``v`` about u x v; where they are
    opposite (1 + u.v < 1e-10), half a turn about ``across(u)``."""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    c = float(u @ v)
    if 1.0 + c < 1e-10:
        h = across(u)
        return 2.0 * np.outer(h, h) - np.eye(3)
    k = np.cross(u, v)
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + K + K @ K / (1.0 + c)


def two_vector_frame(a, b):
    """F(a, b) of §27 as a (3, 3) float64 matrix with the columns e1 = unit(a), e2 = e3 x e1, e3 = unit(e1 x b), or None where a
    or e1 x b has no length (below 1e-9 of |a|, and of |b| for the cross product)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    la, lb = np.linalg.norm(a), np.linalg.norm(b)
    if not la > 0 or not lb > 0:
        return None
    e1 = a / la
    c = np.cross(e1, b)
    if not np.linalg.norm(c) > 1e-9 * lb:
        return None
    e3 = _unit(c)
    return np.stack([e1, np.cross(e3, e1), e3], axis=1)


def skeleton_legs(skeleton):
    """Per leg (hip, knee, ankle) of a skeleton, as ``mdm_foot_skate`` finds them: the three joints above the toe joint
    ``feet[2 l + 1]`` in the chain that ends in it."""
    from .motion_features import get_skeleton
    sk = get_skeleton(skeleton)
    legs = []
    for l in range(2):
        ankle, toe = sk.feet[2 * l], sk.feet[2 * l + 1]
        for c in sk.chains:
            if len(c) >= 4 and c[-1] == toe and c[-2] == ankle:
                legs.append((c[-4], c[-3], c[-2]))
    if len(legs) != 2:
        raise ValueError("the skeleton has no two legs of hip, knee, ankle and toe")
    return legs


def _rotation_basis(up, basis):
    if basis is None:
        if up not in UP_BASIS:
            raise ValueError(f"up must be one of {sorted(UP_BASIS)}, not {up!r}")
        basis = UP_BASIS[up]
    basis = np.asarray(basis.detach().cpu() if torch.is_tensor(basis) else basis, dtype=np.float64)
    if basis.shape != (3, 3) or not np.isfinite(basis).all():
        raise ValueError("basis must be a finite 3 x 3 matrix")
    if np.abs(basis.T @ basis - np.eye(3)).max() > 1e-6 or np.linalg.det(basis) < 0:
        raise ValueError("basis must be a rotation (orthonormal, determinant +1): rotations are carried through it")
    return basis


def target_rig(source, joint_map=None, up="Y", basis=None, skeleton=None):
    """The description of a character to put motions on.  ``source``: BVH text, a path or ``parse_bvh``'s
    namespace (its MOTION rows are not used); ``joint_map`` as in ``resolve_joint_map``; ``up`` / ``basis`` as in
    ``bvh_to_joints``: source world vectors are taken into the file's axes by ``basis^T``, so that importing the written file
    with the same ``up`` gives back our world.  ``skeleton``: "t2m" / "kit", default by the number of mapped joints (22 / 21).
    -> a namespace of ``names``, ``parent``, ``offsets`` (N, 3) in the file's units and ``end_sites``, verbatim; ``pick``
    (``resolve_joint_map``'s; ``N + n`` is the End Site of node n, a child to point at that owns no channels); ``basis``;
    ``rest`` (N, 3) and ``joint_rest`` (J, 3), the rest positions (sums of OFFSETs); per node ``kind`` (``RT_NONE`` it turns with
    the node above, ``RT_COPY`` ``G = basis^T R[src] M``, ``RT_FIT`` ``G = basis^T F(cur) M``), ``res`` (the nearest node at or
    above with a rule, or -1), ``src`` and ``M`` (N, 3, 3); ``fit`` {node: (fa, fb, [bj])}; ``legs`` / ``leg_nodes`` /
    ``leg_rest`` ((l1, l2, u1, u2) per leg) / ``leg_ok`` / ``leg_length``; and ``table``, the ``RT_WORDS`` int32 words that
    ``mdm_retarget_channels`` takes.  All derived in float64.

    A mapped node with one mapped child at a non-zero rest distance copies that child's bone rotation, corrected by the
    shortest arc ``A`` from its rest direction u to the source's rest axis v (``M = basis A``, A from u to ``basis^T v``;
    ``shortest_arc`` states the rule for u = -v); with two or more it is fitted (``two_vector_frame``; a, from the pair of
    children whose rest directions have the smallest dot product, lowest indices on ties; b, the sum of the unit directions to
    the others, or to the two; a rest frame without length makes the node copy its lowest child instead); with none, and every
    unmapped node, it turns with the node above.  Raises ValueError for more than ``MAX_IMPORT_NODES`` nodes or
    ``MAX_TARGET_JOINTS`` joints, a root joint that is not on the file's root, two joints on one node, a joint whose parent
    joint sits on an End Site, a mapped node that is not below the node of its parent joint (an End Site may end that very
    node), a fitted node with more than ``MAX_FIT_CHILDREN + 2`` children, and legs without length."""
    from .motion_features import get_skeleton
    bvh = _as_bvh(source)
    N = len(bvh.names)
    if N > MAX_IMPORT_NODES:
        raise ValueError(f"the target has {N} nodes: at most {MAX_IMPORT_NODES}")
    pick = [int(p) for p in resolve_joint_map(bvh, joint_map)]
    J = len(pick)
    if J > MAX_TARGET_JOINTS:
        raise ValueError(f"{J} mapped joints: at most {MAX_TARGET_JOINTS}")
    if skeleton is None:
        skeleton = {22: "t2m", 21: "kit"}.get(J)
        if skeleton is None:
            raise ValueError(f"{J} mapped joints fit no skeleton: name one")
    sk = get_skeleton(skeleton)
    if sk.joints != J:
        raise ValueError(f"the joint map names {J} joints, the skeleton has {sk.joints}")
    B = _rotation_basis(up, basis)
    parent = [int(p) for p in bvh.parent]
    offsets = np.asarray(bvh.offsets, np.float64).reshape(N, 3)
    end_sites = {int(n): np.asarray(v, np.float64) for n, v in bvh.end_sites.items()}
    if len(set(pick)) != J:
        twice = sorted({p for p in pick if pick.count(p) > 1})
        raise ValueError(f"the joint map puts two joints on one node: {[bvh.names[p % N] + ('/End' if p >= N else '') for p in twice]}")
    if pick[0] != 0:
        raise ValueError(f"the root joint must sit on the file's root node {bvh.names[0]!r}, not on {bvh.names[pick[0] % N]!r}")
    rest = np.zeros((N, 3))  # relative to the root node: its own OFFSET moves the whole figure
    for n in range(1, N):
        rest[n] = rest[parent[n]] + offsets[n]
    for p in pick:
        if p >= N and p - N not in end_sites:
            raise ValueError(f"pick {p}: node {p - N} has no End Site")
    joint_rest = np.stack([rest[p] if p < N else rest[p - N] + end_sites[p - N] for p in pick])
    node_of = [p if p < N else -1 for p in pick]

    def below(n, top, or_equal=False):
        if or_equal and n == top:
            return True
        n = parent[n]
        while n >= 0:
            if n == top:
                return True
            n = parent[n]
        return False

    for j in range(1, J):
        pj = sk.parents[j]
        if node_of[pj] < 0:
            raise ValueError(f"joint {pj} sits on an End Site, which cannot carry joint {j} below it")
        ok = below(node_of[j], node_of[pj]) if node_of[j] >= 0 else below(pick[j] - N, node_of[pj], or_equal=True)
        if not ok:
            raise ValueError(f"joint {j} on {bvh.names[pick[j] % N]!r} is not below {bvh.names[node_of[pj]]!r}, the node of its "
                             f"parent joint {pj}: give a joint_map that follows the target's tree")
    extent = max(float(np.abs(joint_rest).max()), 1e-30)
    raw = np.asarray(sk.raw_offsets, np.float64)
    kind, src, M, fit = [RT_NONE] * N, [-1] * N, np.tile(np.eye(3), (N, 1, 1)), {}

    def copy_rule(n, jc):
        v = raw[jc]
        if not np.linalg.norm(v) > 0:
            raise ValueError(f"joint {jc} has no rest axis in the skeleton")
        kind[n], src[n] = RT_COPY, jc
        M[n] = B @ shortest_arc(_unit(joint_rest[jc] - rest[n]), B.T @ _unit(v))

    for j in range(J):
        n = node_of[j]
        if n < 0:
            continue
        kids = [jc for jc in range(J) if sk.parents[jc] == j and np.linalg.norm(joint_rest[jc] - rest[n]) > 1e-9 * extent]
        if len(kids) == 1:
            copy_rule(n, kids[0])
        elif len(kids) >= 2:
            dirs = {jc: _unit(joint_rest[jc] - rest[n]) for jc in kids}
            best, pair = None, None
            for i, ja in enumerate(kids):
                for jb in kids[i + 1:]:
                    d = float(dirs[ja] @ dirs[jb])
                    if best is None or d < best:
                        best, pair = d, (ja, jb)
            others = [jc for jc in kids if jc not in pair] or list(pair)
            if len(others) > MAX_FIT_CHILDREN:
                raise ValueError(f"node {bvh.names[n]!r} has {len(kids)} mapped children: at most {MAX_FIT_CHILDREN + 2}")
            F = two_vector_frame(joint_rest[pair[0]] - joint_rest[pair[1]], sum(dirs[jc] for jc in others))
            if F is None:
                copy_rule(n, kids[0])  # no rest frame: the node follows its lowest child
            else:
                kind[n], src[n], M[n], fit[n] = RT_FIT, j, F.T, (pair[0], pair[1], others)
    res = []
    for n in range(N):
        res.append(n if kind[n] != RT_NONE else (res[parent[n]] if parent[n] >= 0 else -1))
    legs = skeleton_legs(sk)
    leg_nodes, leg_rest, leg_ok = [], [], True
    for hip, knee, ankle in legs:
        d1, d2 = joint_rest[knee] - joint_rest[hip], joint_rest[ankle] - joint_rest[knee]
        l1, l2 = float(np.linalg.norm(d1)), float(np.linalg.norm(d2))
        if not (l1 > 1e-9 * extent and l2 > 1e-9 * extent):
            raise ValueError("a leg of the target has no length under this joint_map: the root cannot be rescaled")
        leg_nodes.append((node_of[hip], node_of[knee], node_of[ankle]))
        leg_rest.append((l1, l2, d1 / l1, d2 / l2))
        th, sh = node_of[hip], node_of[knee]
        leg_ok = leg_ok and min(th, sh, node_of[ankle]) >= 1 and kind[th] == RT_COPY and src[th] == knee \
            and kind[sh] == RT_COPY and src[sh] == ankle
    leg_length = float(np.mean([l[0] + l[1] for l in leg_rest]))
    table = np.zeros(RT_WORDS, np.int32)
    ftab = table.view(np.float32)[_RT_F_BASE:]
    table[0], table[1], table[2] = N, J, int(leg_ok)
    for l, ((hip, knee, ankle), (th, sh, _), (l1, l2, u1, u2)) in enumerate(zip(legs, leg_nodes, leg_rest)):
        table[4 + 6 * l:9 + 6 * l] = [hip, knee, ankle, max(th, 0), max(sh, 0)]
        ftab[10 + 8 * l:18 + 8 * l] = [l1, l2, *u1, *u2]
    ftab[:9], ftab[9] = B.reshape(9), leg_length
    for n in range(N):
        row = [parent[n], res[n], kind[n], max(src[n], 0)] + [0] * 12
        if kind[n] == RT_FIT:
            fa, fb, others = fit[n]
            row[4:7] = [fa, fb, len(others)]
            row[7:7 + len(others)] = others
        table[_RT_I_HEAD + _RT_I_NODE * n:_RT_I_HEAD + _RT_I_NODE * (n + 1)] = row
        ftab[_RT_F_HEAD + _RT_F_NODE * n:_RT_F_HEAD + _RT_F_NODE * (n + 1)] = [*offsets[n], *M[n].reshape(9)]
    return SimpleNamespace(names=list(bvh.names), parent=parent, offsets=offsets, end_sites=end_sites, pick=pick, n_nodes=N,
                           joints=J, skeleton=skeleton if isinstance(skeleton, str) else None, basis=B, rest=rest,
                           joint_rest=joint_rest, kind=kind, res=res, src=src, M=M, fit=fit, legs=legs, leg_nodes=leg_nodes,
                           leg_rest=leg_rest, leg_ok=bool(leg_ok), leg_length=leg_length, table=table, _device={})


def check_retarget(joints, rotations, lengths, target, offsets, skeleton="t2m", euler="ZXY", fps=None, fps_out=None, leg_ik=None):
    """Argument checks of ``retarget_to_rig`` that need no device: -> (joints (B, T, J, 3), rotations (B, T, J, 3, 3), lengths
    (B,) int64 or None, offsets (B, J, 3) float32, the target, the three axis indices, num, den, lengths_out (B,) int64, leg_ik
    as a bool).  Raises ValueError."""
    from .motion_features import get_skeleton
    if not (isinstance(target, SimpleNamespace) and hasattr(target, "table")):
        target = target_rig(target, skeleton=skeleton)
    sk = get_skeleton(skeleton)
    J = int(sk.joints)
    if target.joints != J or (isinstance(skeleton, str) and target.skeleton not in (None, skeleton)):
        raise ValueError(f"the target maps {target.joints} joints of {target.skeleton!r}, the motion is of {skeleton!r} ({J})")
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
    if offsets is None:
        raise ValueError("offsets are required: the (B, J, 3) bone offsets the forward kinematics returned")
    off = torch.as_tensor(offsets).detach().to(torch.float32)
    if off.dim() == 2:
        off = off[None].expand(B, J, 3)
    if tuple(off.shape) != (B, J, 3):
        raise ValueError(f"offsets of shape {tuple(off.shape)} must be ({J}, 3) or ({B}, {J}, 3)")
    if leg_ik is None:
        leg_ik = target.leg_ok
    if leg_ik and not target.leg_ok:
        raise ValueError("leg_ik needs hip, knee and ankle of both legs on nodes of the target, each with its one bone")
    num, den, _ = retime_ratio(skeleton, fps, fps_out)
    if lengths is not None:
        lengths = L.check_lengths(lengths, B, T)
    n = torch.full((B,), T, dtype=torch.int64) if lengths is None else lengths
    lengths_out = (n - 1) * num // den + 1
    if B and int(lengths_out.max()) * (3 + 3 * target.n_nodes) >= 2 ** 31:
        raise ValueError("the retimed motion is too long")
    return x, r, lengths, off, target, axes, num, den, lengths_out, bool(leg_ik)


@torch.no_grad()
def retarget_to_rig(joints, rotations, lengths, target, *, offsets, skeleton="t2m", euler="ZXY", fps=None, fps_out=None,
                    leg_ik=None, return_globals=False):
    """A motion onto a given character.  joints (B, T, J, 3), global rotations (B, T, J, 3, 3) and ``offsets``
    ((B, J, 3) or (J, 3)) on a GPU, as ``motion_to_joints_fk(..., sigma=0, return_rotations=True, return_offsets=True)`` or
    ``remove_foot_skate(..., rotations=)`` give them, and ``target``, ``target_rig``'s namespace (or what it takes) ->
    ``(channels (B, T_out, 3 + 3 N), lengths_out (B,))`` for the N nodes of the target's own hierarchy: the root's X Y Z in the
    file's units and axes, ``s basis^T x[0] - OFFSET[root]`` with s the target's leg length over the sample's, then three angles
    in degrees per node in ``euler`` order, as ``rotations_to_rig`` writes them.  Bone directions are the source's wherever a
    node has one mapped bone; unmapped nodes (fingers, twist bones) keep their rest pose.  ``leg_ik`` (default: on where the
    target's legs allow it): thigh and shin are turned so that the ankle nodes sit at ``s basis^T x[ankle]``.  ``fps`` /
    ``fps_out``: retimed as in ``rotations_to_rig``.  ``return_globals``: also the nodes' global rotations at the source
    frames (B, T, N, 3, 3), zero past each length.  The arithmetic is in ``mdm_retarget_channels``
    (csrc/motion_retarget.hip); no eager fallback."""
    x, r, lengths, off, target, axes, num, den, lengths_out, leg_ik = check_retarget(
        joints, rotations, lengths, target, offsets, skeleton, euler, fps, fps_out, leg_ik)
    L.require_cuda(x, r)
    dev = x.device
    if r.device != dev:
        raise ValueError("rotations must be on the joints' device")
    x, r = x.detach().to(torch.float32).contiguous(), r.detach().to(torch.float32).contiguous()
    off = off.to(dev).contiguous()
    B, T, J = x.shape[:3]
    N = target.n_nodes
    T_out = int(lengths_out.max()) if B else 1
    ln = None if lengths is None else lengths.to(dev, torch.int32).contiguous()
    ln_out = lengths_out.to(dev, torch.int32).contiguous()
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    if key not in target._device:  # one small device buffer per target
        target._device[key] = torch.from_numpy(target.table).to(dev)
    table = np.ascontiguousarray(target.table, np.int32)
    if table.size != L.lib().mdm_retarget_table_words():
        raise ValueError(f"the target's table has {table.size} words, the library takes {L.lib().mdm_retarget_table_words()}")
    chan = torch.empty(B, T_out, 3 + 3 * N, device=dev)
    glob = torch.empty(B, T, N, 3, 3, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().mdm_retarget_channels(
            x.data_ptr(), r.data_ptr(), off.data_ptr(), L.ptr(ln), B, T, J, table.ctypes.data_as(C.c_void_p),
            target._device[key].data_ptr(), int(leg_ik), axes[0], axes[1], axes[2], num, den, T_out, ln_out.data_ptr(),
            glob.data_ptr(), chan.data_ptr(), L.stream_ptr()), "mdm_retarget_channels")
    return (chan, lengths_out, glob) if return_globals else (chan, lengths_out)


def target_bvh_text(target, channels, n_frames, frame_time, *, euler="ZXY"):
    """The BVH file of one sample on the target's own hierarchy, as a ``str``: the names, OFFSETs and End Sites of ``target``
    (``target_rig``'s namespace) as they are, ``CHANNELS 6`` (X Y Z position, then the rotations in ``euler`` order) on the
    root and ``CHANNELS 3`` on every other node, then the first ``n_frames`` rows of ``channels`` (T, 3 + 3 N) from
    ``retarget_to_rig`` with the same ``euler``.  Numbers are printed with ``%.9g`` (``%.17g`` for float64 channels).  It does
    no arithmetic on the motion."""
    axes = _axes(euler)
    N = target.n_nodes
    ch = channels.detach().cpu().numpy() if torch.is_tensor(channels) else np.asarray(channels)
    if ch.dtype not in (np.float32, np.float64):
        ch = ch.astype(np.float32)
    if ch.ndim != 2 or ch.shape[1] != 3 + 3 * N:
        raise ValueError(f"channels of shape {ch.shape} must be (T, {3 + 3 * N}) for this target")
    n_frames = int(n_frames)
    if not 0 <= n_frames <= ch.shape[0]:
        raise ValueError(f"n_frames must lie in [0, {ch.shape[0]}]")
    if not (np.isfinite(float(frame_time)) and float(frame_time) > 0):
        raise ValueError("frame_time must be > 0")
    fmt = "%.17g" if ch.dtype == np.float64 else "%.9g"
    kids = [[] for _ in range(N)]
    for n in range(1, N):
        kids[target.parent[n]].append(n)
    rot = " ".join("XYZ"[a] + "rotation" for a in axes)
    out = ["HIERARCHY"]

    def vec(v):
        return " ".join(fmt % float(e) for e in v)

    def node(n, depth):
        pad = "  " * depth
        out.append(f"{pad}{'ROOT' if n == 0 else 'JOINT'} {target.names[n]}")
        out.append(pad + "{")
        out.append(f"{pad}  OFFSET {vec(target.offsets[n])}")
        out.append(f"{pad}  CHANNELS 6 Xposition Yposition Zposition {rot}" if n == 0 else f"{pad}  CHANNELS 3 {rot}")
        for k in kids[n]:
            node(k, depth + 1)
        if n in target.end_sites:
            out.extend([f"{pad}  End Site", pad + "  {", f"{pad}    OFFSET {vec(target.end_sites[n])}", pad + "  }"])
        out.append(pad + "}")

    node(0, 0)
    out.extend(["MOTION", f"Frames: {n_frames}", "Frame Time: %.9g" % float(frame_time)])
    out.extend(" ".join([fmt % v for v in row]) for row in ch[:n_frames].tolist())
    return "\n".join(out) + "\n"

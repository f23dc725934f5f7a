"""Numpy restatement of the rig import and the files its tests read, shared by tests/test_rig_import_host.py
and tests/test_rig_import_gpu.py.

Independent of motion_rig.py's import half and of csrc/motion_rig_import.hip: files are read with ``rig_ref.parse_bvh`` and
the arithmetic is ``rig_ref``'s textbook pieces in the dtype asked for (float64: the truth; float32: the yardstick), not the
kernel's forms (it composes quaternions and walks from a node up to the root; this goes down the tree with matrices):

* unretimed: ``rig_ref.bvh_fk`` on the file as the import takes it (``as_imported``: position channels of nodes other than
  the root zeroed, because the import ignores them);
* retimed: per node ``euler_to_matrix`` -> ``matrix_to_quaternion`` -> ``slerp`` -> ``quaternion_to_matrix``, then forward
  kinematics G = G_parent L, pos = pos_parent + G_parent OFFSET, the root's position lerped.

``variant`` builds the mistakes a reader most easily makes (tests/test_rig_import_host.py measures how far each lies from the
truth): "reversed" (L = R_a2 R_a1 R_a0), "radians", "root_order" (the root's axes on every node), "child_offset"
(pos = pos_parent + G_node OFFSET), "end_site_channels" (an End Site owns three columns), "positions_as_rotations" (an inner
node's position channels taken for its rotations), "no_flip" (slerp without the hemisphere flip), "basis_first" (the basis
applied to offsets and root positions before the walk instead of to the result).

No mocap file is in the tree, so the files are written here, in fp64 from joints and global rotations that satisfy
joint[c] = joint[p] + R[c] offset[c]: ``own_export`` (the text ``bvh_text`` prints), ``cmu_like`` and ``chain``.
"""
from types import SimpleNamespace

import numpy as np

import rig_ref as RR

EYE = np.eye(3)
Z_UP = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, -1.0, 0.0]])  # Z-up right-handed -> Y-up
VARIANTS = ("reversed", "radians", "root_order", "child_offset", "end_site_channels", "positions_as_rotations", "no_flip",
            "basis_first")


def as_imported(bvh):
    """The file as the import takes it: position channels on nodes other than the root read as zero."""
    v, col = bvh.values.copy(), 0
    for node, names in enumerate(bvh.channels):
        for name in names:
            if node > 0 and name[1:] == "position":
                v[:, col] = 0
            col += 1
    return SimpleNamespace(**{**vars(bvh), "values": v})


def with_end_sites(bvh):
    """The file with every End Site as a node of its own behind the N nodes, named ``<node>/End``: no channels, its parent the
    node it ends.  A joint map may put a joint there."""
    ends = sorted(bvh.end_sites)
    return SimpleNamespace(**{**vars(bvh), "names": list(bvh.names) + [bvh.names[n] + "/End" for n in ends],
                              "parent": list(bvh.parent) + ends, "channels": list(bvh.channels) + [[] for _ in ends],
                              "offsets": np.concatenate([bvh.offsets, np.stack([bvh.end_sites[n] for n in ends])]) if ends else bvh.offsets})


def node_channels(bvh, variant=None):
    """-> (per node the (column, axis) of its rotation channels in listed order, the root's position columns or -1)."""
    rot, pos, col, width = [], [-1, -1, -1], 0, bvh.values.shape[1]
    for node, names in enumerate(bvh.channels):
        r, p = [], []
        for name in names:
            (r if name[1:] == "rotation" else p).append((col % width, "XYZ".index(name[0])))
            col += 1
        if node == 0:
            for c, a in p:
                pos[a] = c
        elif p and variant == "positions_as_rotations":
            r = p
        rot.append(r)
        if variant == "end_site_channels" and node in bvh.end_sites:
            col += 3  # the End Site follows its node's channels in the file
    if variant == "root_order":
        rot = [[(c, rot[0][k][1]) for k, (c, _) in enumerate(r)] if len(r) == len(rot[0]) else r for r in rot]
    return rot, pos


def local_matrices(bvh, dtype, variant=None):
    """(frames, N, 3, 3): L = R_a0(v0) R_a1(v1) R_a2(v2) per node by ``rig_ref.euler_to_matrix``; a node with fewer than three
    rotation channels gets the angle 0 (about X) for the rest."""
    dtype = np.dtype(dtype)
    v = bvh.values.astype(dtype)
    rot, _ = node_channels(bvh, variant)
    out = []
    for r in rot:
        rad = np.zeros((len(v), 3), dtype)
        order = "".join("XYZ"[a] for _, a in r) + "X" * (3 - len(r))
        for k, (c, _) in enumerate(r):
            rad[:, k] = v[:, c] if variant == "radians" else v[:, c] * dtype.type(np.pi / 180)
        out.append(RR.euler_to_matrix(rad[:, ::-1], order[::-1]) if variant == "reversed" else RR.euler_to_matrix(rad, order))
    out = np.stack(out, 1)
    assert out.dtype == dtype
    return out


def walk_down(parent, offsets, L, root_pos, variant=None):
    """Forward kinematics down the tree, in L's dtype: -> positions (frames, N, 3)."""
    dtype = L.dtype
    n = len(L)
    pos, G = [], []
    for node, p in enumerate(parent):
        Gp = G[p] if p >= 0 else np.broadcast_to(np.eye(3, dtype=dtype), (n, 3, 3))
        G.append(Gp @ L[:, node])
        base = pos[p] if p >= 0 else root_pos.astype(dtype)
        pos.append(base + (G[node] if variant == "child_offset" else Gp) @ offsets[node].astype(dtype))
    out = np.stack(pos, 1)
    assert out.dtype == dtype
    return out


def import_joints(bvh, pick, num=1, den=1, dtype=np.float64, scale=1.0, basis=EYE, variant=None, force_quaternions=False):
    """One file (``rig_ref.parse_bvh``'s namespace) -> (joints (T_out, len(pick), 3), local quaternions (T_out, N', 4) or None)
    in ``dtype``; ``pick`` and N' count the nodes of ``with_end_sites``.  num == den: ``rig_ref.bvh_fk`` (no quaternions, unless
    forced); otherwise the slerp path."""
    dtype = np.dtype(dtype)
    basis = np.asarray(basis, np.float64)
    src = with_end_sites(as_imported(bvh))
    if variant == "basis_first":
        src = SimpleNamespace(**{**vars(src), "offsets": src.offsets @ basis.T})
    T = src.frames
    _, pos_col = node_channels(src, variant)
    v = src.values.astype(dtype)
    root = np.stack([v[:, c] if c >= 0 else np.zeros(T, dtype) for c in pos_col], -1)
    if variant == "basis_first":
        root = root @ basis.astype(dtype).T
    quat = None
    if num == den and variant is None and not force_quaternions:
        pos = RR.bvh_fk(src, dtype)[0]
    else:
        k = np.arange(RR.length_out(T, num, den))
        t0, rem = k * den // num, k * den % num
        t1 = np.where(rem > 0, t0 + 1, t0)  # frame t0 + 1 only where it is needed
        assert t1.max() < T
        f = (rem.astype(dtype) / dtype.type(num))[:, None]
        q = RR.matrix_to_quaternion(local_matrices(src, dtype, variant))
        quat = np.where((rem > 0)[:, None, None], RR.slerp(q[t0], q[t1], f[:, None], flip=variant != "no_flip"), q[t0])
        at = np.where(rem[:, None] > 0, root[t0] + f * (root[t1] - root[t0]), root[t0])
        assert quat.dtype == dtype and at.dtype == dtype
        pos = walk_down(src.parent, src.offsets, RR.quaternion_to_matrix(quat), at, variant)
    out = pos[:, list(pick)]
    if variant != "basis_first":
        out = out @ basis.astype(dtype).T
    out = dtype.type(scale) * out
    assert out.dtype == dtype
    return out, quat


def yardstick(files, picks, **kw):
    """Over a batch of parsed files: (per file the fp64 joints, how far the fp32 restatement lies from them at most)."""
    truth = [import_joints(f, p, dtype=np.float64, **kw)[0] for f, p in zip(files, picks)]
    y = max(float(np.abs(import_joints(f, p, dtype=np.float32, **kw)[0] - t).max()) for f, p, t in zip(files, picks, truth))
    return truth, y


def pick_of(bvh, names):
    """Node indices of ``names`` among the nodes of ``with_end_sites``: exact names, the test's own table and not the product's
    resolver."""
    return [with_end_sites(bvh).names.index(n) for n in names]


# ---- the files ----

def write_bvh(nodes, values, frame_time, fmt="%.9g"):
    """``nodes``: dicts of name, parent, offset, channels (names; None: no CHANNELS line) and an optional ``end`` offset, in
    depth-first order; ``values`` (frames, C) are rounded to float32 first, so that a float32 and a float64 reader see the same
    numbers.  -> text."""
    out, stack = ["HIERARCHY"], []

    def vec(v):
        return " ".join(fmt % float(e) for e in v)

    def close():
        n = stack.pop()
        pad = "  " * len(stack)
        if nodes[n].get("end") is not None:
            out.extend([f"{pad}  End Site", pad + "  {", f"{pad}    OFFSET {vec(nodes[n]['end'])}", pad + "  }"])
        out.append(pad + "}")

    for n, node in enumerate(nodes):
        while stack and stack[-1] != node["parent"]:
            close()
        assert (node["parent"] == -1) == (not stack)
        pad = "  " * len(stack)
        out.extend([f"{pad}{'ROOT' if not stack else 'JOINT'} {node['name']}", pad + "{", f"{pad}  OFFSET {vec(node['offset'])}"])
        if node["channels"] is not None:
            out.append(f"{pad}  CHANNELS {len(node['channels'])}" + "".join(" " + c for c in node["channels"]))
        stack.append(n)
    while stack:
        close()
    values = np.asarray(values, np.float64).astype(np.float32)
    assert values.shape[1] == sum(len(n["channels"] or ()) for n in nodes)
    out.extend(["MOTION", f"Frames: {len(values)}", "Frame Time: %.9g" % frame_time])
    out.extend(" ".join(fmt % v for v in row) for row in values.tolist())
    return "\n".join(out) + "\n"


def own_export(bvh_text, rig, offsets, joints, R, order="ZXY", frame_time=0.05, scale=1.0):
    """(a): the text ``motion_rig.bvh_text`` prints for the fp32 restatement's channels of one clip."""
    chan = RR.rig_channels(rig, joints, R, order, scale, dtype=np.float32)[0]
    return bvh_text(rig, offsets, chan, len(chan), frame_time, euler=order, scale=scale)


CMU_NAMES = {"pelvis": "Hips", "pelvis_to_left_hip": "LHipJoint", "pelvis_to_right_hip": "RHipJoint", "pelvis_to_spine1": "LowerBack",
             "left_hip": "LeftUpLeg", "left_knee": "LeftLeg", "left_ankle": "LeftFoot", "left_foot": "LeftToeBase",
             "right_hip": "RightUpLeg", "right_knee": "RightLeg", "right_ankle": "RightFoot", "right_foot": "RightToeBase",
             "spine1": "Spine", "spine2": "Spine1", "spine3": "Neck1", "spine3_to_neck": "NeckJoint", "neck": "Head",
             "spine3_to_left_collar": "LShoulderJoint", "left_collar": "LeftShoulder", "left_shoulder": "LeftArm",
             "left_elbow": "LeftForeArm", "left_wrist": "LeftHand", "spine3_to_right_collar": "RShoulderJoint",
             "right_collar": "RightShoulder", "right_shoulder": "RightArm", "right_elbow": "RightForeArm", "right_wrist": "RightHand"}
CMU_JOINTS = ("Hips", "LeftUpLeg", "RightUpLeg", "Spine", "LeftLeg", "RightLeg", "Spine1", "LeftFoot", "RightFoot", "Neck1",
              "LeftToeBase", "RightToeBase", "Head", "LeftShoulder", "RightShoulder", "Head/End", "LeftArm", "RightArm",
              "LeftForeArm", "RightForeArm", "LeftHand", "RightHand")  # the 22 joints in SMPL_JOINTS order
CMU_ORDERS = {"Hips": "ZYX", "LeftUpLeg": "XYZ", "RightLeg": "YXZ", "Spine": "YZX", "LeftArm": "XZY", "RightForeArm": "ZYX"}
CMU_SIX, CMU_NONE, CMU_BARE, CMU_ROOT_OFFSET = "LeftLeg", "LeftToeBase", "RightToeBase", (0.3, -0.2, 0.5)
# extra nodes below the hands and one foot: name, parent, offset, Euler order of their own small motion (two letters: the node
# with two rotation channels) and whether they end the chain
CMU_EXTRA = (("LeftFingerBase", "LeftHand", (0.0, -0.03, 0.0), "ZXY", False), ("LeftHandIndex1", "LeftFingerBase", (0.0, -0.04, 0.0), "ZX", True),
             ("LThumb", "LeftHand", (0.02, -0.02, 0.01), "YXZ", True), ("RightFingerBase", "RightHand", (0.0, -0.03, 0.0), "XZY", True),
             ("LeftToeEnd", "LeftToeBase", (0.0, 0.0, 0.05), "ZXY", True))


def cmu_like(rig, offsets, joints, R, frame_time=0.05, prefix="", seed=0):
    """(b): one clip as a CMU-like file, fp64: ``rig``'s nodes under the names of the CMU preset (the head joint is the End Site
    of Head, and a Neck node at zero offset sits below Spine1), extra finger and toe nodes with End Sites and a motion of their own, other Euler orders on several nodes (angles by ``rig_ref.matrix_to_euler``),
    one node with two rotation channels, one with ``CHANNELS 0`` and one with no CHANNELS line, one inner node with six
    channels whose positions repeat its OFFSET, a non-zero root OFFSET, ``prefix`` before every name.  The joints sit at the
    nodes ``CMU_JOINTS``; those of the input clip are what a reader rebuilds (to the rounding of the printed numbers)."""
    assert rig.names[0] == "pelvis" and rig.joints == 22
    rs = np.random.RandomState(seed)
    joints, R, off = np.asarray(joints, np.float64), np.asarray(R, np.float64), np.asarray(offsets, np.float64)
    T = len(joints)
    local = RR.local_rotations(rig, R)
    kids = [[m for m, p in enumerate(rig.parent) if p == n] for n in range(rig.n_nodes)]
    extras = {}
    for e in CMU_EXTRA:
        extras.setdefault(e[1], []).append(e)
    nodes, cols = [], []

    def angles(L, order):
        return np.rad2deg(RR.matrix_to_euler(L, order))

    def add(name, parent, offset, chans, vals, end=None):
        nodes.append(dict(name=prefix + name, parent=parent, offset=np.asarray(offset, np.float64), channels=chans, end=end))
        cols.extend(vals.T if vals is not None else [])
        return len(nodes) - 1

    def add_extras(below, at):
        for name, _, o, order, ends in extras.get(below, ()):
            a = np.cumsum(rs.uniform(-6, 6, (T, len(order))), 0) + rs.uniform(-30, 30, len(order))  # degrees, its own motion
            n = add(name, at, o, [c + "rotation" for c in order], a, end=0.5 * np.asarray(o) if ends else None)
            add_extras(name, n)

    def walk(n, above):
        o = off[rig.joint_of[n]] if rig.has_offset[n] else np.zeros(3)
        if rig.names[n] == "head":  # the head joint is the End Site of the node Head, as the CMU preset has it
            nodes[above]["end"] = o
            return
        if rig.names[n] == "spine3":  # the CMU files' Neck: a node at zero offset that does not turn, between Spine1 and Neck1
            above = add("Neck", above, np.zeros(3), ["Zrotation", "Yrotation", "Xrotation"], np.zeros((T, 3)))
        name = CMU_NAMES[rig.names[n]]
        order = CMU_ORDERS.get(name, "ZXY")
        rot = [c + "rotation" for c in order]
        leaf = not kids[n] and name not in extras
        end = None if not leaf else (0.05 * o / np.linalg.norm(o))
        if n == 0:
            at = add(name, -1, CMU_ROOT_OFFSET, ["Xposition", "Yposition", "Zposition"] + rot,
                     np.concatenate([joints[:, 0] - np.asarray(CMU_ROOT_OFFSET), angles(local[:, n], order)], 1))
        elif name == CMU_SIX:
            at = add(name, above, o, ["Xposition", "Yposition", "Zposition"] + rot,
                     np.concatenate([np.broadcast_to(o, (T, 3)), angles(local[:, n], order)], 1))
        elif name in (CMU_NONE, CMU_BARE):
            assert not kids[n] and np.abs(local[:, n] - np.eye(3)).max() <= 1e-12  # a leaf does not turn
            at = add(name, above, o, [] if name == CMU_NONE else None, None, end)
        else:
            at = add(name, above, o, rot, angles(local[:, n], order), end)
        for m in kids[n]:
            walk(m, at)
        add_extras(name, at)

    walk(0, -1)
    return write_bvh(nodes, np.stack(cols, 1), frame_time)


# The hierarchy of the CMU files (cgspeed conversion) in metres, rounded: name, parent, OFFSET.  LHipJoint, RHipJoint, LowerBack,
# Neck, LeftShoulder and RightShoulder are at zero offset, as the files have them.
CMU_REAL = (("Hips", None, (0, 0, 0)),
            ("LHipJoint", "Hips", (0, 0, 0)), ("LeftUpLeg", "LHipJoint", (0.08, -0.10, 0.05)), ("LeftLeg", "LeftUpLeg", (0.14, -0.39, 0)),
            ("LeftFoot", "LeftLeg", (0.15, -0.41, 0)), ("LeftToeBase", "LeftFoot", (0.01, -0.03, 0.12)),
            ("RHipJoint", "Hips", (0, 0, 0)), ("RightUpLeg", "RHipJoint", (-0.08, -0.10, 0.05)), ("RightLeg", "RightUpLeg", (-0.14, -0.39, 0)),
            ("RightFoot", "RightLeg", (-0.15, -0.41, 0)), ("RightToeBase", "RightFoot", (-0.01, -0.03, 0.12)),
            ("LowerBack", "Hips", (0, 0, 0)), ("Spine", "LowerBack", (0, 0.12, -0.01)), ("Spine1", "Spine", (0, 0.12, 0)),
            ("Neck", "Spine1", (0, 0, 0)), ("Neck1", "Neck", (0, 0.09, 0.01)), ("Head", "Neck1", (0, 0.09, -0.01)),
            ("LeftShoulder", "Spine1", (0, 0, 0)), ("LeftArm", "LeftShoulder", (0.19, 0.05, 0)), ("LeftForeArm", "LeftArm", (0.29, 0, 0)),
            ("LeftHand", "LeftForeArm", (0.20, 0, 0)), ("LeftFingerBase", "LeftHand", (0.04, 0, 0)), ("LeftHandIndex1", "LeftFingerBase", (0.03, 0, 0)),
            ("LThumb", "LeftHand", (0.02, 0, 0.02)),
            ("RightShoulder", "Spine1", (0, 0, 0)), ("RightArm", "RightShoulder", (-0.19, 0.05, 0)), ("RightForeArm", "RightArm", (-0.29, 0, 0)),
            ("RightHand", "RightForeArm", (-0.20, 0, 0)), ("RightFingerBase", "RightHand", (-0.04, 0, 0)),
            ("RightHandIndex1", "RightFingerBase", (-0.03, 0, 0)), ("RThumb", "RightHand", (-0.02, 0, 0.02)))
# the placement that first comes to mind, spine3 at Neck: on this hierarchy spine2 -> spine3 and spine3 -> collars have no length
CMU_NAIVE = tuple({"Neck1": "Neck", "Head": "Neck1", "Head/End": "Head"}.get(n, n) for n in CMU_JOINTS)


def cmu_real(frames=9, seed=0, frame_time=1 / 120):
    """A file on the CMU files' own hierarchy, zero offsets included: 31 nodes, ``CHANNELS 3 Zrotation Yrotation Xrotation``
    on every node, End Sites on the leaves, a walk forward with every node turning by tens of degrees."""
    rs = np.random.RandomState(seed)
    index = {name: i for i, (name, _, _) in enumerate(CMU_REAL)}
    parents = {p for _, p, _ in CMU_REAL}
    nodes, cols = [], []
    for name, p, o in CMU_REAL:
        rot = ["Zrotation", "Yrotation", "Xrotation"]
        o = np.asarray(o, np.float64)
        end = None if name in parents else (0.1 * o / np.linalg.norm(o) if name != "Head" else np.array([0.0, 0.1, 0.0]))
        nodes.append(dict(name=name, parent=-1 if p is None else index[p], offset=o + ((0, 0.9, 0) if p is None else 0),
                          channels=(["Xposition", "Yposition", "Zposition"] if p is None else []) + rot, end=end))
        if p is None:
            cols.extend(np.stack([0.05 * rs.randn(frames), 0.02 * rs.randn(frames), 0.01 * np.arange(frames)]))
        cols.extend((np.cumsum(rs.uniform(-1, 1, (frames, 3)), 0) + rs.uniform(-25, 25, 3)).T)
    return write_bvh(nodes, np.stack(cols, 1), frame_time)


def chain(n_nodes=128, frames=3, seed=0, frame_time=0.05):
    """(c): a single chain of ``n_nodes`` nodes ``n000`` ..., each with its own Euler order, a bone of 2 cm and a few degrees
    of rotation a node, so that the chain curls."""
    rs = np.random.RandomState(seed)
    nodes, cols = [], []
    for n in range(n_nodes):
        order = RR.ORDERS[rs.randint(6)]
        chans = ([a + "position" for a in "XYZ"] if n == 0 else []) + [a + "rotation" for a in order]
        nodes.append(dict(name=f"n{n:03d}", parent=n - 1, offset=rs.uniform(-1, 1, 3) * 0.02, channels=chans,
                          end=(0.0, 0.02, 0.0) if n == n_nodes - 1 else None))
        if n == 0:
            cols.extend(rs.uniform(-1, 1, (3, frames)))
        cols.extend(rs.uniform(-8, 8, (3, frames)) + rs.uniform(-20, 20, (3, 1)))
    return write_bvh(nodes, np.stack(cols, 1), frame_time)


def analytic_joints(rig, offsets, local_at, taus):
    """``rig_ref.spin_clip``'s analytic local rotations and root position at the frame times ``taus``, through fp64 forward
    kinematics on the rig's own tree: joints (len(taus), J, 3)."""
    off = np.asarray(offsets, np.float64)
    node_off = np.stack([off[j] if h else np.zeros(3) for j, h in zip(rig.joint_of, rig.has_offset)])
    L, root = zip(*(local_at(float(t)) for t in taus))
    pos = walk_down(rig.parent, node_off, np.stack(L), np.stack(root))
    at = {j: n for n, j in enumerate(rig.joint_of) if j >= 0}
    return pos[:, [at[j] for j in range(rig.joints)]]

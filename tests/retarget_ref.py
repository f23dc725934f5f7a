"""Numpy restatement of the rig retargeting, shared by tests/test_retarget_host.py and tests/test_retarget_gpu.py.

What it takes from ``motion_rig.target_rig`` is the target's structure, which is data and is checked on its own in the host tests:
the tree, which node follows which rule (``kind``, ``src``, ``fit``), the legs.  Every number is computed here again, in the
dtype asked for (float64: the truth; float32: the yardstick) and in textbook forms that are not the kernel's: the rest
correction as an axis and an arccos angle through Rodrigues' formula (the kernel multiplies by a table the host made from
1 + u.v), the leg as two angles of the law of cosines turned about the bend axis (the kernel adds cos and sin parts of two unit
vectors and swings by a quaternion), the globals down the tree parents first, the positions by the walk down.  Local rotations,
quaternions, slerp and Euler angles are those of tests/rig_ref.py, and so is the text-only BVH reader the results are read
back with.

The synthetic targets are written here as BVH text, nothing comes from a file: (a) ``own_rig_text``, the project's own export
tree (optionally every bone subdivided by an unmapped node); (b) ``mixamo_text()``, a Mixamo-named T-pose skeleton in
centimetres with fingers and ``HeadTop_End``, 65 nodes; (c) ``mixamo_text(pose="A")``, arms 45 degrees down in rest; (d)
``cmu_text()`` with ``CMU_MAP``, zero-offset ``LHipJoint`` / ``LowerBack`` / ``Neck`` / ``LeftShoulder`` nodes and the head on
``Head``'s End Site; (e) ``mixamo_text(up="Z")``; (f) ``mixamo_text(pose="up")``, the left upper arm pointing straight up in rest,
opposite to the source's rest axis of the elbow.

``variant`` builds the mistakes an implementation most easily makes (tests/test_retarget_host.py measures how far each lies from
the truth): "no_rest" (no rest correction), "a_transposed", "own_rotation" (R[j] copied instead of R[jc]), "fit_reversed"
(F(rest) F(cur)^T), "no_scale" (the root not rescaled), "basis" (basis where basis^T belongs), "knee_mirrored".
"""
import numpy as np

import rig_ref as RR

Z_UP = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, -1.0, 0.0]])  # motion_rig.UP_BASIS["Z"]
VARIANTS = ("no_rest", "a_transposed", "own_rotation", "fit_reversed", "no_scale", "basis", "knee_mirrored")


PAIRS = {"t2m": ((1, 2), (4, 5), (7, 8), (10, 11), (13, 14), (16, 17), (18, 19), (20, 21)),
         "kit": ((5, 8), (6, 9), (7, 10), (11, 16), (12, 17), (13, 18), (14, 19), (15, 20))}


def even_offsets(skeleton, offsets):
    """Bone offsets (J, 3) with the lengths of every left / right pair of bones averaged, directions kept.  The shared offsets of
    tests/golden/motion_fk.npz are random per bone (a left thigh of 0.11 beside a right one of 0.31): on them no scale fits both
    legs and half of all leg-frames are out of any target's reach.  The retargeting tests pose the golden rotations on these
    instead, which is the clip chosen for the leg IK."""
    off = np.array(offsets, np.float64)
    for a, b in PAIRS[skeleton]:
        la, lb = np.linalg.norm(off[a]), np.linalg.norm(off[b])
        off[a], off[b] = off[a] * (0.5 * (la + lb) / la), off[b] * (0.5 * (la + lb) / lb)
    return off


def pose(parents, root, R, offsets):
    """Forward kinematics restated: root (T, 3), R (T, J, 3, 3), offsets (J, 3) -> joints (T, J, 3), x[c] = x[parent] + R[c] off[c]."""
    x = np.zeros(R.shape[:2] + (3,), R.dtype)
    x[:, 0] = root
    for c in range(1, R.shape[1]):
        x[:, c] = x[:, parents[c]] + R[:, c] @ offsets[c]
    return x


# ---- the targets, as text ----

def hierarchy_text(tree, turn=None, order="ZXY"):
    """``tree``: (name, offset, children, end site offset or None), nested -> BVH text with an empty MOTION section, in the
    layout ``motion_rig.target_bvh_text`` writes.  ``turn`` (3, 3): every offset is turned by it."""
    rot = " ".join(a + "rotation" for a in order)
    out = ["HIERARCHY"]

    def vec(v):
        v = np.asarray(v, np.float64)
        return " ".join("%.9g" % float(e) for e in (v if turn is None else turn @ v))

    def node(t, depth):
        name, offset, children, end = t
        pad = "  " * depth
        out.extend([f"{pad}{'ROOT' if depth == 0 else 'JOINT'} {name}", pad + "{", f"{pad}  OFFSET {vec(offset)}",
                    f"{pad}  CHANNELS 6 Xposition Yposition Zposition {rot}" if depth == 0 else f"{pad}  CHANNELS 3 {rot}"])
        for c in children:
            node(c, depth + 1)
        if end is not None:
            out.extend([f"{pad}  End Site", pad + "  {", f"{pad}    OFFSET {vec(end)}", pad + "  }"])
        out.append(pad + "}")

    node(tree, 0)
    return "\n".join(out + ["MOTION", "Frames: 0", "Frame Time: 0.05"]) + "\n"


def _chain(names, offsets, tail=(), end=None):
    """A chain of nodes; ``tail``: the children of its last node."""
    t = (names[-1], offsets[-1], list(tail), end)
    for n, o in zip(names[-2::-1], offsets[-2::-1]):
        t = (n, o, [t], None)
    return t


def mixamo_text(pose="T", up="Y"):
    """Rig (b) / (c) / (e) / (f): 65 nodes named as Mixamo names them, centimetres; thigh : shin 46 : 37 and shoulders 17 wide,
    unlike the model's.  ``pose`` "T", "A" (both arms 45 degrees down) or "up" (the left upper arm straight up)."""
    p = "mixamorig:"

    def arm(side, sx):
        a = np.deg2rad(45.0) if pose == "A" else 0.0
        along = np.array([sx * np.cos(a), -np.sin(a), 0.0])   # the arm's direction in rest
        down = np.array([sx * -np.sin(a), -np.cos(a), 0.0])   # across it, in the arm's plane
        fingers = []
        for i, f in enumerate(("Thumb", "Index", "Middle", "Ring", "Pinky")):
            first = 3.0 * along + (i - 2) * 1.1 * np.array([0.0, 0.0, -1.0]) + (0.8 * down if i == 0 else 0.0)
            fingers.append(_chain([f"{p}{side}Hand{f}{k}" for k in (1, 2, 3, 4)], [first, 2.6 * along, 2.1 * along, 1.7 * along]))
        upper = np.array([0.0, 27.0, 0.0]) if pose == "up" and side == "Left" else 27.0 * along
        return _chain([p + side + n for n in ("Shoulder", "Arm", "ForeArm", "Hand")],
                      [np.array([sx * 5.5, 11.0, -0.5]), np.array([sx * 11.5, 0.0, 0.0]), upper, 25.0 * along], fingers)

    def leg(side, sx):
        return _chain([p + side + n for n in ("UpLeg", "Leg", "Foot", "ToeBase", "Toe_End")],
                      [(sx * 9.0, -5.5, 0.0), (0.0, -46.0, 0.5), (0.0, -37.0, -1.0), (0.0, -9.0, 12.0), (0.0, 0.0, 7.0)])

    head = _chain([p + n for n in ("Neck", "Head", "HeadTop_End")], [(0.0, 14.0, 0.5), (0.0, 9.0, 1.5), (0.0, 18.0, 0.0)])
    spine = _chain([p + n for n in ("Spine", "Spine1", "Spine2")], [(0.0, 9.5, -1.0), (0.0, 11.0, 0.0), (0.0, 12.5, 0.0)],
                   [head, arm("Left", 1.0), arm("Right", -1.0)])
    tree = (p + "Hips", (0.0, 0.0, 0.0), [spine, leg("Left", 1.0), leg("Right", -1.0)], None)
    return hierarchy_text(tree, Z_UP.T if up == "Z" else None)


# rig (d): the 22 joints in SMPL_JOINTS order on a CMU-named tree.  spine3 sits on Spine1, where the shoulders hang; spine1 on
# the zero-offset LowerBack (that bone has no length in the target); the head on Head's End Site
CMU_MAP = ("Hips", "LeftUpLeg", "RightUpLeg", "LowerBack", "LeftLeg", "RightLeg", "Spine", "LeftFoot", "RightFoot", "Spine1",
           "LeftToeBase", "RightToeBase", "Neck1", "LeftShoulder", "RightShoulder", "Head/End", "LeftArm", "RightArm",
           "LeftForeArm", "RightForeArm", "LeftHand", "RightHand")


def cmu_text():
    """Rig (d), in units of its own (about 17 to the figure's height, as the CMU files have it): zero-offset ``LHipJoint``,
    ``LowerBack``, ``Neck`` and ``Shoulder`` nodes, legs that start sideways and down, arms that rise before they go out."""
    zero = (0.0, 0.0, 0.0)

    def leg(side, s, sx):
        return _chain([f"{s}HipJoint", side + "UpLeg", side + "Leg", side + "Foot", side + "ToeBase"],
                      [zero, (sx * 1.6, -1.9, 0.9), (sx * 2.4, -7.1, 0.0), (sx * 2.6, -7.3, 0.0), (sx * 0.1, -0.4, 2.1)],
                      end=(0.0, 0.0, 1.0))

    def arm(side, sx):
        hand = [_chain([side + "FingerBase", side + "HandIndex1"], [zero, (sx * 0.7, 0.0, 0.0)], end=(sx * 0.5, 0.0, 0.0)),
                (f"{side[0]}Thumb", zero, [], (sx * 0.5, 0.0, 0.5))]
        return _chain([side + "Shoulder", side + "Arm", side + "ForeArm", side + "Hand"],
                      [zero, (sx * 3.3, 1.7, -0.3), (sx * 5.0, 0.0, 0.0), (sx * 3.4, 0.0, 0.0)], hand)

    head = _chain(["Neck", "Neck1", "Head"], [zero, (-0.1, 1.7, 0.3), (0.0, 1.6, -0.2)], end=(0.0, 1.7, 0.1))
    spine = _chain(["LowerBack", "Spine", "Spine1"], [zero, (0.0, 2.1, -0.2), (0.0, 2.2, 0.0)],
                   [head, arm("Left", 1.0), arm("Right", -1.0)])
    return hierarchy_text(("Hips", zero, [leg("Left", "L", 1.0), leg("Right", "R", -1.0), spine], None))


def own_rig_text(MRig, skeleton, offsets, subdivide=False):
    """Rig (a): the tree of ``MRig.rig_of(skeleton)`` with ``offsets`` (J, 3), as ``bvh_text`` writes it, in metres.
    ``subdivide``: every bone that has length goes through an unmapped node ``<name>_mid`` at 0.4 of it."""
    rig = MRig.rig_of(skeleton)
    if not subdivide:
        return MRig.bvh_text(rig, offsets, np.zeros((1, 3 + 3 * rig.n_nodes), np.float32), 0, 0.05)
    off = np.asarray(offsets, np.float64)
    kids = [[] for _ in rig.names]
    for n, p in enumerate(rig.parent):
        if p >= 0:
            kids[p].append(n)

    def build(n):
        o = off[rig.joint_of[n]] if rig.has_offset[n] else np.zeros(3)
        t = (rig.names[n], o, [build(k) for k in kids[n]], None if kids[n] else (0.0, 0.05, 0.0))
        if np.any(o):
            t = (rig.names[n] + "_mid", 0.4 * o, [(t[0], 0.6 * o, t[2], t[3])], None)
        return t

    return hierarchy_text(build(0))


# ---- the conversion, restated ----

def _rodrigues(axis, ang, dt):
    """The rotation about the unit ``axis`` by ``ang`` radians, I + sin K + (1 - cos) K K, in ``dt``."""
    x, y, z = (dt.type(e) for e in axis)
    o, ang = dt.type(0), dt.type(ang)
    K = np.array([[o, -z, y], [z, o, -x], [-y, x, o]], dt)
    return np.eye(3, dtype=dt) + np.sin(ang) * K + (dt.type(1) - np.cos(ang)) * (K @ K)


def _across(u):
    m = int(np.argmin(np.abs(u)))
    k = np.cross(u, np.eye(3, dtype=u.dtype)[m])
    return k / np.linalg.norm(k)


def arc(u, v):
    """The shortest turn from unit u to unit v: about unit(u x v) by arccos(u.v); opposite vectors (no axis): half a turn about
    unit(u x e_m), m the axis of u's smallest component."""
    dt = u.dtype
    k = np.cross(u, v)
    s = np.linalg.norm(k)
    if s < 1e-5 and u @ v < 0:
        return _rodrigues(_across(u), dt.type(np.pi), dt)
    if s == 0:
        return np.eye(3, dtype=dt)
    return _rodrigues(k / s, np.arctan2(s, u @ v), dt)  # the angle between two vectors, well conditioned at every angle


def frame(a, b):
    """F(a, b) as columns, or None where it has no length."""
    la = np.linalg.norm(a)
    if not la > 1e-10:
        return None
    e1 = a / la
    c = np.cross(e1, b)
    lc = np.linalg.norm(c)
    if not lc > 1e-6:
        return None
    e3 = c / lc
    return np.stack([e1, np.cross(e3, e1), e3], axis=1)


def _unit(v):
    return v / np.linalg.norm(v)


def scale_of(target, off):
    """s: the target's leg length over the sample's, thigh + shin, left and right averaged."""
    want = np.mean([np.linalg.norm(target.joint_rest[k] - target.joint_rest[h]) + np.linalg.norm(target.joint_rest[a] - target.joint_rest[k])
                    for h, k, a in target.legs])
    have = np.mean([np.linalg.norm(off[k]) + np.linalg.norm(off[a]) for h, k, a in target.legs])
    return want / have


def globals_of(target, raw, x, R, off, dtype=np.float64, leg_ik=False, variant=None):
    """One sample, x (T, J, 3), R (T, J, 3, 3), off (J, 3) -> (the nodes' global rotations (T, N, 3, 3), the root position
    (T, 3), s), everything in ``dtype``."""
    dt = np.dtype(dtype)
    x, R, off = np.asarray(x).astype(dt), np.asarray(R).astype(dt), np.asarray(off).astype(dt)
    Bt = np.asarray(target.basis).astype(dt).T
    vecs = Bt.T if variant == "basis" else Bt       # what takes a source world vector into the file's axes
    rest, jrest, raw = target.rest.astype(dt), target.joint_rest.astype(dt), np.asarray(raw).astype(dt)
    T, N = len(x), target.n_nodes
    s = dt.type(1) if variant == "no_scale" else (scale_of(target, off)).astype(dt)
    root = s * (x[:, 0] @ vecs.T)
    G = np.zeros((T, N, 3, 3), dt)
    eye = np.eye(3, dtype=dt)
    for n in range(N):
        p = target.parent[n]
        if target.kind[n] == 0:
            G[:, n] = G[:, p] if p >= 0 else eye
        elif target.kind[n] == 1:
            jc = target.src[n]
            A = arc(_unit(jrest[jc] - rest[n]), vecs @ _unit(raw[jc]))
            if variant == "no_rest":
                A = eye
            if variant == "a_transposed":
                A = A.T
            take = [j for j, q in enumerate(target.pick) if q == n][0] if variant == "own_rotation" else jc
            G[:, n] = (vecs @ R[:, take] @ vecs.T) @ A
        else:
            fa, fb, others = target.fit[n]
            j = target.src[n]
            Fr = frame(jrest[fa] - jrest[fb], sum(_unit(jrest[c] - rest[n]) for c in others))
            for t in range(T):
                cur = [(x[t, c] - x[t, j]) @ vecs.T for c in others]
                Fc = frame((x[t, fa] - x[t, fb]) @ vecs.T, sum(c / np.linalg.norm(c) for c in cur if np.linalg.norm(c) > 0))
                if Fc is None:
                    G[t, n] = vecs @ R[t, j] @ vecs.T  # the documented fallback: the joint's own rotation
                else:
                    G[t, n] = Fr @ Fc.T if variant == "fit_reversed" else Fc @ Fr.T
    assert G.dtype == dt and root.dtype == dt
    if leg_ik:
        for (hip, knee, ankle), (th, sh, an) in zip(target.legs, target.leg_nodes):
            path, a = [], th
            while a > 0:
                path.append(a)
                a = target.parent[a]
            l1, l2 = np.linalg.norm(jrest[knee] - jrest[hip]), np.linalg.norm(jrest[ankle] - jrest[knee])
            u1, u2 = (jrest[knee] - jrest[hip]) / l1, (jrest[ankle] - jrest[knee]) / l2
            under_thigh = [n for n in range(N) if target.res[n] == th]
            under_shin = [n for n in range(N) if target.res[n] == sh]
            for t in range(T):
                at = root[t] + sum(G[t, target.parent[a]] @ target.offsets[a].astype(dt) for a in path)
                d = s * (vecs @ x[t, ankle]) - at
                dist = np.linalg.norm(d)
                c1, c2 = G[t, th] @ u1, G[t, sh] @ u2
                nrm = d / dist if dist > 1e-6 * (l1 + l2) else c1
                eps = dt.type(1e-4) * (l1 + l2)
                reach = np.clip(dist, abs(l1 - l2) + eps, l1 + l2 - eps)
                w = vecs @ (x[t, knee] - x[t, hip])
                pole = w - (w @ nrm) * nrm
                if pole @ pole <= 1e-10 * (w @ w):
                    pole = c1 - (c1 @ nrm) * nrm
                    if pole @ pole <= 1e-10:
                        pole = _across(nrm)
                pole = pole / np.linalg.norm(pole)
                if variant == "knee_mirrored":
                    pole = -pole
                bend = _unit(np.cross(nrm, pole))  # turning about it takes nrm towards the pole
                alpha = np.arccos(np.clip((l1 * l1 + reach * reach - l2 * l2) / (2 * l1 * reach), -1, 1))
                beta = np.arccos(np.clip((l2 * l2 + reach * reach - l1 * l1) / (2 * l2 * reach), -1, 1))
                d1 = _rodrigues(bend, alpha, dt) @ nrm
                d2 = _rodrigues(bend, -beta, dt) @ nrm
                G[t, under_thigh] = arc(c1, d1.astype(dt)) @ G[t, under_thigh]
                G[t, under_shin] = arc(c2, d2.astype(dt)) @ G[t, under_shin]
    return G, root - target.offsets[0].astype(dt), s


def channels_of(target, raw, x, R, off, order="ZXY", num=1, den=1, dtype=np.float64, leg_ik=False, variant=None):
    """One sample -> (channels (T_out, 3 + 3 N), the globals at the source frames (T, N, 3, 3)) in ``dtype``."""
    dt = np.dtype(dtype)
    G, root, _ = globals_of(target, raw, x, R, off, dt, leg_ik, variant)
    Lo = np.empty_like(G)
    for n, p in enumerate(target.parent):
        Lo[:, n] = G[:, n] if p < 0 else np.swapaxes(G[:, p], -1, -2) @ G[:, n]
    T = len(G)
    k = np.arange(RR.length_out(T, num, den))
    t0, rem = k * den // num, k * den % num
    t1 = np.where(rem > 0, t0 + 1, t0)
    f = (rem.astype(dt) / dt.type(num))[:, None]
    q = RR.matrix_to_quaternion(Lo)
    qk = np.where((rem > 0)[:, None, None], RR.slerp(q[t0], q[t1], f[:, None]), q[t0])
    pos = np.where(rem[:, None] > 0, root[t0] + f * (root[t1] - root[t0]), root[t0])
    ang = RR.matrix_to_euler(RR.quaternion_to_matrix(qk), order) * dt.type(180 / np.pi)
    chan = np.concatenate([pos, ang.reshape(len(k), -1)], axis=1)
    assert chan.dtype == dt
    return chan, G


# ---- reading back ----

def read_back(text, target):
    """BVH text -> (the mapped joints' positions (frames, J, 3), every node's position (frames, N, 3) and global rotation
    (frames, N, 3, 3)) by the fp64 text-only reader; a joint on an End Site sits at its node's position + G OFFSET."""
    bvh = RR.parse_bvh(text)
    assert bvh.names == list(target.names) and bvh.parent == list(target.parent)
    pos, G = RR.bvh_fk(bvh)
    N = len(bvh.names)
    joints = np.stack([pos[:, p] if p < N else pos[:, p - N] + G[:, p - N] @ bvh.end_sites[p - N] for p in target.pick], axis=1)
    return joints, pos, G


def yardstick(MRig, target, raw, joints, R, offs, lengths, order="ZXY", num=1, den=1, leg_ik=False):
    """Over a batch: per sample the truth (joints, positions, globals) read back from the fp64 restatement's text, and the
    yardsticks (joints, globals): how far the fp32 restatement's text reads back from it."""
    truth, yj, yg = [], 0.0, 0.0
    for b, n in enumerate(lengths):
        got = []
        for dt in (np.float64, np.float32):
            chan = channels_of(target, raw, joints[b][:n], R[b][:n], offs[b], order, num, den, dt, leg_ik)[0]
            got.append(read_back(MRig.target_bvh_text(target, chan, len(chan), 0.05, euler=order), target))
        truth.append(got[0])
        yj, yg = max(yj, float(np.abs(got[1][0] - got[0][0]).max())), max(yg, float(np.abs(got[1][2] - got[0][2]).max()))
    return truth, yj, yg

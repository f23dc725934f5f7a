"""Numpy restatement of the rig export, shared by tests/test_motion_rig_host.py and tests/test_motion_rig_gpu.py.

Independent of motion_rig.py and csrc/motion_rig.hip but for the node tree, which is data (``rig_of``'s tables, checked on their
own in the host tests): local rotations, matrix -> quaternion -> slerp -> matrix -> Euler angles, all in the dtype asked for
(float64: the truth; float32: the yardstick), and a BVH reader that knows nothing of the rig beyond what the text says: it
parses HIERARCHY and MOTION and runs G = G_parent R_A R_B R_C, pos = pos_parent + G_parent OFFSET.

``variant`` builds the mistakes an implementation most easily makes (tests/test_motion_rig_host.py measures how far each lies
from the truth): "right_division" (L = G G_parent^T), "reversed" (the angles of R_C R_B R_A written as a, b, c), "radians",
"arms_from_root" (a helper below a joint other than the root turned against the root), "no_flip" (slerp without the hemisphere
flip); ``without_helpers`` is the rig of the remaining one.
"""
from types import SimpleNamespace

import numpy as np

ORDERS = ("XYZ", "XZY", "YXZ", "YZX", "ZXY", "ZYX")


def resolved(rig):
    """Per node the joint whose R is the node's global rotation: its own carried one, else its parent node's; -1: identity."""
    src = []
    for n, c in enumerate(rig.carried):
        src.append(c if c >= 0 else (src[rig.parent[n]] if rig.parent[n] >= 0 else -1))
    return src


def global_rotations(rig, R):
    """R (T, J, 3, 3) -> the nodes' global rotations (T, N, 3, 3)."""
    eye = np.broadcast_to(np.eye(3, dtype=R.dtype), R[:, 0].shape)
    return np.stack([R[:, s] if s >= 0 else eye for s in resolved(rig)], axis=1)


def local_rotations(rig, R, variant=None):
    G = global_rotations(rig, R)
    L = np.empty_like(G)
    for n, p in enumerate(rig.parent):
        if p < 0:
            L[:, n] = G[:, n]
            continue
        P = G[:, p]
        if variant == "arms_from_root" and rig.joint_of[n] < 0 and rig.joint_of[p] != 0:
            P = G[:, 0]
        Pt = np.swapaxes(P, -1, -2)
        L[:, n] = G[:, n] @ Pt if variant == "right_division" else Pt @ G[:, n]
    return L


def matrix_to_quaternion(M):
    """(..., 3, 3) -> unit (w, x, y, z) with w >= 0: of 4 w^2, 4 x^2, 4 y^2, 4 z^2 the largest (>= 1) picks the row."""
    m = lambda r, c: M[..., r, c]
    cand = np.stack([
        np.stack([1 + m(0, 0) + m(1, 1) + m(2, 2), m(2, 1) - m(1, 2), m(0, 2) - m(2, 0), m(1, 0) - m(0, 1)], -1),
        np.stack([m(2, 1) - m(1, 2), 1 + m(0, 0) - m(1, 1) - m(2, 2), m(0, 1) + m(1, 0), m(0, 2) + m(2, 0)], -1),
        np.stack([m(0, 2) - m(2, 0), m(0, 1) + m(1, 0), 1 - m(0, 0) + m(1, 1) - m(2, 2), m(1, 2) + m(2, 1)], -1),
        np.stack([m(1, 0) - m(0, 1), m(0, 2) + m(2, 0), m(1, 2) + m(2, 1), 1 - m(0, 0) - m(1, 1) + m(2, 2)], -1)], -2)
    pick = np.argmax(np.stack([cand[..., i, i] for i in range(4)], -1), -1)
    q = np.take_along_axis(cand, pick[..., None, None], -2)[..., 0, :]
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    return np.where(q[..., :1] < 0, -q, q).astype(M.dtype)


def quaternion_to_matrix(q):
    w, x, y, z = (q[..., i] for i in range(4))
    rows = [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
            [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
            [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]
    return np.stack([np.stack(r, -1) for r in rows], -2)


def slerp(q0, q1, f, flip=True):
    """Unit quaternions (..., 4), f (..., 1) in [0, 1], in the quaternions' dtype."""
    d = (q0 * q1).sum(-1, keepdims=True)
    if flip:
        q1 = np.where(d < 0, -q1, q1)
        d = np.abs(d)
    th = np.arccos(np.clip(d, -1, 1))
    s = np.sin(th)
    near = s < 1e-4  # the two nearly coincide: lerp (off by th^3 / 20 at most)
    s = np.where(near, s.dtype.type(1), s)
    w0 = np.where(near, 1 - f, np.sin((1 - f) * th) / s)
    w1 = np.where(near, f, np.sin(f * th) / s)
    q = w0 * q0 + w1 * q1
    return (q / np.linalg.norm(q, axis=-1, keepdims=True)).astype(q0.dtype)


def _axes(order):
    i, j, k = ("XYZ".index(ch) for ch in order)
    return i, j, k, (1 if (j - i) % 3 == 1 else -1)


def matrix_to_euler(M, order):
    """(..., 3, 3) -> radians (a, b, c) of M = R_A(a) R_B(b) R_C(c): M[A][C] = +-sin b, the row A and the column C hold the
    rest; at the gimbal c = 0 and a comes from the other 2 x 2 block."""
    i, j, k, sg = _axes(order)
    sb = np.clip(sg * M[..., i, k], -1, 1)
    gimbal = np.abs(sb) > 1 - 4 * np.finfo(M.dtype).eps
    b = np.arcsin(sb)
    c = np.where(gimbal, M.dtype.type(0), np.arctan2(-sg * M[..., i, j], M[..., i, i]))
    a = np.where(gimbal, np.arctan2(sg * M[..., k, j], M[..., j, j]), np.arctan2(-sg * M[..., j, k], M[..., k, k]))
    return np.stack([a, b, c], -1).astype(M.dtype)


def axis_rotation(axis, ang):
    """The rotation by ``ang`` radians (...,) about X, Y or Z (0, 1, 2): (..., 3, 3)."""
    c, s = np.cos(ang), np.sin(ang)
    o, z = np.ones_like(c), np.zeros_like(c)
    rows = {0: [[o, z, z], [z, c, -s], [z, s, c]], 1: [[c, z, s], [z, o, z], [-s, z, c]], 2: [[c, -s, z], [s, c, z], [z, z, o]]}[axis]
    return np.stack([np.stack(r, -1) for r in rows], -2)


def euler_to_matrix(rad, order):
    A, B, C = ("XYZ".index(ch) for ch in order)
    return axis_rotation(A, rad[..., 0]) @ axis_rotation(B, rad[..., 1]) @ axis_rotation(C, rad[..., 2])


def length_out(n, num, den):
    return (n - 1) * num // den + 1


def rig_channels(rig, joints, R, order="ZXY", scale=1.0, num=1, den=1, dtype=np.float64, variant=None):
    """One sample: joints (T, J, 3), R (T, J, 3, 3) -> (channels (T_out, 3 + 3 N), local quaternions (T_out, N, 4))."""
    dtype = np.dtype(dtype)
    joints, R = np.asarray(joints).astype(dtype), np.asarray(R).astype(dtype)
    T = len(R)
    k = np.arange(length_out(T, num, den))
    t0, rem = k * den // num, k * den % num
    t1 = np.where(rem > 0, t0 + 1, t0)  # frame t0 + 1 only where it is needed
    assert t1.max() < T
    f = (rem.astype(dtype) / dtype.type(num))[:, None]
    q = matrix_to_quaternion(local_rotations(rig, R, variant))
    qk = np.where((rem > 0)[:, None, None], slerp(q[t0], q[t1], f[:, None], flip=variant != "no_flip"), q[t0])
    pos = np.where(rem[:, None] > 0, joints[t0, 0] + f * (joints[t1, 0] - joints[t0, 0]), joints[t0, 0])
    M = quaternion_to_matrix(qk)
    ang = matrix_to_euler(M, order[::-1])[..., ::-1] if variant == "reversed" else matrix_to_euler(M, order)
    if variant != "radians":
        ang = ang * dtype.type(180 / np.pi)
    chan = np.concatenate([dtype.type(scale) * pos, ang.reshape(len(k), -1)], axis=1)
    assert chan.dtype == dtype and qk.dtype == dtype
    return chan, qk


def without_helpers(rig):
    """The rig of the mistake "branching joints have no helper nodes": one node per joint, the children of a branching joint
    hang off its node and so turn with the R that it carries."""
    keep = [n for n, j in enumerate(rig.joint_of) if j >= 0]
    new = {n: i for i, n in enumerate(keep)}

    def up(n):
        p = rig.parent[n]
        return -1 if p < 0 else (new[p] if p in new else up(p))

    return SimpleNamespace(names=[rig.names[n] for n in keep], parent=[up(n) for n in keep], carried=[rig.carried[n] for n in keep],
                           joint_of=[rig.joint_of[n] for n in keep], has_offset=[rig.has_offset[n] for n in keep],
                           joints=rig.joints, n_nodes=len(keep))


def parse_bvh(text, dtype=np.float64):
    """BVH text -> namespace: names, parent, offsets (N, 3), channels (per node the channel names), end_sites {node: offset},
    frames, frame_time, values (frames, number of channels) in ``dtype``."""
    lines = [ln.split() for ln in text.splitlines() if ln.strip()]
    assert lines[0] == ["HIERARCHY"]
    names, parent, offsets, channels, ends, stack, pending, i = [], [], [], [], {}, [], None, 1
    while lines[i] != ["MOTION"]:
        w = lines[i]
        if w[0] in ("ROOT", "JOINT"):
            assert (w[0] == "ROOT") == (not stack)
            names.append(w[1]), parent.append(stack[-1] if stack else -1), offsets.append(None), channels.append([])
            pending = len(names) - 1
        elif w[:2] == ["End", "Site"]:
            pending = "end"
        elif w == ["{"]:
            stack.append(pending)
        elif w == ["}"]:
            stack.pop()
        elif w[0] == "OFFSET":
            v = np.array([float(x) for x in w[1:4]], dtype)
            if stack[-1] == "end":
                ends[stack[-2]] = v
            else:
                offsets[stack[-1]] = v
        elif w[0] == "CHANNELS":
            assert int(w[1]) == len(w) - 2
            channels[stack[-1]] = w[2:]
        else:
            raise AssertionError(w)
        i += 1
    assert not stack
    assert lines[i + 1][0] == "Frames:" and lines[i + 2][:2] == ["Frame", "Time:"]
    frames, frame_time = int(lines[i + 1][1]), float(lines[i + 2][2])
    rows = lines[i + 3:]
    width = sum(len(c) for c in channels)
    assert len(rows) == frames and all(len(r) == width for r in rows)
    values = np.array([[float(x) for x in r] for r in rows], dtype).reshape(frames, width)
    return SimpleNamespace(names=names, parent=parent, offsets=np.stack(offsets), channels=channels, end_sites=ends,
                           frames=frames, frame_time=frame_time, values=values)


def bvh_fk(bvh, dtype=np.float64):
    """What a BVH reader computes: -> (positions (frames, N, 3), global rotations (frames, N, 3, 3))."""
    dtype = np.dtype(dtype)
    v = bvh.values.astype(dtype)
    n = len(v)
    pos, G, col = [], [], 0
    for node, p in enumerate(bvh.parent):
        Gp = G[p] if p >= 0 else np.broadcast_to(np.eye(3, dtype=dtype), (n, 3, 3))
        at = (pos[p] if p >= 0 else np.zeros((n, 3), dtype)) + Gp @ bvh.offsets[node].astype(dtype)
        Rl = np.broadcast_to(np.eye(3, dtype=dtype), (n, 3, 3))
        for name in bvh.channels[node]:
            axis = "XYZ".index(name[0])
            if name[1:] == "position":
                at = at + v[:, col, None] * np.eye(3, dtype=dtype)[axis]
            else:
                assert name[1:] == "rotation"
                Rl = Rl @ axis_rotation(axis, v[:, col] * dtype.type(np.pi / 180))
            col += 1
        pos.append(at), G.append(Gp @ Rl)
    return np.stack(pos, 1), np.stack(G, 1)


def read_back(text, rig):
    """BVH text -> (joints (frames, J, 3), the nodes' global rotations (frames, N, 3, 3)) by the fp64 reader; the text's nodes
    are the rig's, in its order."""
    bvh = parse_bvh(text)
    assert bvh.names == list(rig.names) and bvh.parent == list(rig.parent)
    pos, G = bvh_fk(bvh)
    at = {j: n for n, j in enumerate(rig.joint_of) if j >= 0}
    return pos[:, [at[j] for j in range(rig.joints)]], G


def yardstick(bvh_text, rig, offsets, joints, R, lengths, order="ZXY", scale=1.0, num=1, den=1):
    """Over a batch (joints (B, T, J, 3), R (B, T, J, 3, 3), lengths): the truth per sample, (joints, globals) read back from the
    fp64 restatement's text, and the yardsticks (joints, globals): how far the fp32 restatement's text reads back from it."""
    truth, yj, yg = [], 0.0, 0.0
    for b, n in enumerate(lengths):
        got = []
        for dt in (np.float64, np.float32):
            chan = rig_channels(rig, joints[b][:n], R[b][:n], order, scale, num, den, dt)[0]
            got.append(read_back(bvh_text(rig, offsets, chan, len(chan), 0.05, euler=order, scale=scale), rig))
        truth.append(got[0])
        yj, yg = max(yj, float(np.abs(got[1][0] - got[0][0]).max())), max(yg, float(np.abs(got[1][1] - got[0][1]).max()))
    return truth, yj, yg


def rodrigues(axis, ang):
    """Unit axes (..., 3), angles (...,) in radians -> rotation matrices (..., 3, 3)."""
    x, y, z = (axis[..., i] for i in range(3))
    o = np.zeros_like(x)
    K = np.stack([np.stack([o, -z, y], -1), np.stack([z, o, -x], -1), np.stack([-y, x, o], -1)], -2)
    s, c = np.sin(ang)[..., None, None], np.cos(ang)[..., None, None]
    return np.eye(3) + s * K + (1 - c) * (K @ K)


def spin_clip(rig, offsets, T, seed, turning=None, span=(170.0, 190.0)):
    """A clip by construction, fp64: every node that carries a rotation of its own turns about one fixed axis of its own at a constant rate
    of its own (2 .. 12 degrees a frame), so the slerp between two frames is the motion itself; node ``turning``'s angle runs
    over ``span`` degrees across the clip instead (through 180 degrees, where the canonical quaternion changes sign).  The
    root walks a straight line.  -> (joints (T, J, 3), R (T, J, 3, 3), local_at), local_at(tau) being the analytic local
    rotations (N, 3, 3) and root position at the frame time tau (a float)."""
    rs = np.random.RandomState(seed)
    N = rig.n_nodes
    axis = rs.randn(N, 3)
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    rate, phase = np.deg2rad(rs.uniform(2, 12, N)) * rs.choice([-1, 1], N), rs.uniform(-1, 1, N)
    if turning is not None:
        phase[turning], rate[turning] = np.deg2rad(span[0]), np.deg2rad(span[1] - span[0]) / max(T - 1, 1)
    src = resolved(rig)  # a branching joint's node carries the R that the node above it carries already: it does not turn
    turns = np.array([c >= 0 and (p < 0 or src[p] != c) for c, p in zip(rig.carried, rig.parent)])
    start, step = rs.uniform(-1, 1, 3), np.array([0.03, 0.002, 0.05])
    offsets = np.asarray(offsets, np.float64)

    def local_at(tau):
        return np.where(turns[:, None, None], rodrigues(axis, phase + rate * tau), np.eye(3)), start + step * tau

    joints, R = np.zeros((T, rig.joints, 3)), np.zeros((T, rig.joints, 3, 3))
    R[:] = np.eye(3)
    parent_joint = {}
    for n, j in enumerate(rig.joint_of):  # the joint above each joint, through the helpers
        if j > 0:
            p = rig.parent[n]
            while rig.joint_of[p] < 0:
                p = rig.parent[p]
            parent_joint[j] = rig.joint_of[p]
    for t in range(T):
        L, joints[t, 0] = local_at(float(t))
        G = [None] * N
        for n, p in enumerate(rig.parent):
            G[n] = L[n] if p < 0 else G[p] @ L[n]
            if rig.carried[n] >= 0:
                R[t, rig.carried[n]] = G[n]
        for n, j in enumerate(rig.joint_of):  # nodes come parents first, and so do their joints
            if j > 0:
                joints[t, j] = joints[t, parent_joint[j]] + R[t, j] @ offsets[j]
    return joints, R, local_at

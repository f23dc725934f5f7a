"""CPU restatement of the reference's joints -> feature rows pipeline (TEST INFRASTRUCTURE ONLY).

Follows, for the HumanML3D 22-joint (263-d) and KIT 21-joint (251-d) representations:
  * uniform_skeleton / process_file / extract_features                              utils/motion_process.py:13-36,39-166,169-218
  * Skeleton.get_offsets_joints / inverse_kinematics_np / forward_kinematics_np     utils/skeleton.py:43-51,55-101,126-147
  * qinv / qmul / qrot / qbetween / quaternion_to_matrix / quaternion_to_cont6d     utils/quaternion.py
Two things are reproduced as the reference has them, because its training data was made with them: every kinematic chain
starts its accumulated rotation from the ROOT quaternion (also the arm chains that start at the upper spine), and the
inverse kinematics reads the face joints as (l_hip, r_hip, sdr_r, sdr_l) from a list ordered (r_hip, l_hip, sdr_r, sdr_l).

Precision: the reference's quaternion helpers always run in fp32 torch; what it does in numpy follows the dtype of its input
(fp64 clips: differences, normalisations and the facing-direction filter in fp64).  ``all32=False`` keeps that mix for an
fp64 input (pinned by tests/golden/motion_features.npz, tools/make_motion_features_golden.py); ``all32=True`` rounds the
input to fp32 and keeps every numpy step in fp32: what an fp32 device kernel can be held to.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch
from scipy.ndimage import gaussian_filter1d

FORWARD_SIGMA = 20  # skeleton.py:68


def skeleton_from_tables(chains, raw_offsets, face, feet, legs):
    chains = [list(map(int, c)) for c in chains]
    raw = np.asarray(raw_offsets, dtype=np.float32)
    parents = [0] * len(raw)
    parents[0] = -1
    for c in chains:
        for a, b in zip(c[:-1], c[1:]):
            parents[b] = a
    return SimpleNamespace(chains=chains, raw=raw, face=tuple(map(int, face)), feet=tuple(map(int, feet)),
                           legs=tuple(map(int, legs)), parents=parents, J=len(raw))


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).float()


def qinv(q):
    return q * torch.tensor([1.0, -1.0, -1.0, -1.0])


def qmul(q, r):
    # products r_i * q_j of the reference's outer product, summed in its order (quaternion.py:45-50)
    t = lambda i, j: r[..., i] * q[..., j]  # noqa: E731
    w = t(0, 0) - t(1, 1) - t(2, 2) - t(3, 3)
    x = t(0, 1) + t(1, 0) - t(2, 3) + t(3, 2)
    y = t(0, 2) + t(1, 3) + t(2, 0) - t(3, 1)
    z = t(0, 3) - t(1, 2) + t(2, 1) + t(3, 0)
    return torch.stack((w, x, y, z), dim=-1)


def qrot(q, v):
    qvec = q[..., 1:]
    uv = torch.cross(qvec, v, dim=-1)
    uuv = torch.cross(qvec, uv, dim=-1)
    return v + 2 * (q[..., :1] * uv + uuv)


def qbetween(v0, v1):
    v = torch.cross(v0, v1, dim=-1)
    w = torch.sqrt((v0 ** 2).sum(-1, keepdim=True) * (v1 ** 2).sum(-1, keepdim=True)) + (v0 * v1).sum(-1, keepdim=True)
    q = torch.cat([w, v], dim=-1)
    return q / torch.norm(q, dim=-1, keepdim=True)


def quat_to_cont6d(q):
    r, i, j, k = torch.unbind(q, -1)
    two_s = 2.0 / (q * q).sum(-1)
    col0 = torch.stack((1 - two_s * (j * j + k * k), two_s * (i * j + k * r), two_s * (i * k - j * r)), -1)
    col1 = torch.stack((two_s * (i * j - k * r), 1 - two_s * (i * i + k * k), two_s * (j * k + i * r)), -1)
    return torch.cat([col0, col1], dim=-1)


def _unit(v):
    return v / np.sqrt((v ** 2).sum(axis=-1))[..., None]


def get_offsets(sk, pose):
    """(J, 3) bone offsets of one pose: each bone's length along its raw axis (skeleton.py:43-51)."""
    off = torch.from_numpy(sk.raw).clone()
    pose = torch.as_tensor(pose)
    for i in range(1, sk.J):
        off[i] = torch.norm(pose[i] - pose[sk.parents[i]], p=2, dim=0) * off[i]
    return off


def inverse_kinematics(sk, joints, smooth, wide):
    """(n, J, 4) local quaternions, fp32 (skeleton.py:55-101); ``wide`` is the dtype of the facing direction."""
    l_hip, r_hip, sdr_r, sdr_l = sk.face  # the reference's unpacking of a list ordered r_hip, l_hip, ...
    across = _unit((joints[:, r_hip] - joints[:, l_hip]) + (joints[:, sdr_r] - joints[:, sdr_l]))
    forward = np.zeros(across.shape, dtype=wide)  # cross((0, 1, 0), across)
    forward[:, 0], forward[:, 2] = across[:, 2], -across[:, 0]
    if smooth:
        forward = gaussian_filter1d(forward, FORWARD_SIGMA, axis=0, mode="nearest")
    forward = _unit(forward)
    target = torch.tensor([[0.0, 0.0, 1.0]]).expand(len(forward), 3)
    root = qbetween(_t(forward), target)
    root[0] = torch.tensor([1.0, 0.0, 0.0, 0.0])
    quats = torch.zeros(joints.shape[:-1] + (4,))
    quats[:, 0] = root
    for chain in sk.chains:
        R = root  # also for the chains that do not start at the root
        for a, b in zip(chain[:-1], chain[1:]):
            u = torch.from_numpy(sk.raw[b])[None].expand(len(joints), 3)
            v = _unit(joints[:, b] - joints[:, a])
            loc = qmul(qinv(R), qbetween(u, _t(v)))
            quats[:, b] = loc
            R = qmul(R, loc)
    return quats


def uniform_skeleton(sk, positions, target_offsets, wide):
    src = get_offsets(sk, positions[0]).numpy()
    tgt = np.asarray(target_offsets, dtype=np.float32)
    l1, l2 = sk.legs
    scale = (np.abs(tgt[l1]).max() + np.abs(tgt[l2]).max()) / (np.abs(src[l1]).max() + np.abs(src[l2]).max())
    quats = inverse_kinematics(sk, positions, False, wide)
    out = np.zeros(positions.shape, dtype=wide)
    out[:, 0] = positions[:, 0] * scale
    tgt_t = torch.from_numpy(tgt)
    for chain in sk.chains:
        R = quats[:, 0]
        for a, b in zip(chain[:-1], chain[1:]):
            R = qmul(R, quats[:, b])
            out[:, b] = qrot(R, tgt_t[b][None].expand(len(out), 3)).numpy() + out[:, a]
    return out


def canonicalize(sk, positions, target_offsets=None, all32=False):
    """process_file up to ``global_positions`` (motion_process.py:169-218): fp32 (n, J, 3)."""
    wide = np.float32 if all32 else np.float64
    positions = np.array(positions, dtype=wide)
    if target_offsets is not None:
        positions = uniform_skeleton(sk, positions, target_offsets, wide)
    positions[:, :, 1] -= positions[:, :, 1].min()
    init = positions[0]
    positions = positions - init[0] * np.array([1, 0, 1], dtype=wide)
    r_hip, l_hip, sdr_r, sdr_l = sk.face
    across = _unit((init[r_hip] - init[l_hip]) + (init[sdr_r] - init[sdr_l]))
    forward = _unit(np.array([across[2], 0, -across[0]], dtype=wide))
    q = qbetween(_t(forward[None]), torch.tensor([[0.0, 0.0, 1.0]]))
    return qrot(q[None].expand(positions.shape[:-1] + (4,)), _t(positions)).numpy()


def extract_features(sk, positions, feet_thre, all32=False):
    """(n, J, 3) -> (n - 1, 12 J - 1) rows (motion_process.py:39-166)."""
    positions = np.asarray(positions)
    if all32:
        positions = positions.astype(np.float32)
    wide = np.float32 if all32 else np.float64
    glob = positions.copy()
    feet = list(sk.feet)
    d = ((positions[1:, feet] - positions[:-1, feet]) ** 2)
    speed2 = d[..., 0] + d[..., 1] + d[..., 2]
    contacts = (speed2 < np.float64(feet_thre)).astype(positions.dtype)
    quats = inverse_kinematics(sk, positions, True, wide)
    cont6d = quat_to_cont6d(quats).numpy()
    r_rot = quats[:, 0].clone()
    velocity = qrot(r_rot[1:], _t(positions[1:, 0] - positions[:-1, 0])).numpy()
    r_velocity = qmul(r_rot[1:], qinv(r_rot[:-1])).numpy()
    local = positions.copy()
    local[..., 0] -= local[:, 0:1, 0]
    local[..., 2] -= local[:, 0:1, 2]
    local = qrot(r_rot[:, None].expand(local.shape[:-1] + (4,)), _t(local)).numpy()
    root = np.concatenate([np.arcsin(r_velocity[:, 2:3]), velocity[:, [0, 2]], local[:-1, 0, 1:2]], axis=-1)
    ric = local[:, 1:].reshape(len(local), -1)
    rot = cont6d[:, 1:].reshape(len(cont6d), -1)
    vel = qrot(r_rot[:-1, None].expand(glob.shape[0] - 1, glob.shape[1], 4), _t(glob[1:] - glob[:-1])).numpy()
    data = np.concatenate([root, ric[:-1], rot[:-1], vel.reshape(len(vel), -1), contacts], axis=-1)
    return data, speed2


def process_file(sk, positions, feet_thre, target_offsets=None, all32=False):
    """-> (data (n - 1, F), global_positions (n, J, 3) fp32)."""
    glob = canonicalize(sk, positions, target_offsets, all32)
    return extract_features(sk, glob, feet_thre, all32)[0], glob


def joints_to_motion(sk, clips, mean=None, std=None, feet_thre=0.002, canonical=True, target_offsets=None, T=None,
                     all32=True):
    """Batch form of the device function: list of (n_i, J, 3) -> rows (B, T - 1, F) and positions (B, T, J, 3), zero past
    each clip; ``(x - mean) / std`` in fp32 on the valid rows."""
    T = T or max(len(c) for c in clips)
    F_ = 12 * sk.J - 1
    rows = np.zeros((len(clips), T - 1, F_), np.float32)
    pos = np.zeros((len(clips), T, sk.J, 3), np.float32)
    for i, c in enumerate(clips):
        c = np.asarray(c)
        g = canonicalize(sk, c, target_offsets, all32) if canonical else c.astype(np.float32)
        d = extract_features(sk, g, feet_thre, all32)[0].astype(np.float32)
        if mean is not None:
            d = (d - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)
        rows[i, :len(c) - 1], pos[i, :len(c)] = d, g
    return rows, pos


GROUPS = ("root", "ric", "rot6d", "vel")


def column_groups(J):
    """name -> slice of the columns compared by tolerance; the last 4 columns (foot contacts) are compared exactly."""
    a, b, c = 4, 4 + 3 * (J - 1), 4 + 9 * (J - 1)
    return {"root": slice(0, a), "ric": slice(a, b), "rot6d": slice(b, c), "vel": slice(c, c + 3 * J)}


def synth_clip(sk, n, seed, turn=1.0):
    """A valid skeleton in motion: forward kinematics of smooth random joint rotations on random bone lengths, with a
    turning, translating root, off the origin, off the floor and not facing Z+.  fp64 (n, J, 3).  The heading drifts by
    0.2 ``turn`` rad/s: clips of 196 frames stay clear of facing away from frame 0, where the reference's root quaternion
    (qbetween towards Z+) is ill-conditioned; pass ``turn=0`` for much longer clips."""
    rng = np.random.RandomState(seed)
    t = np.arange(n) / 20.0
    lengths = 0.1 + 0.3 * rng.rand(sk.J)
    # shoulders wider than hips, as on a person: the inverse kinematics' facing direction is (shoulder width - hip width)
    # along the body's left-right axis (the reproduced slip), and it must not flip or vanish
    for j in range(1, sk.J):
        if sk.raw[j][0] != 0:
            lengths[j] = (0.08 + 0.04 * rng.rand()) if j in sk.face[:2] else (0.2 + 0.05 * rng.rand())

    def smooth(shape, amp):
        k = 3
        f = 0.2 + 1.3 * rng.rand(k, *shape)
        ph = 2 * np.pi * rng.rand(k, *shape)
        a = amp * rng.randn(k, *shape) / k
        return (a[None] * np.sin(2 * np.pi * f[None] * t.reshape((-1,) + (1,) * (len(shape) + 1)) + ph[None])).sum(1)

    def rotmat(rv):  # Rodrigues, (n, 3) -> (n, 3, 3)
        th = np.linalg.norm(rv, axis=-1)[:, None, None] + 1e-12
        k = rv / th[:, :, 0]
        K = np.zeros((len(rv), 3, 3))
        K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -k[:, 2], k[:, 1], k[:, 2], -k[:, 0], -k[:, 1], k[:, 0]
        return np.eye(3)[None] + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)

    heading = rng.uniform(0.6, 2.4) * rng.choice([-1, 1]) + turn * 0.2 * t + smooth((), 0.3)
    yaw = np.zeros((n, 3))
    yaw[:, 1] = heading
    root_R = rotmat(yaw) @ rotmat(smooth((3,), 0.15))
    root = np.stack([rng.uniform(-2, 2) + 0.5 * t * np.cos(0.3 * t) + smooth((), 0.1),
                     rng.uniform(0.9, 1.4) + smooth((), 0.05),
                     rng.uniform(-2, 2) + 0.5 * t * np.sin(0.3 * t) + smooth((), 0.1)], -1)
    out = np.zeros((n, sk.J, 3))
    out[:, 0] = root
    glob = {0: root_R}
    for chain in sk.chains:
        for a, b in zip(chain[:-1], chain[1:]):
            amp = 0.45 if b in sk.feet or a in sk.feet else 0.3
            glob[b] = glob[a] @ rotmat(smooth((3,), amp))
            out[:, b] = out[:, a] + (glob[b] @ (sk.raw[b].astype(np.float64) * lengths[b])[None, :, None])[..., 0]
    return out

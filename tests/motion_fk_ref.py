"""CPU restatement of the reference's rows -> joints by forward kinematics (TEST INFRASTRUCTURE ONLY).

Follows, for the HumanML3D 22-joint (263-d) and KIT 21-joint (251-d) representations:
  * recover_root_rot_pos / recover_from_rot                                          utils/motion_process.py:362-398
  * Skeleton.forward_kinematics_cont6d                                               utils/skeleton.py:173-194
  * quaternion_to_matrix / quaternion_to_cont6d / cont6d_to_matrix                   utils/quaternion.py:274-336
``dtype=torch.float32`` keeps the reference's operation order in fp32 torch (pinned against the reference's own output by
tests/golden/motion_fk.npz); ``torch.float64`` is the same arithmetic in double: the truth every fp32 result, the
reference's included, is measured against.  Every kinematic chain starts its accumulated rotation from the ROOT matrix,
also the arm chains that start at the upper spine.

``WRONG`` names the mistakes an implementation most easily makes; ``recover_from_rot(..., wrong=name)`` makes one of them, so
that a test can show that its inputs tell each from the truth.
"""
from __future__ import annotations

import numpy as np
import torch
from scipy.ndimage import gaussian_filter1d

WRONG = ("arm_from_spine",   # a chain that starts at another joint takes that joint's accumulated rotation
         "z_flipped",        # z = y_raw x x
         "rows",             # x, y, z taken as the matrix's rows
         "left_multiply",    # R <- M R
         "root_inverted",    # the root quaternion conjugated
         "ric_offset")       # the rot6d block read where the ric block starts


def recover_root(data, wrong=None):
    """data (T, F) torch -> (root quaternion (T, 4), root position (T, 3)) in data's dtype (motion_process.py:362-382)."""
    rot_vel = data[..., 0]
    ang = torch.zeros_like(rot_vel)
    ang[1:] = rot_vel[:-1]
    ang = torch.cumsum(ang, dim=-1)
    quat = torch.zeros(data.shape[:-1] + (4,), dtype=data.dtype)
    quat[..., 0] = torch.cos(ang)
    quat[..., 2] = torch.sin(ang)
    pos = torch.zeros(data.shape[:-1] + (3,), dtype=data.dtype)
    pos[1:, 0], pos[1:, 2] = data[:-1, 1], data[:-1, 2]
    pos = qrot(quat * torch.tensor([1.0, -1.0, -1.0, -1.0], dtype=data.dtype), pos)
    pos = torch.cumsum(pos, dim=-2)
    pos[..., 1] = data[..., 3]
    if wrong == "root_inverted":
        quat = quat * torch.tensor([1.0, -1.0, -1.0, -1.0], dtype=data.dtype)
    return quat, pos


def qrot(q, v):
    qvec = q[..., 1:]
    uv = torch.cross(qvec, v, dim=-1)
    uuv = torch.cross(qvec, uv, dim=-1)
    return v + 2 * (q[..., :1] * uv + uuv)


def quaternion_to_cont6d(q):
    r, i, j, k = torch.unbind(q, -1)
    two_s = 2.0 / (q * q).sum(-1)
    col0 = torch.stack((1 - two_s * (j * j + k * k), two_s * (i * j + k * r), two_s * (i * k - j * r)), -1)
    col1 = torch.stack((two_s * (i * j - k * r), 1 - two_s * (i * i + k * k), two_s * (j * k + i * r)), -1)
    return torch.cat([col0, col1], dim=-1)


def cont6d_to_matrix(c, wrong=None):
    x_raw, y_raw = c[..., 0:3], c[..., 3:6]
    x = x_raw / torch.norm(x_raw, dim=-1, keepdim=True)
    z = torch.cross(y_raw, x, dim=-1) if wrong == "z_flipped" else torch.cross(x, y_raw, dim=-1)
    z = z / torch.norm(z, dim=-1, keepdim=True)
    y = torch.cross(z, x, dim=-1)
    return torch.stack([x, y, z], dim=-2 if wrong == "rows" else -1)


def gram_schmidt_margins(sk, data):
    """Smallest |x_raw| and |x_raw x y_raw| over the rot6d pairs of de-normalised rows (T, F): what bounds the conditioning of
    cont6d_to_matrix."""
    J = sk.J
    c = torch.as_tensor(np.asarray(data), dtype=torch.float64)[..., 4 + 3 * (J - 1):4 + 9 * (J - 1)].reshape(-1, 6)
    return float(torch.norm(c[:, :3], dim=-1).min()), float(torch.norm(torch.cross(c[:, :3], c[:, 3:], dim=-1), dim=-1).min())


def recover_from_rot(sk, data, offsets, dtype=torch.float32, wrong=None, return_rotations=False):
    """De-normalised rows (T, F) and bone offsets (J, 3) -> joints (T, J, 3) numpy [, global rotations (T, J, 3, 3)]."""
    J = sk.J
    data = torch.as_tensor(np.asarray(data)).to(dtype)
    off = torch.as_tensor(np.asarray(offsets)).to(dtype)
    quat, r_pos = recover_root(data, wrong)
    start = 4 if wrong == "ric_offset" else 4 + (J - 1) * 3
    cont6d = torch.cat([quaternion_to_cont6d(quat), data[..., start:start + (J - 1) * 6]], dim=-1).reshape(-1, J, 6)
    mats = cont6d_to_matrix(cont6d, wrong)
    joints = torch.zeros(cont6d.shape[:-1] + (3,), dtype=dtype)
    rots = torch.zeros(cont6d.shape[:-1] + (3, 3), dtype=dtype)
    joints[:, 0] = r_pos
    rots[:, 0] = mats[:, 0]
    for chain in sk.chains:
        R = mats[:, 0]
        if wrong == "arm_from_spine" and chain[0] != 0:
            R = rots[:, chain[0]]
        for a, b in zip(chain[:-1], chain[1:]):
            R = torch.matmul(mats[:, b], R) if wrong == "left_multiply" else torch.matmul(R, mats[:, b])
            joints[:, b] = torch.matmul(R, off[b][None, :, None].expand(len(R), 3, 1)).squeeze(-1) + joints[:, a]
            rots[:, b] = R
    return (joints.numpy(), rots.numpy()) if return_rotations else joints.numpy()


def recover_from_ric(sk, data, dtype=torch.float32):
    """De-normalised rows (T, F) -> joints (T, J, 3) numpy from the position columns (motion_process.py:401-416)."""
    data = torch.as_tensor(np.asarray(data)).to(dtype)
    quat, r_pos = recover_root(data)
    p = data[..., 4:(sk.J - 1) * 3 + 4].reshape(len(data), -1, 3)
    p = qrot((quat * torch.tensor([1.0, -1.0, -1.0, -1.0], dtype=dtype))[:, None].expand(p.shape[:-1] + (4,)), p)
    p[..., 0] += r_pos[..., 0:1]
    p[..., 2] += r_pos[..., 2:3]
    return torch.cat([r_pos[:, None], p], dim=-2).numpy()


def mean_bone_offsets(sk, data, dtype=torch.float32):
    """(J, 3) offsets that make a clip's bones rigid: each bone's mean length over the frames of de-normalised rows (T, F) on
    its recover_from_ric joints (per frame in ``dtype``, summed in double in frame order), times the bone's axis."""
    p = recover_from_ric(sk, data, dtype)
    par = np.asarray(sk.parents[1:])
    d = p[:, 1:] - p[:, par]
    lens = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])
    acc = np.zeros(sk.J - 1, np.float64)
    for row in lens:
        acc += row.astype(np.float64)
    out = sk.raw.astype(p.dtype).copy()
    out[1:] = (acc / len(lens)).astype(p.dtype)[:, None] * out[1:]
    return out


def motion_to_joints_fk(sk, rows, mean, std, lengths=None, offsets=None, sigma=0.0, dtype=torch.float32, wrong=None):
    """Batch form of the device function: normalised rows (B, T, F) -> (joints (B, T, J, 3), rotations (B, T, J, 3, 3),
    offsets (B, J, 3)), zero past each length; ``offsets`` (J, 3), (B, J, 3) or None (each sample's mean bone lengths);
    ``sigma`` filters the joints over the valid frames ("nearest" edges).  ``dtype`` is that of the arithmetic after the fp32
    de-normalisation ``rows * std + mean``."""
    np_t = np.float32 if dtype == torch.float32 else np.float64
    rows = np.asarray(rows)
    B, T, _ = rows.shape
    # de-normalised in fp32 whatever the dtype: the fp32 rows are the input, as they are for the reference
    data = (rows.astype(np.float32) * np.asarray(std, np.float32) + np.asarray(mean, np.float32)).astype(np_t)
    lengths = [T] * B if lengths is None else [int(n) for n in lengths]
    joints, rots, offs = np.zeros((B, T, sk.J, 3), np_t), np.zeros((B, T, sk.J, 3, 3), np_t), np.zeros((B, sk.J, 3), np_t)
    for b, n in enumerate(lengths):
        if offsets is None:
            offs[b] = mean_bone_offsets(sk, data[b, :n], dtype)
        else:
            o = np.asarray(offsets)
            offs[b] = o if o.ndim == 2 else o[b]
        j, r = recover_from_rot(sk, data[b, :n], offs[b], dtype, wrong, return_rotations=True)
        if sigma and sigma > 0:
            j = gaussian_filter1d(j, sigma, axis=0, mode="nearest")
        joints[b, :n], rots[b, :n] = j, r
    return joints, rots, offs

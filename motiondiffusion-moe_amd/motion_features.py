"""Joint positions -> feature rows on the device: the inverse of ``postprocess.motion_to_joints``.

Host side of ``mdm_motion_features`` (csrc/motion_features.hip), which restates the reference's dataset pipeline
(utils/motion_process.py ``process_file`` / ``extract_features``, utils/skeleton.py, utils/quaternion.py): a clip of n
joint frames (n, J, 3) becomes n - 1 rows ``root 4 | ric (J-1) 3 | rot6d (J-1) 6 | local velocity J 3 | foot contacts 4``
(the last frame only supplies velocities).  All arithmetic is in the kernel; no eager fallback.

The skeleton is data (``SKELETONS``): the HumanML3D 22-joint tree ("t2m", F = 263) named after ``motion_edit.SMPL_JOINTS``
and the KIT 21-joint tree ("kit", F = 251).
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from .motion_edit import FOOT_CONTACT_JOINTS, SMPL_JOINTS
from .postprocess import gaussian_taps, motion_to_joints

FORWARD_SIGMA = 20.0  # the facing direction's temporal filter (utils/skeleton.py:68)


def max_frames() -> int:
    """The longest clip ``mdm_motion_features`` takes (16 bytes of LDS per frame); longer ones are MDM_ERR_UNSUPPORTED."""
    return int(L.lib().mdm_motion_features_max_frames())

_X, _Y, _Z = (1, 0, 0), (0, 1, 0), (0, 0, 1)


def _neg(a):
    return tuple(-v for v in a)


def _skeleton(chains, raw_offsets, face, feet, legs, feet_thre):
    parents = [-1] + [0] * (len(raw_offsets) - 1)
    for c in chains:
        for a, b in zip(c[:-1], c[1:]):
            parents[b] = a
    return SimpleNamespace(chains=tuple(tuple(c) for c in chains), raw_offsets=np.asarray(raw_offsets, dtype=np.float32),
                           face=tuple(face), feet=tuple(feet), legs=tuple(legs), parents=tuple(parents),
                           joints=len(raw_offsets), feats=12 * len(raw_offsets) - 1, feet_thre=feet_thre)


def _t2m():
    j = {n: i for i, n in enumerate(SMPL_JOINTS)}
    # the tree as parent-ordered chains (right leg, left leg, spine, right arm, left arm; the arms hang off spine3) and
    # the rest-pose axis of each joint's bone
    names = (("pelvis", "right_hip", "right_knee", "right_ankle", "right_foot"),
             ("pelvis", "left_hip", "left_knee", "left_ankle", "left_foot"),
             ("pelvis", "spine1", "spine2", "spine3", "neck", "head"),
             ("spine3", "right_collar", "right_shoulder", "right_elbow", "right_wrist"),
             ("spine3", "left_collar", "left_shoulder", "left_elbow", "left_wrist"))
    axis = {"pelvis": (0, 0, 0), "left_hip": _X, "right_hip": _neg(_X), "left_collar": _X, "right_collar": _neg(_X),
            "spine1": _Y, "spine2": _Y, "spine3": _Y, "neck": _Y, "left_foot": _Z, "right_foot": _Z, "head": _Z}
    raw = [axis.get(n, _neg(_Y)) for n in SMPL_JOINTS]  # knees, ankles, shoulders, elbows, wrists: down
    face = [j[n] for n in ("right_hip", "left_hip", "right_shoulder", "left_shoulder")]
    return _skeleton([[j[n] for n in c] for c in names], raw, face, FOOT_CONTACT_JOINTS,
                     (j["right_knee"], j["right_ankle"]), 0.002)


def _kit():
    # KIT-ML: 0 root, 1-4 spine to head, 5-7 / 8-10 arms off joint 3, 11-15 / 16-20 legs (the last two of each: foot joints)
    chains = [[0, 11, 12, 13, 14, 15], [0, 16, 17, 18, 19, 20], [0, 1, 2, 3, 4], [3, 5, 6, 7], [3, 8, 9, 10]]
    down = _neg(_Y)
    raw = [(0, 0, 0), _Y, _Y, _Y, _Y, _X, down, down, _neg(_X), down, down, _X, down, down, _Z, _Z, _neg(_X), down, down,
           _Z, _Z]
    return _skeleton(chains, raw, (11, 16, 5, 8), (19, 20, 14, 15), (17, 18), 0.05)


SKELETONS = {"t2m": _t2m(), "kit": _kit()}


def skeleton_for_feats(dim_pose, strict=False):
    """The name in ``SKELETONS`` of the skeleton whose feature rows are ``dim_pose`` wide (263: "t2m", 251: "kit"); for
    another width None, or with ``strict`` the KeyError of a lookup."""
    names = {sk.feats: name for name, sk in SKELETONS.items()}
    return names[int(dim_pose)] if strict else names.get(int(dim_pose))


def get_skeleton(skeleton):
    if isinstance(skeleton, str):
        if skeleton not in SKELETONS:
            raise ValueError(f"skeleton must be one of {sorted(SKELETONS)}, not {skeleton!r}")
        return SKELETONS[skeleton]
    return skeleton


def _skeleton_struct(sk) -> L.Skeleton:
    s = L.Skeleton()
    entries = [j for c in sk.chains for j in c]
    if sk.joints > L.SKEL_MAX_JOINTS or len(sk.chains) > L.SKEL_MAX_CHAINS or len(entries) > L.SKEL_MAX_CHAIN_ENTRIES:
        raise ValueError("skeleton too large for MdmSkeleton")
    s.joints, s.nchains = sk.joints, len(sk.chains)
    off = 0
    for i, c in enumerate(sk.chains):
        s.chain_offsets[i] = off
        off += len(c)
    s.chain_offsets[len(sk.chains)] = off
    for i, j in enumerate(entries):
        s.chain_joints[i] = j
    for i, v in enumerate(np.asarray(sk.raw_offsets, dtype=np.float32).reshape(-1)):
        s.raw_offsets[i] = float(v)
    for i in range(4):
        s.face[i], s.feet[i] = sk.face[i], sk.feet[i]
    s.legs[0], s.legs[1] = sk.legs
    return s


def pad_clips(clips, J):
    """List of (n_i, J, 3) clips -> ((B, max n, J, 3) float32 zero-padded, lengths (B,) int64); device of the first clip."""
    clips = [torch.as_tensor(c) for c in clips]
    if not clips:
        raise ValueError("no clips given")
    for i, c in enumerate(clips):
        if c.dim() != 3 or tuple(c.shape[1:]) != (J, 3):
            raise ValueError(f"clip {i} of shape {tuple(c.shape)} must be (n, {J}, 3)")
    lens = torch.tensor([c.shape[0] for c in clips], dtype=torch.int64)
    out = torch.zeros((len(clips), int(lens.max()), J, 3), dtype=torch.float32, device=clips[0].device)
    for i, c in enumerate(clips):
        out[i, :c.shape[0]] = c.to(out.device, torch.float32)
    return out, lens


def check_joints(joints, lengths, mean, std, sk, target_offsets=None):
    """Argument checks that need no device: -> (joints (B, T, J, 3) float32, lengths (B,) int64 or None, mean, std float32
    (F,) or None, target_offsets float32 (J, 3) or None).  Raises ValueError."""
    J, F_ = sk.joints, sk.feats
    if isinstance(joints, (list, tuple)):
        if lengths is not None:
            raise ValueError("a list of clips carries its own lengths")
        joints, lengths = pad_clips(joints, J)
    joints = torch.as_tensor(joints)
    if joints.dim() == 3:
        joints = joints[None]
    if joints.dim() != 4 or tuple(joints.shape[2:]) != (J, 3):
        raise ValueError(f"joints of shape {tuple(joints.shape)} must be (B, T, {J}, 3) for this skeleton")
    B, T = joints.shape[:2]
    if T < 2:
        raise ValueError("a clip needs at least 2 frames: n frames give n - 1 rows")
    if lengths is not None:
        lengths = L.check_lengths(lengths, B, T, 2, ": n frames give n - 1 rows")
    joints = joints.to(torch.float32)
    bad = ~torch.isfinite(joints)
    if lengths is not None:  # frames past a clip's length are never read
        bad = bad & (torch.arange(T)[None] < lengths[:, None]).to(joints.device)[..., None, None]
    if bool(bad.any()):
        raise ValueError("joints has non-finite values")
    if (mean is None) != (std is None):
        raise ValueError("mean and std go together: give both or neither")
    if mean is not None:
        mean, std = L.mean_std(mean, std, F_)
    if target_offsets is not None:
        target_offsets = torch.as_tensor(target_offsets).detach().to("cpu", torch.float32)
        if tuple(target_offsets.shape) != (J, 3) or not bool(torch.isfinite(target_offsets).all()):
            raise ValueError(f"target_offsets must be finite and of shape ({J}, 3)")
    return joints, lengths, mean, std, target_offsets


@torch.no_grad()
def joints_to_motion(joints, lengths=None, mean=None, std=None, *, skeleton="t2m", feet_thre=None, canonicalize=True,
                     target_offsets=None, return_positions=False):
    """joints (B, T, J, 3) on a GPU, or a list of ragged (n_i, J, 3) clips -> feature rows (B, T - 1, F), normalised with
    ``mean`` / ``std`` when given; rows at or past ``lengths[b] - 1`` are zero.  ``canonicalize``: put every clip on the
    floor, frame 0's root XZ at the origin, frame 0 facing Z+ (``process_file``); with ``target_offsets`` (J, 3), e.g. from
    ``skeleton_offsets``, re-pose it on those bone offsets first.  ``feet_thre`` defaults to the skeleton's (0.002 t2m,
    0.05 KIT).  ``return_positions``: also the (B, T, J, 3) positions the rows describe (the canonical ones)."""
    sk = get_skeleton(skeleton)
    if target_offsets is not None and not canonicalize:
        raise ValueError("target_offsets needs canonicalize=True (the uniform skeleton is part of process_file)")
    feet_thre = sk.feet_thre if feet_thre is None else float(feet_thre)
    if not feet_thre >= 0:
        raise ValueError("feet_thre must be >= 0")
    x, lengths, mean, std, target_offsets = check_joints(joints, lengths, mean, std, sk, target_offsets)
    L.require_cuda(x)
    dev = x.device
    x = x.contiguous()
    B, T = x.shape[:2]
    ln = None if lengths is None else lengths.to(dev, torch.int32).contiguous()
    mean_t, std_t = (None, None) if mean is None else (mean.to(dev).contiguous(), std.to(dev).contiguous())
    tgt = None if target_offsets is None else target_offsets.to(dev).contiguous()
    w = gaussian_taps(FORWARD_SIGMA)
    w_t = torch.from_numpy(w).to(dev)
    pos = torch.empty_like(x) if canonicalize else None
    out = torch.empty((B, T - 1, sk.feats), dtype=torch.float32, device=dev)
    s = _skeleton_struct(sk)
    with torch.cuda.device(dev):
        L.check(L.lib().mdm_motion_features(
            x.data_ptr(), L.ptr(ln), L.ptr(mean_t), L.ptr(std_t), C.byref(s), L.ptr(tgt), B, T, feet_thre, 1 if canonicalize else 0,
            len(w) - 1, w_t.data_ptr(), L.ptr(pos), out.data_ptr(), L.stream_ptr()), "mdm_motion_features")
    return (out, pos if canonicalize else x) if return_positions else out


def skeleton_offsets(joints_frame, skeleton="t2m") -> torch.Tensor:
    """(J, 3) bone offsets of one pose (J, 3): each bone's length along its axis (``Skeleton.get_offsets_joints``); the
    ``target_offsets`` of ``joints_to_motion``."""
    sk = get_skeleton(skeleton)
    p = torch.as_tensor(joints_frame).detach().to("cpu", torch.float64)
    if tuple(p.shape) != (sk.joints, 3):
        raise ValueError(f"joints_frame of shape {tuple(p.shape)} must be ({sk.joints}, 3)")
    par = torch.tensor(sk.parents[1:])
    off = torch.from_numpy(sk.raw_offsets).clone()
    off[1:] = torch.linalg.vector_norm(p[1:] - p[par], dim=-1).to(torch.float32)[:, None] * off[1:]
    return off


def process_file(positions, feet_thre=None, *, skeleton="t2m", target_offsets=None):
    """Same name / meaning as utils/motion_process.py:169 for one clip (n, J, 3) on a GPU: -> (data (n - 1, F),
    global_positions (n, J, 3)); ``target_offsets`` None leaves the skeleton as it is."""
    data, pos = joints_to_motion(torch.as_tensor(positions)[None], skeleton=skeleton, feet_thre=feet_thre,
                                 target_offsets=target_offsets, return_positions=True)
    return data[0], pos[0]


def extract_features(positions, feet_thre=None, *, skeleton="t2m"):
    """Same name / meaning as utils/motion_process.py:39 for one clip (n, J, 3) on a GPU, taken as it is: (n - 1, F)."""
    return joints_to_motion(torch.as_tensor(positions)[None], skeleton=skeleton, feet_thre=feet_thre, canonicalize=False)[0]


@torch.no_grad()
def refeaturize(motion, mean, std, lengths: Optional[torch.Tensor] = None, *, skeleton="t2m", feet_thre=None):
    """Normalised rows (B, T, F) -> (B, T - 1, F) rows whose every column describes the joints ``recover_from_ric`` shows
    for ``motion``: ``joints_to_motion(motion_to_joints(motion, sigma=0), canonicalize=False)``.  Joint control and
    editing write the root and position columns only; this brings rot6d, velocities and foot contacts back in line."""
    sk = get_skeleton(skeleton)
    j = motion_to_joints(motion, mean, std, lengths, sk.joints, sigma=0.0)
    return joints_to_motion(j, lengths, mean, std, skeleton=sk, feet_thre=feet_thre, canonicalize=False)

"""Masks for motion editing (``DDPMTrainer.generate(..., edit_motion=, edit_mask=)``).

Pure host helpers: each returns a float32 CPU tensor of 0 / 1 that broadcasts against a ``(N, T, F)`` motion, and masks
combine with ``torch.maximum`` (keep what either keeps) or ``*`` (keep what both keep).

The feature layout is HumanML3D's 263-d row for J = 22 joints, in this order:

    root 4 | ric (J-1)*3 | rot6d (J-1)*6 | local velocity J*3 | foot contacts 4

root = (angular velocity about Y, linear velocity X, linear velocity Z, height); ric / rot6d = the root-relative position
and 6-D rotation of joints 1..J-1; local velocity = the velocity of joints 0..J-1; foot contacts = left ankle, left foot,
right ankle, right foot (joints 7, 10, 8, 11).  Joint 0 (the pelvis) owns the root columns and its velocity columns.
"""
from __future__ import annotations

from typing import Iterable

import torch

# the SMPL skeleton's 22 joints, in order
SMPL_JOINTS = ("pelvis", "left_hip", "right_hip", "spine1", "left_knee", "right_knee", "spine2", "left_ankle",
               "right_ankle", "spine3", "left_foot", "right_foot", "neck", "left_collar", "right_collar", "head",
               "left_shoulder", "right_shoulder", "left_elbow", "right_elbow", "left_wrist", "right_wrist")
LOWER_BODY = (0, 1, 2, 4, 5, 7, 8, 10, 11)                       # pelvis, legs and feet
UPPER_BODY = (3, 6, 9, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21)   # spine, neck, head, arms
FOOT_CONTACT_JOINTS = (7, 10, 8, 11)                             # owner of each of the 4 contact columns, in order


def feature_dim(joints_num: int = 22) -> int:
    return 4 + (joints_num - 1) * 9 + joints_num * 3 + 4


def joint_columns(j: int, joints_num: int = 22) -> list:
    """Feature columns joint ``j`` owns (see the module docstring); every column has exactly one owner."""
    J = joints_num
    if J != 22:
        raise ValueError("the foot-contact columns are defined for the 22-joint skeleton only")
    if not 0 <= j < J:
        raise ValueError(f"joint {j} outside [0, {J})")
    ric, rot, vel, contact = 4, 4 + (J - 1) * 3, 4 + (J - 1) * 9, 4 + (J - 1) * 9 + J * 3
    cols = list(range(4)) if j == 0 else []
    if j > 0:
        cols += list(range(ric + (j - 1) * 3, ric + j * 3)) + list(range(rot + (j - 1) * 6, rot + j * 6))
    cols += list(range(vel + j * 3, vel + (j + 1) * 3))
    cols += [contact + c for c, owner in enumerate(FOOT_CONTACT_JOINTS) if owner == j]
    return cols


def joint_feature_mask(joints: Iterable[int], joints_num: int = 22) -> torch.Tensor:
    """(F,) mask: 1 on the columns of ``joints`` (e.g. ``UPPER_BODY`` to keep the upper body and regenerate the legs)."""
    m = torch.zeros(feature_dim(joints_num), dtype=torch.float32)
    for j in joints:
        m[joint_columns(int(j), joints_num)] = 1.0
    return m


def prefix_mask(T: int, n: int) -> torch.Tensor:
    """(T, 1) frame mask keeping the first ``n`` frames (motion completion / continuation)."""
    if not 0 <= n <= T:
        raise ValueError(f"prefix of {n} frames outside [0, {T}]")
    m = torch.zeros((T, 1), dtype=torch.float32)
    m[:n] = 1.0
    return m


def inbetween_mask(T: int, head: int, tail: int) -> torch.Tensor:
    """(T, 1) frame mask keeping the first ``head`` and the last ``tail`` frames (in-betweening)."""
    if head < 0 or tail < 0 or head + tail > T:
        raise ValueError(f"head {head} + tail {tail} frames do not fit in {T}")
    m = torch.zeros((T, 1), dtype=torch.float32)
    m[:head] = 1.0
    m[T - tail:] = 1.0
    return m

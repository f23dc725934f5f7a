"""Device-side post-processing of generated motions.

Host mirror of what the reference does on the CPU after sampling (tools/visualization.py:21-27,89):
``motion * std + mean`` -> ``recover_from_ric`` (utils/motion_process.py:403-416) -> ``motion_temporal_filter``
(utils/utils.py:125-130).  All arithmetic is in ``mdm_motion_postprocess`` (csrc/motion_post.hip); no eager fallback.

``motion_to_joints_fk`` is the other way to joints: forward kinematics of the rows' rot6d columns on fixed
bone offsets (``recover_from_rot``, utils/motion_process.py:384-398), in ``mdm_motion_fk`` (csrc/motion_fk.hip).  Bones are
rigid by construction, and the per-joint global rotations come with it."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib as L


def gaussian_taps(sigma: float, truncate: float = 4.0) -> np.ndarray:
    """w[0..radius] of scipy.ndimage.gaussian_filter1d's normalised kernel (w[k] == w[-k]), fp64."""
    if sigma is None or sigma <= 0:
        return np.zeros(1, dtype=np.float64)
    radius = int(truncate * float(sigma) + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    return np.ascontiguousarray(phi[radius:], dtype=np.float64)


@torch.no_grad()
def motion_to_joints(motion: torch.Tensor, mean, std, lengths: Optional[torch.Tensor] = None, joints_num: int = 22,
                     sigma: float = 1.0) -> torch.Tensor:
    """motion (B, T, 263) normalised samples on a GPU -> joints (B, T, joints_num, 3); frames >= lengths[b] are zero."""
    L.require_cuda(motion)
    dev = motion.device
    x = motion.detach().to(torch.float32).contiguous()
    if x.dim() == 2:
        x = x[None]
    B, T, Fe = x.shape
    mean_t = torch.as_tensor(np.asarray(mean), dtype=torch.float32).to(dev).contiguous()
    std_t = torch.as_tensor(np.asarray(std), dtype=torch.float32).to(dev).contiguous()
    if mean_t.numel() != Fe or std_t.numel() != Fe:
        raise ValueError(f"mean/std must have {Fe} entries")
    w = gaussian_taps(sigma)
    radius = len(w) - 1
    w_t = torch.from_numpy(w).to(dev)
    ln = None if lengths is None else torch.as_tensor(lengths).to(dev, torch.int32).contiguous()
    scratch = torch.empty(B, T, joints_num, 3, device=dev)
    out = torch.empty_like(scratch)
    with torch.cuda.device(dev):
        L.check(L.lib().mdm_motion_postprocess(
            C.c_void_p(x.data_ptr()), C.c_void_p(L.ptr(ln)), C.c_void_p(mean_t.data_ptr()), C.c_void_p(std_t.data_ptr()),
            C.c_int32(B), C.c_int32(T), C.c_int32(Fe), C.c_int32(joints_num), C.c_int32(radius), C.c_void_p(w_t.data_ptr()),
            C.c_void_p(scratch.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(L.stream_ptr())), "mdm_motion_postprocess")
    return out


def recover_from_ric(data: torch.Tensor, joints_num: int = 22) -> torch.Tensor:
    """Same name / meaning as utils/motion_process.py:403: de-normalised 263-d rows (..., T, 263) -> (..., T, J, 3)."""
    lead = data.shape[:-2]
    x = data.reshape((-1,) + tuple(data.shape[-2:]))
    Fe = x.shape[-1]
    j = motion_to_joints(x, np.zeros(Fe, np.float32), np.ones(Fe, np.float32), None, joints_num, sigma=0.0)
    return j.reshape(lead + tuple(j.shape[1:]))


def fk_max_frames() -> int:
    """The longest motion ``mdm_motion_fk`` takes (20 bytes of LDS per frame); longer ones are MDM_ERR_UNSUPPORTED."""
    return int(L.lib().mdm_motion_fk_max_frames())


def check_fk(motion, mean, std, lengths, offsets, sk):
    """Argument checks of ``motion_to_joints_fk`` that need no device: -> (motion (B, T, F), mean, std float32 (F,) on the CPU,
    lengths (B,) int64 or None, offsets float32 (J, 3) / (B, J, 3) on the CPU or None).  Raises ValueError."""
    J, F_ = sk.joints, sk.feats
    x = torch.as_tensor(motion)
    if x.dim() == 2:
        x = x[None]
    if x.dim() != 3 or x.shape[-1] != F_:
        raise ValueError(f"motion of shape {tuple(x.shape)} must be (B, T, {F_}) for a skeleton of {J} joints")
    B, T = x.shape[:2]
    if T < 1:
        raise ValueError("a motion needs at least 1 frame")
    mean, std = (torch.as_tensor(v if torch.is_tensor(v) else np.asarray(v)).detach().to("cpu", torch.float32).flatten()
                 for v in (mean, std))
    if mean.numel() != F_ or std.numel() != F_:
        raise ValueError(f"mean/std must have {F_} entries")
    if not (bool(torch.isfinite(mean).all()) and bool(torch.isfinite(std).all())):
        raise ValueError("mean / std have non-finite values")
    if bool((std == 0).any()):
        raise ValueError("std has zero entries")
    if lengths is not None:
        lengths = torch.as_tensor(lengths).flatten().to(torch.int64).cpu()
        if lengths.numel() != B:
            raise ValueError(f"lengths must have {B} entries")
        if B and (int(lengths.min()) < 1 or int(lengths.max()) > T):
            raise ValueError(f"every length must lie in [1, {T}]")
    if offsets is not None:
        offsets = torch.as_tensor(offsets).detach().to("cpu", torch.float32)
        if tuple(offsets.shape) not in ((J, 3), (B, J, 3)) or not bool(torch.isfinite(offsets).all()):
            raise ValueError(f"offsets must be finite and of shape ({J}, 3) or ({B}, {J}, 3)")
    if T > fk_max_frames():
        raise ValueError(f"a motion of {T} frames: forward kinematics takes at most {fk_max_frames()} frames")
    return x, mean, std, lengths, offsets


@torch.no_grad()
def motion_to_joints_fk(motion: torch.Tensor, mean, std, lengths: Optional[torch.Tensor] = None, offsets=None, *,
                        skeleton="t2m", sigma: float = 1.0, return_rotations: bool = False, return_offsets: bool = False):
    """motion (B, T, F) normalised rows on a GPU -> joints (B, T, J, 3) by forward kinematics of the rot6d columns; frames
    >= lengths[b] are zero.  ``offsets``: bone offsets (J, 3) for the whole batch or (B, J, 3) per sample, e.g. from
    ``motion_features.skeleton_offsets``; None gives every sample its own, each bone's mean length over the sample's valid
    frames on its ``recover_from_ric`` joints ("make this clip's bones rigid").  ``sigma`` filters the joints over time as
    ``motion_to_joints`` does.  ``return_rotations``: also the global rotation matrices (B, T, J, 3, 3), the root's at joint
    0, never filtered (``sigma=0`` makes joints and rotations agree); ``return_offsets``: also the offsets used (B, J, 3).
    A rot6d pair of zero norm, or a parallel one, gives non-finite joints down that frame's chain, as in the reference."""
    from .motion_features import _skeleton_struct, get_skeleton
    sk = get_skeleton(skeleton)
    x, mean_c, std_c, lengths, offsets = check_fk(motion, mean, std, lengths, offsets, sk)
    L.require_cuda(x)
    dev = x.device
    x = x.detach().to(torch.float32).contiguous()
    B, T, Fe = x.shape
    J = sk.joints
    mean_t, std_t = mean_c.to(dev), std_c.to(dev)
    w = gaussian_taps(sigma)
    radius = len(w) - 1
    w_t = torch.from_numpy(w).to(dev)
    ln = None if lengths is None else lengths.to(dev, torch.int32).contiguous()
    off_t = None if offsets is None else offsets.to(dev).contiguous()
    out = torch.empty(B, T, J, 3, device=dev)
    scratch = torch.empty_like(out) if radius > 0 or off_t is None else None
    rot = torch.empty(B, T, J, 3, 3, device=dev) if return_rotations else None
    used = torch.empty(B, J, 3, device=dev) if return_offsets else None
    s = _skeleton_struct(sk)
    with torch.cuda.device(dev):
        L.check(L.lib().mdm_motion_fk(
            C.c_void_p(x.data_ptr()), C.c_void_p(L.ptr(ln)), C.c_void_p(mean_t.data_ptr()), C.c_void_p(std_t.data_ptr()),
            C.byref(s), C.c_void_p(L.ptr(off_t)), C.c_int32(1 if off_t is not None and off_t.dim() == 3 else 0), C.c_int32(B),
            C.c_int32(T), C.c_int32(Fe), C.c_int32(radius), C.c_void_p(w_t.data_ptr()), C.c_void_p(L.ptr(scratch)),
            C.c_void_p(out.data_ptr()), C.c_void_p(L.ptr(rot)), C.c_void_p(L.ptr(used)), C.c_void_p(L.stream_ptr())),
            "mdm_motion_fk")
    res = (out,) + ((rot,) if return_rotations else ()) + ((used,) if return_offsets else ())
    return res if len(res) > 1 else out


def recover_from_rot(data: torch.Tensor, joints_num: int, offsets, *, skeleton=None) -> torch.Tensor:
    """Same name / meaning as utils/motion_process.py:384 with the skeleton's offsets given: de-normalised rows
    (..., T, F) -> (..., T, J, 3).  ``skeleton`` defaults by ``joints_num`` (22: "t2m", 21: "kit")."""
    if skeleton is None:
        if joints_num not in (22, 21):
            raise ValueError("joints_num must be 22 (t2m) or 21 (kit) when no skeleton is given")
        skeleton = {22: "t2m", 21: "kit"}[joints_num]
    from .motion_features import get_skeleton
    if get_skeleton(skeleton).joints != joints_num:
        raise ValueError(f"the skeleton has {get_skeleton(skeleton).joints} joints, not {joints_num}")
    lead = data.shape[:-2]
    x = data.reshape((-1,) + tuple(data.shape[-2:]))
    Fe = x.shape[-1]
    j = motion_to_joints_fk(x, np.zeros(Fe, np.float32), np.ones(Fe, np.float32), None, offsets, skeleton=skeleton, sigma=0.0)
    return j.reshape(lead + tuple(j.shape[1:]))

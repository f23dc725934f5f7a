"""Device-side post-processing of generated motions.

Host mirror of what the reference does on the CPU after sampling (tools/visualization.py:21-27,89):
``motion * std + mean`` -> ``recover_from_ric`` (utils/motion_process.py:403-416) -> ``motion_temporal_filter``
(utils/utils.py:125-130).  All arithmetic is in ``mdm_motion_postprocess`` (csrc/motion_post.hip); no eager fallback.

``motion_to_joints_fk`` is the other way to joints: forward kinematics of the rows' rot6d columns on fixed
bone offsets (``recover_from_rot``, utils/motion_process.py:384-398), in ``mdm_motion_fk`` (csrc/motion_fk.hip).  Bones are
rigid by construction, and the per-joint global rotations come with it.

``remove_foot_skate`` is the next stage: where a foot-contact label is on, the ankle is pinned to its mean
position over the run by two-bone leg IK and the toe is aimed at its own, in ``mdm_foot_skate`` (csrc/foot_skate.hip).

``pin_limbs`` is the last stage: where a wrist or ankle has a 3-D target, the joint is put on it by two-bone
IK of its limb, in ``mdm_limb_pin`` (csrc/limb_pin.hip)."""
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
    mean_t, std_t = (v.to(dev) for v in L.mean_std(mean, std, Fe, values=False))
    w = gaussian_taps(sigma)
    radius = len(w) - 1
    w_t = torch.from_numpy(w).to(dev)
    ln = None if lengths is None else torch.as_tensor(lengths).to(dev, torch.int32).contiguous()
    scratch = torch.empty(B, T, joints_num, 3, device=dev)
    out = torch.empty_like(scratch)
    with torch.cuda.device(dev):
        L.check(L.lib().mdm_motion_postprocess(
            x.data_ptr(), L.ptr(ln), mean_t.data_ptr(), std_t.data_ptr(), B, T, Fe, joints_num, radius, w_t.data_ptr(),
            scratch.data_ptr(), out.data_ptr(), L.stream_ptr()), "mdm_motion_postprocess")
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
    mean, std = L.mean_std(mean, std, F_)
    if lengths is not None:
        lengths = L.check_lengths(lengths, B, T)
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
            x.data_ptr(), L.ptr(ln), mean_t.data_ptr(), std_t.data_ptr(), C.byref(s), L.ptr(off_t),
            1 if off_t is not None and off_t.dim() == 3 else 0, B, T, Fe, radius, w_t.data_ptr(), L.ptr(scratch), out.data_ptr(),
            L.ptr(rot), L.ptr(used), L.stream_ptr()), "mdm_motion_fk")
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


def foot_skate_max_frames() -> int:
    """The longest motion ``mdm_foot_skate`` takes (5 bytes of LDS per frame); longer ones are MDM_ERR_UNSUPPORTED."""
    return int(L.lib().mdm_foot_skate_max_frames())


def leg_joints(sk):
    """((hip, knee, ankle, toe), (hip, knee, ankle, toe)) of a skeleton: per pair of ``sk.feet`` (ankle, toe) the last four
    entries of the chain that ends in the toe.  Raises ValueError where the skeleton has no such legs."""
    legs = []
    for ankle, toe in (sk.feet[0:2], sk.feet[2:4]):
        found = [c for c in sk.chains if len(c) >= 4 and c[-1] == toe and c[-2] == ankle]
        if not found:
            raise ValueError(f"the skeleton has no chain of 4 or more joints that ends in ankle {ankle}, toe {toe}")
        legs.append(tuple(int(j) for j in found[0][-4:]))
    if any(a == b for a, b in zip(*legs)):
        raise ValueError("the skeleton's two legs share a joint")
    return tuple(legs)


def check_foot_skate(joints, lengths, contacts, rotations, sk, blend=5, contact_thre=0.5, feet_thre=None):
    """Argument checks of ``remove_foot_skate`` that need no device: -> (joints (B, T, J, 3), lengths (B,) int64 or None,
    contact values ((B, T, 4), or the rows (B, T, F) whose last four columns they are) or None, their four thresholds as
    float32 or None, feet_thre, rotations (B, T, J, 3, 3) or None).  Raises ValueError."""
    J, F_ = sk.joints, sk.feats
    leg_joints(sk)
    x = torch.as_tensor(joints)
    if x.dim() == 3:
        x = x[None]
    if x.dim() != 4 or tuple(x.shape[2:]) != (J, 3):
        raise ValueError(f"joints of shape {tuple(x.shape)} must be (B, T, {J}, 3) for this skeleton")
    B, T = x.shape[:2]
    if T < 1:
        raise ValueError("a motion needs at least 1 frame")
    if int(blend) != blend or blend < 0:
        raise ValueError("blend must be a whole number of frames >= 0")
    if lengths is not None:
        lengths = L.check_lengths(lengths, B, T)
    feet_thre = sk.feet_thre if feet_thre is None else float(feet_thre)
    if not feet_thre >= 0:
        raise ValueError("feet_thre must be >= 0")
    thre = None
    if isinstance(contacts, (tuple, list)):
        if len(contacts) != 3:
            raise ValueError("contacts as a tuple is (motion, mean, std): the rows' own contact columns")
        rows, mean, std = contacts
        rows = torch.as_tensor(rows)
        if rows.dim() == 2:
            rows = rows[None]
        if tuple(rows.shape) != (B, T, F_):
            raise ValueError(f"contacts: motion of shape {tuple(rows.shape)} must be ({B}, {T}, {F_})")
        mean, std = L.mean_std(mean, std, F_, torch.float64, values=False)  # only the contact columns are read
        if not (bool(torch.isfinite(mean[-4:]).all()) and bool(torch.isfinite(std[-4:]).all()) and bool((std[-4:] > 0).all())):
            raise ValueError("mean / std of the contact columns must be finite, std > 0")
        thre = ((float(contact_thre) - mean[-4:]) / std[-4:]).to(torch.float32)  # fp64 on the host, rounded once
        contacts = rows
    elif contacts is not None:
        contacts = torch.as_tensor(contacts)
        if contacts.dim() == 2:
            contacts = contacts[None]
        if tuple(contacts.shape) != (B, T, 4):
            raise ValueError(f"contacts of shape {tuple(contacts.shape)} must be ({B}, {T}, 4)")
        thre = torch.full((4,), float(contact_thre), dtype=torch.float32)
    if thre is not None and not bool(torch.isfinite(thre).all()):
        raise ValueError("contact_thre must be finite")
    if rotations is not None:
        rotations = torch.as_tensor(rotations)
        if rotations.dim() == 4:
            rotations = rotations[None]
        if tuple(rotations.shape) != (B, T, J, 3, 3):
            raise ValueError(f"rotations of shape {tuple(rotations.shape)} must be ({B}, {T}, {J}, 3, 3)")
    if T > foot_skate_max_frames():
        raise ValueError(f"a motion of {T} frames: foot-skate clean-up takes at most {foot_skate_max_frames()} frames")
    return x, lengths, contacts, thre, feet_thre, rotations


@torch.no_grad()
def remove_foot_skate(joints, lengths=None, contacts=None, *, skeleton="t2m", feet_thre=None, contact_thre=0.5, blend=5,
                      rotations=None, return_slide=False):
    """joints (B, T, J, 3) on a GPU -> joints whose planted feet stand still; frames >= lengths[b] are zero.
    Where a foot joint's contact label is on, its ankle is moved in XZ to its mean position over that run of frames by
    two-bone IK of the leg with the hip fixed, and the toe is aimed from the new ankle at its own pinned position (aimed, not
    pinned: the toe keeps its bone length).  ``blend`` frames either side of a run the correction fades out.  Heights, the
    hips and the rest of the body are untouched.  ``contacts``: None detects the labels from the joints (squared
    displacement to the next frame under ``feet_thre``, default the skeleton's); a (B, T, 4) tensor of label values, on
    where > ``contact_thre``; or ``(motion, mean, std)``: the last four columns of the normalised rows (B, T, F) that the
    joints came from, read in place, on where the de-normalised value is > ``contact_thre``.  ``rotations`` (B, T, J, 3, 3)
    global rotations (``motion_to_joints_fk(..., return_rotations=True)``) are turned with the bones and returned after the
    joints.  ``return_slide``: also ``(slide (B, 2, 4), pairs (B, 4))``, per foot joint the mean XZ step between neighbouring
    contact frames before [:, 0] and after [:, 1], and the number of such pairs.  A target out of the leg's reach is
    approached as far as the leg goes."""
    from .motion_features import _skeleton_struct, get_skeleton
    sk = get_skeleton(skeleton)
    x, lengths, cont, thre, feet_thre, rot = check_foot_skate(joints, lengths, contacts, rotations, sk, blend, contact_thre,
                                                             feet_thre)
    L.require_cuda(x, cont, rot)
    dev = x.device
    x = x.detach().to(torch.float32).contiguous()
    B, T, J = x.shape[:3]
    ln = None if lengths is None else lengths.to(dev, torch.int32).contiguous()
    cptr, stride, thre_c = 0, 0, None
    if cont is not None:
        if cont.device != dev:
            raise ValueError("contacts must be on the joints' device")
        cont = cont.detach().to(torch.float32).contiguous()
        stride = cont.shape[-1]
        cptr = cont.data_ptr() + 4 * (stride - 4)  # a (B, T, 4) tensor, or the rows' last four columns in place
        thre_c = (C.c_float * 4)(*[float(v) for v in thre])
    if rot is not None:
        if rot.device != dev:
            raise ValueError("rotations must be on the joints' device")
        rot = rot.detach().to(torch.float32).contiguous()
    out = torch.empty_like(x)
    rot_out = None if rot is None else torch.empty_like(rot)
    scratch = torch.empty(B, T, 4, 2, device=dev)
    slide = torch.empty(B, 2, 4, device=dev) if return_slide else None
    pairs = torch.empty(B, 4, dtype=torch.int32, device=dev) if return_slide else None
    s = _skeleton_struct(sk)
    with torch.cuda.device(dev):
        L.check(L.lib().mdm_foot_skate(
            x.data_ptr(), L.ptr(ln), C.byref(s), cptr, stride, thre_c, feet_thre, int(blend), B, T, L.ptr(rot), out.data_ptr(),
            L.ptr(rot_out), L.ptr(slide), L.ptr(pairs), scratch.data_ptr(), L.stream_ptr()), "mdm_foot_skate")
    res = (out,) + ((rot_out,) if rot is not None else ()) + (((slide, pairs),) if return_slide else ())
    return res if len(res) > 1 else out


LIMB_NAMES = ("right_leg", "left_leg", "right_arm", "left_arm")
MAX_LIMBS = 8


def limb_pin_max_frames() -> int:
    """The longest motion ``mdm_limb_pin`` takes (9 bytes of LDS per frame); longer ones are MDM_ERR_UNSUPPORTED."""
    return int(L.lib().mdm_limb_pin_max_frames())


def limbs(skeleton="t2m"):
    """The two-bone limbs of a skeleton by name, each ``(root, mid, end, tip)`` with ``tip = -1`` where the end joint has no
    child: ``right_leg`` / ``left_leg`` (hip, knee, ankle, toe: ``leg_joints``, the legs of ``remove_foot_skate``) and
    ``right_arm`` / ``left_arm`` (shoulder, elbow, wrist, -1: the last three entries of the chains that do not start at
    joint 0).  The right side is the one whose chain holds ``face[0]`` (legs) / ``face[2]`` (arms)."""
    from .motion_features import get_skeleton
    sk = get_skeleton(skeleton)
    legs = sorted(leg_joints(sk), key=lambda leg: sk.face[0] not in [c for c in sk.chains if c[-1] == leg[-1]][0])
    arms = sorted([c for c in sk.chains if c[0] != 0 and len(c) >= 3], key=lambda c: sk.face[2] not in c)
    if len(arms) != 2:
        raise ValueError("the skeleton has no two arm chains (chains of 3 or more joints that do not start at joint 0)")
    rows = [tuple(int(j) for j in leg) for leg in legs] + [tuple(int(j) for j in c[-3:]) + (-1,) for c in arms]
    return dict(zip(LIMB_NAMES, rows))


def _limb_table(limbs_arg, skeleton, J):
    """``limbs=`` of ``pin_limbs`` -> int32 (L, 4): None (all four defaults), names of ``limbs(skeleton)``, or rows."""
    if limbs_arg is None:
        limbs_arg = LIMB_NAMES
    if isinstance(limbs_arg, str):
        limbs_arg = (limbs_arg,)
    rows = []
    named = None
    for q in limbs_arg:
        if isinstance(q, str):
            named = limbs(skeleton) if named is None else named
            if q not in named:
                raise ValueError(f"limbs: {q!r} is not one of {sorted(named)}")
            q = named[q]
        q = [int(v) for v in np.asarray(q).reshape(-1)] if np.asarray(q).size in (3, 4) else None
        if q is None:
            raise ValueError("limbs: a limb is a name or (root, mid, end[, tip])")
        rows.append(q + [-1] * (4 - len(q)))
    if not 1 <= len(rows) <= MAX_LIMBS:
        raise ValueError(f"limbs: between 1 and {MAX_LIMBS} limbs, not {len(rows)}")
    moved = []
    for q in rows:
        if any(not (-1 if k == 3 else 0) <= v < J for k, v in enumerate(q)):
            raise ValueError(f"limbs: {tuple(q)} has a joint outside 0 .. {J - 1} (only the tip may be -1)")
        if len(set(q)) != 4:
            raise ValueError(f"limbs: {tuple(q)} names a joint twice")
        moved += [v for v in q[1:] if v >= 0]
    if len(set(moved)) != len(moved) or any(q[0] in moved for q in rows):
        raise ValueError("limbs: a joint that one limb moves belongs to no other limb")
    return np.ascontiguousarray(rows, dtype=np.int32)


def check_pin_limbs(joints, lengths, targets, weights, rotations, sk, limbs=None, blend=5, skeleton="t2m"):
    """Argument checks of ``pin_limbs`` that need no device: -> (joints (B, T, J, 3), lengths (B,) int64 or None, targets
    (B, T, J, 3), weights expanded to (B, T, J, 3), rotations (B, T, J, 3, 3) or None, limb table int32 (L, 4)).  Weights
    broadcast as ``control_weights`` do: aligned on the leading dims, (B,) per sample, (B, T) per frame, (B, T, J) per joint.
    Raises ValueError: shapes, weights that are negative or not finite in a frame that counts, limb tables, ``blend``, CPU
    tensors."""
    from .conditioning import expand_to
    J = sk.joints
    x = torch.as_tensor(joints)
    g, w = torch.as_tensor(targets), torch.as_tensor(weights)
    if x.dim() == 3:  # one clip: targets (T, J, 3), weights aligned on the frame dim
        x, g, w = x[None], g[None], w[None]
    if x.dim() != 4 or tuple(x.shape[2:]) != (J, 3):
        raise ValueError(f"joints of shape {tuple(x.shape)} must be (B, T, {J}, 3) for this skeleton")
    B, T = x.shape[:2]
    if T < 1:
        raise ValueError("a motion needs at least 1 frame")
    if int(blend) != blend or blend < 0:
        raise ValueError("blend must be a whole number of frames >= 0")
    if lengths is not None:
        lengths = L.check_lengths(lengths, B, T)
    if tuple(g.shape) != (B, T, J, 3):
        raise ValueError(f"targets of shape {tuple(g.shape)} must be {(B, T, J, 3)}")
    if not (g.dtype.is_floating_point and w.dtype.is_floating_point):
        raise ValueError("targets and weights must be floating point")
    w = expand_to(w, 1, (B, T, J, 3), "weights", f"must lead with the batch size {B}")
    wv = w if lengths is None else w[torch.arange(T)[None] < lengths[:, None]]  # frames past a length are never read
    if not bool(torch.isfinite(wv).all()):
        raise ValueError("weights has non-finite values")
    if bool((wv < 0).any()):
        raise ValueError("weights must be >= 0")
    table = _limb_table(limbs, skeleton, J)
    if rotations is not None:
        rotations = torch.as_tensor(rotations)
        if rotations.dim() == 4:
            rotations = rotations[None]
        if tuple(rotations.shape) != (B, T, J, 3, 3):
            raise ValueError(f"rotations of shape {tuple(rotations.shape)} must be ({B}, {T}, {J}, 3, 3)")
    for name, v in (("joints", x), ("rotations", rotations)):
        if v is not None and v.device.type == "cpu":
            raise ValueError(f"{name} must be on a GPU: limb pins have no CPU path")
    if T > limb_pin_max_frames():
        raise ValueError(f"a motion of {T} frames: limb pins take at most {limb_pin_max_frames()} frames")
    return x, lengths, g, w, rotations, table


@torch.no_grad()
def pin_limbs(joints, lengths, targets, weights, *, skeleton="t2m", limbs=None, blend=5, rotations=None, return_error=False):
    """joints (B, T, J, 3) on a GPU -> joints whose wrists and ankles lie on their targets; frames >=
    lengths[b] are zero.  ``targets`` (B, T, J, 3) and ``weights`` broadcastable to it are ``control_joints`` /
    ``control_weights`` as joint control takes them (on any device): frame t is a pin frame of a limb where all three
    weights of its end joint are > 0; targets on other joints or with fewer weighted coordinates are ignored, targets under
    weight 0 are never read, and a weight's size does not matter.  In a pin frame the end joint is moved onto its target by
    two-bone IK with the limb root (hip, shoulder) fixed, the mid joint staying in its bend plane and the tip (toe) carried
    rigidly; ``blend`` frames either side of a pin frame the correction fades out.  A target out of the limb's reach is
    approached as far as the limb goes.  ``limbs``: names out of ``limbs(skeleton)`` (default all four) or rows
    ``(root, mid, end, tip)``.  ``rotations`` (B, T, J, 3, 3) global rotations (``motion_to_joints_fk(...,
    return_rotations=True)``) are turned with the bones and returned after the joints.  ``return_error``: also
    ``(error (B, L, 2, 2), counts (B, L, 2))``: per limb over its pin frames the mean and maximum distance of the end joint
    to its target before [:, :, 0] and after [:, :, 1], and the number of pin frames and of those out of reach."""
    from .motion_features import get_skeleton
    sk = get_skeleton(skeleton)
    x, lengths, g, w, rot, table = check_pin_limbs(joints, lengths, targets, weights, rotations, sk, limbs, blend, skeleton)
    L.require_cuda(x, rot)
    dev = x.device
    x = x.detach().to(torch.float32).contiguous()
    B, T, J = x.shape[:3]
    ln = None if lengths is None else lengths.to(dev, torch.int32).contiguous()
    g = g.detach().to(dev, torch.float32).contiguous()
    w = w.detach().to(dev, torch.float32).contiguous()
    if rot is not None:
        if rot.device != dev:
            raise ValueError("rotations must be on the joints' device")
        rot = rot.detach().to(torch.float32).contiguous()
    nl = int(table.shape[0])
    out = torch.empty_like(x)
    rot_out = None if rot is None else torch.empty_like(rot)
    scratch = torch.empty(B, T, nl, 3, device=dev)
    err = torch.empty(B, nl, 2, 2, device=dev) if return_error else None
    counts = torch.empty(B, nl, 2, dtype=torch.int32, device=dev) if return_error else None
    with torch.cuda.device(dev):
        L.check(L.lib().mdm_limb_pin(
            x.data_ptr(), L.ptr(ln), g.data_ptr(), w.data_ptr(), table.ctypes.data, nl, J, int(blend), B, T, L.ptr(rot),
            out.data_ptr(), L.ptr(rot_out), L.ptr(err), L.ptr(counts), scratch.data_ptr(), L.stream_ptr()), "mdm_limb_pin")
    res = (out,) + ((rot_out,) if rot is not None else ()) + (((err, counts),) if return_error else ())
    return res if len(res) > 1 else out

"""Scene constraints (``DDPMTrainer.generate(..., scene=)``): keep joints out of obstacles and above the floor.

A scene is a list of at most ``MAX_PRIMS`` primitives fixed in the frame of ``recover_from_ric`` applied to de-normalised
features (``motion_control``'s units: metres in HumanML3D, Y up, the motion starting at the origin of the XZ plane with
heading 0; for a long motion, the canvas frame).  Primitive k has a signed distance d_k(p) (negative inside), a margin m_k, a
weight a_k >= 0 and a sign: +1 keeps joints out, -1 (``inside=True``) keeps them in, e.g. a walkable region.  Joint j has a
radius r_j >= 0 and a weight u_j >= 0 (0 exempts it).  The guidance of joint control (§14) minimises, next to its target term,

    L_scene,b = sum_{t < len_b} sum_j u_j sum_k a_k max(0, m_k + r_j - sigma_k d_k(P[t, j]))^2

``sphere``, ``capsule``, ``box``, ``half_space`` and ``floor`` make primitives, ``pack_scene`` turns a list of them into the
(K, 12) float32 records the kernels read (kind, sigma, weight, margin, eight parameters; a box's yaw is stored as its cosine
and sine).  ``scene_loss_grad`` / ``canvas_scene_loss_grad`` run the loss and its gradient on the device
(``mdm_joint_scene_loss_grad`` / ``mdm_canvas_scene_loss_grad``); ``penetration`` checks a result in plain torch."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib as L
from .motion_control import LDS_BYTES, _rows, joints_for_feats, steerable_columns

MAX_PRIMS, REC = L.SCENE_MAX_PRIMS, L.SCENE_REC
PAD, SPHERE, CAPSULE, BOX, HALF_SPACE = 0, 1, 2, 3, 4


class Primitive(tuple):
    """One primitive's record: REC floats (kind, sigma, weight, margin, eight parameters)."""


def _vec(v, n, name):
    a = np.asarray(v, dtype=np.float64).reshape(-1)
    if a.size != n:
        raise ValueError(f"{name} must have {n} entries, not {a.size}")
    if not np.isfinite(a).all():
        raise ValueError(f"{name} has non-finite values")
    return a.tolist()


def _positive(v, name):
    v = float(v)
    if not (math.isfinite(v) and v > 0):
        raise ValueError(f"{name} must be finite and > 0, not {v}")
    return v


def _record(kind, params, margin, weight, inside):
    margin, weight = float(margin), float(weight)
    if not math.isfinite(margin):
        raise ValueError("margin must be finite")
    if not (math.isfinite(weight) and weight >= 0):
        raise ValueError(f"weight must be finite and >= 0, not {weight}")
    return Primitive([float(kind), -1.0 if inside else 1.0, weight, margin] + list(params) + [0.0] * (8 - len(params)))


def sphere(center, radius, *, margin=0.0, weight=1.0, inside=False):
    """A sphere: d(p) = |p - center| - radius."""
    return _record(SPHERE, _vec(center, 3, "center") + [_positive(radius, "radius")], margin, weight, inside)


def capsule(a, b, radius, *, margin=0.0, weight=1.0, inside=False):
    """A capsule (a pillar, a bar): d(p) = distance to the segment a b - radius; a == b is a sphere."""
    return _record(CAPSULE, _vec(a, 3, "a") + _vec(b, 3, "b") + [_positive(radius, "radius")], margin, weight, inside)


def box(center, half_extents, yaw=0.0, *, margin=0.0, weight=1.0, inside=False):
    """A box (a table, a wall with a thickness) turned by ``yaw`` radians about Y: the exact box distance in its own frame."""
    yaw = float(yaw)
    if not math.isfinite(yaw):
        raise ValueError("yaw must be finite")
    h = _vec(half_extents, 3, "half_extents")
    for v in h:
        _positive(v, "every half extent")
    return _record(BOX, _vec(center, 3, "center") + h + [math.cos(yaw), math.sin(yaw)], margin, weight, inside)


def half_space(normal, offset, *, margin=0.0, weight=1.0, inside=False):
    """A half-space (the floor, an infinite wall): d(p) = n . p - offset, n = ``normal`` normalised here; joints are kept on
    the side the normal points to."""
    n = np.asarray(_vec(normal, 3, "normal"))
    length = float(np.linalg.norm(n))
    if not length > 0:
        raise ValueError("normal must not be zero")
    offset = float(offset)
    if not math.isfinite(offset):
        raise ValueError("offset must be finite")
    return _record(HALF_SPACE, (n / length).tolist() + [offset], margin, weight, inside)


def floor(height=0.0, *, margin=0.0, weight=1.0):
    """The floor at Y = ``height``: joints stay above it."""
    return half_space((0.0, 1.0, 0.0), height, margin=margin, weight=weight)


def check_records(rec, name="scene"):
    """``rec`` (..., K, REC), packed records, as a float32 tensor; ValueError for more than MAX_PRIMS primitives, non-finite
    values, an unknown kind, a sign other than +-1, a weight < 0, a radius or half extent <= 0 and a zero normal."""
    rec = torch.as_tensor(rec)
    if rec.dim() < 2 or rec.shape[-1] != REC or not rec.is_floating_point():
        raise ValueError(f"{name} of shape {tuple(rec.shape)} must be floating point (..., K, {REC})")
    if rec.shape[-2] > MAX_PRIMS:
        raise ValueError(f"{name} has {rec.shape[-2]} primitives: a scene takes at most {MAX_PRIMS}")
    r = rec.detach().to("cpu", torch.float32).reshape(-1, REC)
    if not bool(torch.isfinite(r).all()):
        raise ValueError(f"{name} has non-finite values")
    kind = r[:, 0]
    if bool(((kind != kind.round()) | (kind < PAD) | (kind > HALF_SPACE)).any()):
        raise ValueError(f"{name} has an unknown primitive kind")
    live = r[kind != PAD]
    if bool((live[:, 1].abs() != 1).any()):
        raise ValueError(f"{name}: a primitive's sign must be +1 (keep out) or -1 (keep in)")
    if bool((live[:, 2] < 0).any()):
        raise ValueError(f"{name}: a primitive's weight must be >= 0")
    k = live[:, 0]
    if bool((live[k == SPHERE][:, 7] <= 0).any()) or bool((live[k == CAPSULE][:, 10] <= 0).any()):
        raise ValueError(f"{name}: a radius must be > 0")
    if bool((live[k == BOX][:, 7:10] <= 0).any()):
        raise ValueError(f"{name}: a box's half extents must be > 0")
    if bool((live[k == HALF_SPACE][:, 4:7].norm(dim=1) == 0).any()):
        raise ValueError(f"{name}: a half-space's normal must not be zero")
    return rec.detach().to(torch.float32)


def pack_scene(prims) -> torch.Tensor:
    """A list of primitives as the (K, REC) float32 records of the kernels (CPU).  ValueError for more than MAX_PRIMS."""
    prims = list(prims)
    if len(prims) > MAX_PRIMS:
        raise ValueError(f"{len(prims)} primitives: a scene takes at most {MAX_PRIMS}")
    for p in prims:
        if not isinstance(p, Primitive):
            raise ValueError("a scene is a list of primitives made by sphere / capsule / box / half_space / floor")
    out = torch.tensor([list(p) for p in prims], dtype=torch.float64).reshape(len(prims), REC).to(torch.float32)
    return check_records(out)


def batch_scene(scene, N: int) -> torch.Tensor:
    """``scene``, one list of primitives shared by N samples or one list per sample (or packed records (K, REC) /
    (N, K, REC)), as (N, K, REC) float32 records, K the longest list, shorter ones padded with kind 0."""
    if torch.is_tensor(scene) or isinstance(scene, np.ndarray):
        rec = check_records(scene)
        if rec.dim() == 2:
            rec = rec[None].expand(N, -1, -1)
        if rec.dim() != 3 or rec.shape[0] != N:
            raise ValueError(f"scene of shape {tuple(rec.shape)} must be (K, {REC}) or ({N}, K, {REC})")
        return rec.contiguous()
    scene = list(scene)
    if all(isinstance(p, Primitive) for p in scene):
        return pack_scene(scene)[None].expand(N, -1, -1).contiguous()
    if len(scene) != N:
        raise ValueError(f"scene must be one list of primitives, or one list per sample ({N}), not {len(scene)} entries")
    packed = [pack_scene(s) for s in scene]
    out = torch.zeros((N, max(p.shape[0] for p in packed), REC))
    for i, p in enumerate(packed):
        out[i, :p.shape[0]] = p
    return out


def joint_params(J: int, joint_radius=None, joint_weights=None) -> torch.Tensor:
    """The joints' (radius, weight) as (J, 2) float32: radius 0 and weight 1 by default.  ValueError for values that are
    negative, non-finite or not J of them."""
    out = torch.zeros((J, 2))
    out[:, 1] = 1.0
    for col, (name, v) in enumerate((("joint radius", joint_radius), ("joint weights", joint_weights))):
        if v is None:
            continue
        v = torch.as_tensor(v if torch.is_tensor(v) else np.asarray(v, dtype=np.float64)).detach().to("cpu", torch.float32)
        if v.dim() == 0:
            v = v.expand(J)
        if tuple(v.shape) != (J,):
            raise ValueError(f"{name} must have {J} entries, not shape {tuple(v.shape)}")
        if not bool(torch.isfinite(v).all()) or bool((v < 0).any()):
            raise ValueError(f"{name} must be finite and >= 0")
        out[:, col] = v
    return out


def max_frames(F: int, prims: int = MAX_PRIMS) -> int:
    """Longest T the window kernel takes at feature width F with a scene of ``prims`` primitives: §14's LDS layout plus
    the records and the joints' (radius, weight) (202 frames at F = 263, 208 at 251 with 16 primitives).  Equals
    ``mdm_joint_scene_max_frames``."""
    if not 0 <= prims <= MAX_PRIMS:
        raise ValueError(f"a scene takes 0 to {MAX_PRIMS} primitives, not {prims}")
    ds = steerable_columns(F) | 1
    fixed = 2 * ds * 4 + (prims * REC + 2 * joints_for_feats(F)) * 4
    return (LDS_BYTES - fixed) // (ds * 4 + 48)


def signed_distances(p: torch.Tensor, records: torch.Tensor) -> torch.Tensor:
    """d_k(p) of points ``p`` (..., 3) to the K primitives of ``records`` (K, REC): (..., K), in p's dtype on p's device;
    0 for padding.  Plain torch ops."""
    rec = records.detach().to(p.device, p.dtype)
    out = []
    for k, kind in enumerate(records[:, 0].tolist()):
        q = rec[k]
        if kind == SPHERE:
            d = (p - q[4:7]).norm(dim=-1) - q[7]
        elif kind == CAPSULE:
            e, v = q[7:10] - q[4:7], p - q[4:7]
            den = (e * e).sum()
            h = ((v * e).sum(-1) / den).clamp(0, 1) if float(den) > 0 else torch.zeros_like(v[..., 0])
            d = (v - h[..., None] * e).norm(dim=-1) - q[10]
        elif kind == BOX:
            c, s = q[10], q[11]
            dx, dz = p[..., 0] - q[4], p[..., 2] - q[6]
            loc = torch.stack([c * dx - s * dz, p[..., 1] - q[5], s * dx + c * dz], -1)
            qq = loc.abs() - q[7:10]
            d = qq.clamp(min=0).norm(dim=-1) + qq.max(dim=-1).values.clamp(max=0)
        elif kind == HALF_SPACE:
            d = (p * q[4:7]).sum(-1) - q[7]
        else:
            d = torch.zeros_like(p[..., 0])
        out.append(d)
    return torch.stack(out, -1) if out else p.new_zeros(p.shape[:-1] + (0,))


@torch.no_grad()
def penetration(joints, lengths, scene, joint_radius=None):
    """How far a result violates a scene, per sample: ``(depth (B,), share (B,))``.  ``joints`` (B, T, J, 3) joint positions
    (``recover_from_ric`` units) with ``lengths`` (B,), ``scene`` as in ``DDPMTrainer.generate`` (one list, or one per
    sample), ``joint_radius`` (J,) or None.  ``depth``: the deepest penetration of any joint's sphere into any primitive
    (out of a keep-in one), max(0, r_j - sigma_k d_k), margins not counted; ``share``: the share of the sample's frames in
    which any joint is inside a margin (m_k + r_j - sigma_k d_k > 0).  Primitives of weight 0 are ignored.  Plain torch ops
    on the device the joints are on."""
    P = torch.as_tensor(joints)
    if P.dim() != 4 or P.shape[-1] != 3:
        raise ValueError(f"joints of shape {tuple(P.shape)} must be (B, T, J, 3)")
    B, T, J, _ = P.shape
    rec = batch_scene(scene, B)
    r = joint_params(J, joint_radius)[:, 0].to(P.device, P.dtype)
    ln = torch.as_tensor(lengths).flatten().to(P.device)
    if ln.numel() != B:
        raise ValueError(f"lengths must hold {B} entries")
    depth, share = P.new_zeros(B), P.new_zeros(B)
    for b in range(B):
        n = min(max(int(ln[b]), 0), T)
        live = rec[b][(rec[b][:, 0] != PAD) & (rec[b][:, 2] > 0)]
        if n == 0 or live.shape[0] == 0:
            continue
        q = live.to(P.device, P.dtype)
        sd = q[:, 1] * signed_distances(P[b, :n], live)  # (n, J, K)
        depth[b] = (r[None, :, None] - sd).clamp(min=0).max()
        share[b] = ((q[:, 3] + r[None, :, None] - sd) > 0).any(-1).any(-1).to(P.dtype).mean()
    return depth, share


def _scene_args(scene, N, J, joint_radius, joint_weights, dev):
    rec = batch_scene(scene, N).to(dev).contiguous()
    jp = joint_params(J, joint_radius, joint_weights)[None].expand(N, -1, -1).to(dev).contiguous()
    return rec, jp


@torch.no_grad()
def scene_loss_grad(x0: torch.Tensor, lengths, mean, std, scene, joint_radius=None, joint_weights=None, targets=None,
                    weights=None):
    """Loss (B,) and gradient (B, T, F) of L_scene (module docstring), plus §14's target term when ``targets`` (B, T, J, 3)
    and ``weights`` are given, with respect to the normalised features ``x0`` (B, T, F) on a GPU, through
    ``mdm_joint_scene_loss_grad``.  ``scene``: one list of primitives, or one per sample; ``mean`` / ``std``: (F,) or (B, F).
    The gradient is exactly 0 in every column past 3 J and in every frame at or past ``lengths[b]``."""
    L.require_cuda(x0)
    dev = x0.device
    x = x0.detach().to(torch.float32).contiguous()
    if x.dim() != 3:
        raise ValueError(f"x0 of shape {tuple(x.shape)} must be (B, T, F)")
    B, T, F = x.shape
    J = joints_for_feats(F)
    rec, jp = _scene_args(scene, B, J, joint_radius, joint_weights, dev)
    K = rec.shape[1]
    if not 1 <= T <= max_frames(F, K):
        raise ValueError(f"T = {T}: with {K} primitives the control kernels take 1 to {max_frames(F, K)} frames at F = {F}")
    if (targets is None) != (weights is None):
        raise ValueError("targets and weights go together: give both or neither")
    tg = w = None
    if targets is not None:
        tg = torch.as_tensor(targets).to(dev, torch.float32).contiguous()
        if tuple(tg.shape) != (B, T, J, 3):
            raise ValueError(f"targets of shape {tuple(tg.shape)} must be {(B, T, J, 3)}")
        w = torch.broadcast_to(torch.as_tensor(weights).to(dev, torch.float32), (B, T, J, 3)).contiguous()
    mean_t = _rows(mean, B, F, "mean").to(dev).contiguous()
    std_t = _rows(std, B, F, "std").to(dev).contiguous()
    ln = torch.as_tensor(lengths).to(dev, torch.int32).contiguous()
    if tuple(ln.shape) != (B,):
        raise ValueError(f"lengths must hold {B} entries")
    loss = torch.empty(B, device=dev)
    grad = torch.empty_like(x)
    with torch.cuda.device(dev):
        L.check(L.lib().mdm_joint_scene_loss_grad(
            x.data_ptr(), ln.data_ptr(), mean_t.data_ptr(), std_t.data_ptr(), L.ptr(tg), L.ptr(w), rec.data_ptr() if K else 0, K,
            jp.data_ptr(), B, T, F, loss.data_ptr(), grad.data_ptr(), L.stream_ptr()), "mdm_joint_scene_loss_grad")
    return loss, grad


@torch.no_grad()
def canvas_scene_loss_grad(rows: torch.Tensor, motion_offsets, frame_rows, mean, std, scene, joint_radius=None,
                           joint_weights=None, targets=None, weights=None):
    """``scene_loss_grad`` over the canvases of M long motions, as ``motion_control.canvas_loss_grad``: loss (M,) and gradient
    (total, F) dense in canvas order, through ``mdm_canvas_scene_loss_grad``.  ``scene``: one list of primitives, or one per
    motion, in the canvas frame; ``targets`` (total, J, 3) in canvas order and ``weights``, or neither.  Any canvas length."""
    L.require_cuda(rows)
    dev = rows.device
    x = rows.detach().to(torch.float32).contiguous()
    F = x.shape[-1]
    x = x.reshape(-1, F)
    J = joints_for_feats(F)
    off = torch.as_tensor(motion_offsets).flatten().to(torch.int64).cpu()
    fr = torch.as_tensor(frame_rows).flatten().to(torch.int64).cpu()
    M, total = off.numel() - 1, fr.numel()
    if M < 0 or int(off[0]) != 0 or int(off[-1]) != total or bool((off[1:] < off[:-1]).any()):
        raise ValueError(f"motion_offsets must rise from 0 to the number of frame rows {total}")
    if total and (int(fr.min()) < 0 or int(fr.max()) >= x.shape[0] or torch.unique(fr).numel() != total):
        raise ValueError(f"frame_rows must be distinct rows in [0, {x.shape[0]})")
    rec, jp = _scene_args(scene, M, J, joint_radius, joint_weights, dev)
    K = rec.shape[1]
    if (targets is None) != (weights is None):
        raise ValueError("targets and weights go together: give both or neither")
    tg = w = None
    if targets is not None:
        tg = torch.as_tensor(targets).to(dev, torch.float32).contiguous()
        if tuple(tg.shape) != (total, J, 3):
            raise ValueError(f"targets of shape {tuple(tg.shape)} must be {(total, J, 3)}")
        w = torch.broadcast_to(torch.as_tensor(weights).to(dev, torch.float32), (total, J, 3)).contiguous()
    mean_t = _rows(mean, M, F, "mean").to(dev).contiguous()
    std_t = _rows(std, M, F, "std").to(dev).contiguous()
    off_d, fr_d = off.to(dev, torch.int32), fr.to(dev, torch.int32)
    loss = torch.zeros(M, device=dev)
    grad = torch.zeros((total, F), device=dev)
    ws = torch.empty(max(int(L.lib().mdm_canvas_control_workspace_floats(total, F)), 1), device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().mdm_canvas_scene_loss_grad(
            x.data_ptr(), off_d.data_ptr(), fr_d.data_ptr(), mean_t.data_ptr(), std_t.data_ptr(), L.ptr(tg), L.ptr(w),
            rec.data_ptr() if K else 0, K, jp.data_ptr(), M, F, loss.data_ptr(), grad.data_ptr(), ws.data_ptr(), L.stream_ptr()),
            "mdm_canvas_scene_loss_grad")
    return loss, grad

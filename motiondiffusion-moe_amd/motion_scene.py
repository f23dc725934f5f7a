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
(``mdm_joint_scene_loss_grad`` / ``mdm_canvas_scene_loss_grad``); ``penetration`` checks a result in plain torch.

Tracks are primitives that move: a track is a (T, 12) stack of records, one per frame (kind 0: absent in that
frame), made by ``moving_sphere`` / ``moving_capsule`` / ``moving_box`` / ``moving_half_space`` or, for a generated character as
an obstacle, ``character_tracks`` (one capsule per bone; ``to_world`` / ``to_local`` / ``records_to_local`` move joints and
records between a character's own frame and the world).  At most ``MAX_TRACKS`` per sample; ``pack_tracks`` / ``batch_tracks``
give the (T, Km, 12) / (N, T, Km, 12) records of the kernels and ``track_bounds`` the per-frame balls of their broad phase.
They add

    L_tracks,b = sum_{t < len_b} sum_j u_j sum_k a_tk max(0, m_tk + r_j - sigma_tk d(R[t, k]; P[t, j]))^2

to the loss; the records are data (no gradient reaches the obstacle's own motion).  ``scene_loss_grad`` /
``canvas_scene_loss_grad`` / ``penetration`` take ``tracks=``.

A terrain is a height-map ground: a grid of heights (Gz, Gx) in metres with cells of ``cell_x`` by ``cell_z``
metres, its corner sample at ``origin`` = (x, z), turned by ``yaw`` about Y, interpolated bilinearly and continued flat past
its edges.  ``heightfield`` makes one from an array of heights, ``ramp`` and ``stairs`` rasterise into one, ``batch_terrain``
gives the (N, Gz, Gx) grids and (N, 8) records of the kernels, ``terrain_height`` evaluates h in plain torch and
``terrain_to_local`` moves a terrain from the world into a character's frame.  With e = p_y - h(p) the *vertical* clearance (not
the true distance to the surface) and stand weights S[t, j] >= 0 it adds

    L_terrain,b = sum_{t < len_b} sum_j u_j a (max(0, m + r_j - e)^2 + S[t, j] max(0, e - r_j - m)^2)

to the loss: every joint stays above the ground, and a joint said to be planted (S > 0) is pulled down onto it.  The grid and S
are data.  ``scene_loss_grad`` / ``canvas_scene_loss_grad`` take ``terrain=`` and ``stand=``, ``penetration`` takes ``terrain=``.

Characters sampled together: the characters of a scene are rows of one batch, and on every step the tracks a
row avoids are the capsules of its partners' current estimate and the targets it reaches for the meeting points of its
contacts.  ``contact`` makes a contact, ``partner_tables`` the host tables (partner rows, bones, placements, the contact table
and the constant target weights) and ``partner_tracks`` runs the device call (``mdm_partner_tracks``) on its own:
``(tracks, track_bounds, targets)`` as the tracks guidance takes them.

Self-collision avoidance: every joint keeps out of the capsules of the character's own bones.  With the bones
held fixed,

    L_self,b = a sum_{t < len_b} sum_j u_j sum_{i allowed for j} max(0, m + r_j + rho_i - d_i(t, j))^2

with d_i(t, j) the distance of P[t, j] to the segment of bone i in the same frame.  Its gradient is that of the target term at
the targets P + sum_i pen_i n_i under the weights a u_j, so a producer launch writes those in front of the unchanged guidance on
every step.  ``self_body`` makes the body (``default_offsets`` a plain skeleton for it), ``self_push`` runs the push and the
depth on the device (``mdm_self_push``), ``self_targets`` the whole producer (``mdm_self_targets``) and ``self_penetration``
checks a result in plain torch."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib as L
from .motion_control import LDS_BYTES, _rows, joints_for_feats, steerable_columns

MAX_PRIMS, REC, MAX_TRACKS = L.SCENE_MAX_PRIMS, L.SCENE_REC, L.SCENE_MAX_TRACKS
MAX_GRID, TERRAIN_REC = L.TERRAIN_MAX_GRID, L.TERRAIN_REC
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


def check_records(rec, name="scene", limit=MAX_PRIMS):
    """``rec`` (..., K, REC), packed records, as a float32 tensor; ValueError for more than ``limit`` primitives (MAX_PRIMS of a
    scene, MAX_TRACKS of a frame's tracks), non-finite values, an unknown kind, a sign other than +-1, a weight < 0, a radius or
    half extent <= 0 and a zero normal."""
    rec = torch.as_tensor(rec)
    if rec.dim() < 2 or rec.shape[-1] != REC or not rec.is_floating_point():
        raise ValueError(f"{name} of shape {tuple(rec.shape)} must be floating point (..., K, {REC})")
    if rec.shape[-2] > limit:
        raise ValueError(f"{name} has {rec.shape[-2]} primitives: " + (f"a scene takes at most {MAX_PRIMS}" if limit == MAX_PRIMS
                                                                      else f"at most {limit} are allowed"))
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
def penetration(joints, lengths, scene, joint_radius=None, tracks=None, terrain=None):
    """How far a result violates a scene, per sample: ``(depth (B,), share (B,))``.  ``joints`` (B, T, J, 3) joint positions
    (``recover_from_ric`` units) with ``lengths`` (B,), ``scene`` as in ``DDPMTrainer.generate`` (one list, or one per
    sample), ``joint_radius`` (J,) or None.  ``depth``: the deepest penetration of any joint's sphere into any primitive
    (out of a keep-in one), max(0, r_j - sigma_k d_k), margins not counted; ``share``: the share of the sample's frames in
    which any joint is inside a margin (m_k + r_j - sigma_k d_k > 0).  Primitives of weight 0 are ignored.  ``tracks``
    (as ``batch_tracks`` takes them; ``scene`` may then be None): the moving primitives of §25 count as well, every frame
    against its own records.  ``terrain`` (as ``batch_terrain`` takes it): the ground of §29 counts as well, with the vertical
    clearance e = p_y - h(p) in the place of a distance (a terrain of weight 0 is ignored).  Plain torch ops on the device the
    joints are on."""
    P = torch.as_tensor(joints)
    if P.dim() != 4 or P.shape[-1] != 3:
        raise ValueError(f"joints of shape {tuple(P.shape)} must be (B, T, J, 3)")
    B, T, J, _ = P.shape
    rec = batch_scene([] if scene is None else scene, B)
    r = joint_params(J, joint_radius)[:, 0].to(P.device, P.dtype)
    ln = torch.as_tensor(lengths).flatten().to(P.device)
    if ln.numel() != B:
        raise ValueError(f"lengths must hold {B} entries")
    trk = None if tracks is None else batch_tracks(tracks, B, T, ln.cpu())
    ground = None if terrain is None else batch_terrain(terrain, B)
    depth, share = P.new_zeros(B), P.new_zeros(B)
    for b in range(B):
        n = min(max(int(ln[b]), 0), T)
        live = rec[b][(rec[b][:, 0] != PAD) & (rec[b][:, 2] > 0)]
        if n == 0:
            continue
        deep, inside = P.new_zeros(()), torch.zeros(n, dtype=torch.bool, device=P.device)
        if live.shape[0]:
            q = live.to(P.device, P.dtype)
            sd = q[:, 1] * signed_distances(P[b, :n], live)  # (n, J, K)
            deep = (r[None, :, None] - sd).clamp(min=0).max()
            inside = ((q[:, 3] + r[None, :, None] - sd) > 0).any(-1).any(-1)
        if trk is not None and trk.shape[2]:
            q = trk[b, :n].to(P.device, P.dtype)[:, None]  # (n, 1, Km, REC)
            on = (q[..., 0] != PAD) & (q[..., 2] > 0)
            sd = q[..., 1] * track_distances(P[b, :n], trk[b, :n])  # (n, J, Km)
            deep = torch.maximum(deep, torch.where(on, (r[None, :, None] - sd).clamp(min=0), torch.zeros_like(sd)).max())
            inside = inside | (on & ((q[..., 3] + r[None, :, None] - sd) > 0)).any(-1).any(-1)
        if ground is not None and float(ground[1][b, 6]) > 0:
            g = ground[1][b].to(P.device, P.dtype)
            e = P[b, :n, :, 1] - _terrain_height(P[b, :n, :, 0], P[b, :n, :, 2], ground[0][b].to(P.device, P.dtype), g)  # (n, J)
            deep = torch.maximum(deep, (r[None] - e).clamp(min=0).max())
            inside = inside | ((g[7] + r[None] - e) > 0).any(-1)
        depth[b], share[b] = deep, inside.to(P.dtype).mean()
    return depth, share


# ---- tracks: primitives whose record differs from frame to frame ----------------------------------------
def _per_frame(cols, active):
    """``cols``: (value, width, name) per parameter, each a (width,) vector (a scalar for width 1) or (T, width) / (T,)
    per frame; ``active`` None or (T,) bool.  Returns T and the (T, width) float64 arrays.  ValueError for non-finite values,
    other shapes, per-frame lengths that disagree and no per-frame argument at all."""
    arrs, T = [], None
    if active is not None:
        active = np.asarray(active)
        if active.ndim != 1 or active.dtype != np.bool_:
            raise ValueError(f"active must be a (T,) bool array, not {active.dtype} of shape {active.shape}")
        T = active.shape[0]
    for v, n, name in cols:
        a = np.asarray(v.detach().cpu().numpy() if torch.is_tensor(v) else v, dtype=np.float64)
        if not np.isfinite(a).all():
            raise ValueError(f"{name} has non-finite values")
        if a.ndim == 0 and n == 1:
            a = a.reshape(1)
        if a.ndim == 1 and n == 1 and a.shape[0] != 1:
            a = a[:, None]  # (T,) -> (T, 1)
        if a.ndim == 1 and a.shape[0] == n:
            arrs.append(a)
            continue
        if a.ndim != 2 or a.shape[1] != n:
            raise ValueError(f"{name} of shape {np.shape(v)} must be ({n},) or (T, {n})" if n > 1 else
                             f"{name} of shape {np.shape(v)} must be a scalar or (T,)")
        if T is not None and a.shape[0] != T:
            raise ValueError(f"per-frame shapes disagree: {name} has {a.shape[0]} frames, another argument {T}")
        T = a.shape[0]
        arrs.append(a)
    if T is None:
        raise ValueError("a moving primitive needs a per-frame argument (T, .) or active= (T,)")
    return T, [np.broadcast_to(a, (T, a.shape[-1])) for a in arrs]


def _track(kind, cols, margin, weight, inside, active):
    """The (T, REC) float64 record stack of one track; a frame with ``active`` False is padding (kind 0, all zeros)."""
    T, arrs = _per_frame(list(cols) + [(margin, 1, "margin"), (weight, 1, "weight")], active)
    margin, weight = arrs[-2][:, 0], arrs[-1][:, 0]
    if (weight < 0).any():
        raise ValueError("weight must be finite and >= 0")
    rec = np.zeros((T, REC))
    rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3] = kind, -1.0 if inside else 1.0, weight, margin
    params = np.concatenate(arrs[:-2], axis=1)
    rec[:, 4:4 + params.shape[1]] = params
    if active is not None:
        rec[~np.asarray(active)] = 0.0
    return torch.from_numpy(rec)


def _all_positive(a, name):
    if (a <= 0).any():
        raise ValueError(f"{name} must be > 0")


def moving_sphere(centers, radius, *, margin=0.0, weight=1.0, inside=False, active=None):
    """A sphere whose centre (T, 3) (and radius, a scalar or (T,)) changes with the frame: the (T, REC) record stack of one
    track.  ``margin`` / ``weight`` (scalars or (T,)) / ``inside`` as ``sphere``; ``active`` (T,) bool: False leaves the
    track out of that frame."""
    T, (c, r) = _per_frame([(centers, 3, "centers"), (radius, 1, "radius")], active)
    _all_positive(r, "radius")
    return _track(SPHERE, [(c, 3, "centers"), (r, 1, "radius")], margin, weight, inside, active)


def moving_capsule(a, b, radius, *, margin=0.0, weight=1.0, inside=False, active=None):
    """A capsule with ends ``a`` and ``b`` (T, 3) per frame (a limb, a swinging bar)."""
    T, (pa, pb, r) = _per_frame([(a, 3, "a"), (b, 3, "b"), (radius, 1, "radius")], active)
    _all_positive(r, "radius")
    return _track(CAPSULE, [(pa, 3, "a"), (pb, 3, "b"), (r, 1, "radius")], margin, weight, inside, active)


def moving_box(centers, half_extents, yaw=0.0, *, margin=0.0, weight=1.0, inside=False, active=None):
    """A box with centre (T, 3), half extents (3,) or (T, 3) and yaw (radians about Y; a scalar or (T,)) per frame."""
    T, (c, h, y) = _per_frame([(centers, 3, "centers"), (half_extents, 3, "half_extents"), (yaw, 1, "yaw")], active)
    _all_positive(h, "every half extent")
    return _track(BOX, [(c, 3, "centers"), (h, 3, "half_extents"), (np.cos(y), 1, "yaw"), (np.sin(y), 1, "yaw")], margin, weight,
                  inside, active)


def moving_half_space(normals, offsets, *, margin=0.0, weight=1.0, inside=False, active=None):
    """A half-space with normal (3,) or (T, 3) (normalised here) and offset (a scalar or (T,)) per frame: a rising floor, a
    closing wall."""
    T, (n, o) = _per_frame([(normals, 3, "normals"), (offsets, 1, "offsets")], active)
    length = np.linalg.norm(n, axis=1, keepdims=True)
    if (length == 0).any():
        raise ValueError("normal must not be zero")
    return _track(HALF_SPACE, [(n / length, 3, "normals"), (o, 1, "offsets")], margin, weight, inside, active)


def check_tracks(rec, name="tracks"):
    """``rec`` (..., T, Km, REC), packed track records, as a float32 tensor, checked as ``check_records`` checks a scene's, with
    at most MAX_TRACKS of them a frame."""
    rec = torch.as_tensor(rec)
    if rec.dim() < 3:
        raise ValueError(f"{name} of shape {tuple(rec.shape)} must be (..., T, Km, {REC})")
    return check_records(rec, name, MAX_TRACKS)


def pack_tracks(tracks, T: int) -> torch.Tensor:
    """A list of track stacks (Tk, REC) as the (T, Km, REC) float32 records of the kernels (CPU): the first T frames of
    every track; frames past a track's own length are padding.  ValueError for more than MAX_TRACKS."""
    tracks = list(tracks)
    if len(tracks) > MAX_TRACKS:
        raise ValueError(f"{len(tracks)} tracks: a sample takes at most {MAX_TRACKS}")
    out = torch.zeros((int(T), len(tracks), REC), dtype=torch.float64)
    for k, tr in enumerate(tracks):
        tr = torch.as_tensor(tr)
        if tr.dim() != 2 or tr.shape[1] != REC:
            raise ValueError(f"track {k} of shape {tuple(tr.shape)} must be a (T, {REC}) record stack (moving_sphere / "
                             "moving_capsule / moving_box / moving_half_space / character_tracks)")
        n = min(int(T), tr.shape[0])
        out[:n, k] = tr[:n].to(torch.float64)
    return check_tracks(out.to(torch.float32))


def canvas_tracks(tracks, motion_offsets) -> torch.Tensor:
    """``tracks``, one list of track stacks per motion in that motion's canvas frames (or packed (total, Km, REC) records),
    as the (total, Km, REC) float32 records in canvas order of the canvas kernels: Km the longest list, the rest padding.
    ValueError for packed records that are not ``total`` frames long."""
    off = [int(v) for v in torch.as_tensor(motion_offsets).flatten().tolist()]
    M, total = len(off) - 1, off[-1]
    if torch.is_tensor(tracks) or isinstance(tracks, np.ndarray):
        rec = check_tracks(tracks)
        if rec.dim() != 3 or rec.shape[0] != total:
            raise ValueError(f"tracks of shape {tuple(rec.shape)} must be ({total}, Km, {REC}) in canvas order: shorter or longer "
                             "than the motions' lengths")
        return rec.contiguous()
    tracks = list(tracks)
    if len(tracks) != M or any(_is_stack(t) for t in tracks):
        raise ValueError(f"tracks must hold one list of track stacks per motion ({M}), in its canvas frames")
    packed = [pack_tracks(t, off[m + 1] - off[m]) for m, t in enumerate(tracks)]
    out = torch.zeros((total, max([p.shape[1] for p in packed] + [0]), REC))
    for m, p in enumerate(packed):
        out[off[m]:off[m + 1], :p.shape[1]] = p
    return out


def _is_stack(v):
    return (torch.is_tensor(v) or isinstance(v, np.ndarray)) and v.ndim == 2


def batch_tracks(tracks, N: int, T: int, lengths=None) -> torch.Tensor:
    """``tracks``, one list of track stacks shared by N samples or one list per sample (or packed records (Tt, Km, REC) /
    (N, Tt, Km, REC)), as (N, T, Km, REC) float32 records: Km the longest list, shorter ones and frames past a track's own
    length padded with kind 0, frames past T dropped.  ValueError for packed records with fewer frames than a sample's
    ``lengths`` entry (T without ``lengths``)."""
    T = int(T)
    if torch.is_tensor(tracks) or isinstance(tracks, np.ndarray):
        rec = check_tracks(tracks)
        if rec.dim() == 3:
            rec = rec[None].expand(N, -1, -1, -1)
        if rec.dim() != 4 or rec.shape[0] != N:
            raise ValueError(f"tracks of shape {tuple(rec.shape)} must be (T, Km, {REC}) or ({N}, T, Km, {REC})")
        need = T if lengths is None else min(T, max([int(v) for v in torch.as_tensor(lengths).flatten().tolist()] + [0]))
        if rec.shape[1] < need:
            raise ValueError(f"tracks hold {rec.shape[1]} frames: shorter than a sample's length {need}")
        out = torch.zeros((N, T, rec.shape[2], REC))
        n = min(T, rec.shape[1])
        out[:, :n] = rec[:, :n]
        return out
    tracks = list(tracks)
    if all(_is_stack(t) for t in tracks):
        return pack_tracks(tracks, T)[None].expand(N, -1, -1, -1).contiguous()
    if len(tracks) != N or any(_is_stack(t) for t in tracks):
        raise ValueError(f"tracks must be one list of track stacks, or one list per sample ({N}), not {len(tracks)} entries")
    packed = [pack_tracks(t, T) for t in tracks]
    out = torch.zeros((N, T, max(p.shape[1] for p in packed), REC))
    for i, p in enumerate(packed):
        out[i, :, :p.shape[1]] = p
    return out


BOUND_REL, BOUND_ABS = 1e-3, 1e-3  # the broad phase's ball is inflated by this share of its radius plus this many metres


def track_bounds(records) -> torch.Tensor:
    """The broad phase of the kernels: for packed track records (..., T, Km, REC) the (..., T, 4) float32 balls (centre,
    radius) that contain, per frame, every keep-out track of weight > 0 inflated by its margin, computed in float64 and
    inflated by BOUND_REL of the radius plus BOUND_ABS metres, so that float32 rounding in the kernel cannot skip a record
    that penalises.  A joint of radius r farther than radius + r from the centre touches none of the frame's tracks.  Radius
    +inf for a frame with a half-space or a keep-in track of weight > 0 (never skipped), -inf for a frame without a live
    track (always skipped)."""
    rec = torch.as_tensor(records).detach().cpu().to(torch.float64)
    if rec.dim() < 3 or rec.shape[-1] != REC:
        raise ValueError(f"records of shape {tuple(rec.shape)} must be (..., T, Km, {REC})")
    lead, Km = rec.shape[:-2], rec.shape[-2]
    q = rec.reshape(math.prod(lead), Km, REC).numpy()
    kind, live = q[..., 0], (q[..., 0] != PAD) & (q[..., 2] > 0)
    m = np.maximum(q[..., 3], 0.0)
    centre = np.where((kind == CAPSULE)[..., None], 0.5 * (q[..., 4:7] + q[..., 7:10]), q[..., 4:7])
    reach = np.where(kind == SPHERE, q[..., 7], np.where(kind == CAPSULE, 0.5 * np.linalg.norm(q[..., 7:10] - q[..., 4:7], axis=-1)
                                                         + q[..., 10], np.linalg.norm(q[..., 7:10], axis=-1))) + m
    count = live.sum(-1)
    mid = (centre * live[..., None]).sum(1) / np.maximum(count, 1)[:, None]
    mid = mid.astype(np.float32).astype(np.float64)  # the centre the kernel reads
    far = np.where(live, np.linalg.norm(centre - mid[:, None], axis=-1) + reach, 0.0).max(-1) if Km else np.zeros(q.shape[0])
    radius = far * (1.0 + BOUND_REL) + BOUND_ABS
    unbounded = (live & ((kind == HALF_SPACE) | (q[..., 1] < 0))).any(-1)
    radius = np.where(unbounded, np.inf, np.where(count > 0, radius, -np.inf))
    out = np.concatenate([np.where((count > 0)[:, None], mid, 0.0), radius[:, None]], axis=1)
    return torch.from_numpy(out).to(torch.float32).reshape(*lead, 4)


def _rot_y(p, yaw, inverse=False):
    """R_y(yaw) p (R_y(-yaw) p with ``inverse``) of points (..., 3): x' = cos x + sin z, z' = -sin x + cos z; in p's dtype."""
    yaw = -float(yaw) if inverse else float(yaw)
    c, s = math.cos(yaw), math.sin(yaw)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    return torch.stack([c * x + s * z, y, -s * x + c * z], -1)


def _shift(p, position):
    x, z = (float(v) for v in position)
    return torch.tensor([x, 0.0, z], dtype=p.dtype, device=p.device)


def to_world(joints, position, yaw):
    """Joints (..., 3) of a character's own frame (``recover_from_ric``'s: it starts at the origin with heading 0) in the
    world: p_world = R_y(yaw) p + (x, 0, z) with ``position`` = (x, z).  In the joints' dtype, on their device."""
    p = torch.as_tensor(joints)
    return _rot_y(p, yaw) + _shift(p, position)


def to_local(joints, position, yaw):
    """The inverse of ``to_world``: p = R_y(-yaw) (p_world - (x, 0, z))."""
    p = torch.as_tensor(joints)
    return _rot_y(p - _shift(p, position), yaw, inverse=True)


def records_to_local(records, position, yaw) -> torch.Tensor:
    """Packed records (..., REC) given in the world, in the frame of a character at ``position`` = (x, z) turned by ``yaw``
    (``to_local`` of the primitives): centres and ends moved, a box's yaw reduced by ``yaw``, a half-space's normal turned
    and its offset reduced by n . (x, 0, z).  Float64; padding stays padding."""
    q = torch.as_tensor(records).detach().cpu().to(torch.float64).clone()
    if q.shape[-1] != REC:
        raise ValueError(f"records of shape {tuple(q.shape)} must be (..., {REC})")
    kind = q[..., 0]
    point = (kind == SPHERE) | (kind == CAPSULE) | (kind == BOX)
    cap, box_, half = kind == CAPSULE, kind == BOX, kind == HALF_SPACE
    a, b = to_local(q[..., 4:7], position, yaw), to_local(q[..., 7:10], position, yaw)
    n = _rot_y(q[..., 4:7], yaw, inverse=True)
    off = q[..., 7] - (q[..., 4:7] * _shift(q, position)).sum(-1)
    c, s, cy, sy = q[..., 10].clone(), q[..., 11].clone(), math.cos(float(yaw)), math.sin(float(yaw))
    q[..., 4:7] = torch.where(point[..., None], a, torch.where(half[..., None], n, q[..., 4:7]))
    q[..., 7:10] = torch.where(cap[..., None], b, q[..., 7:10])
    q[..., 7] = torch.where(half, off, q[..., 7])
    q[..., 10] = torch.where(box_, c * cy + s * sy, q[..., 10])
    q[..., 11] = torch.where(box_, s * cy - c * sy, q[..., 11])
    return q


def character_tracks(joints, radius=0.08, *, margin=0.0, weight=1.0, bones=None):
    """A generated character as an obstacle: one capsule track of ``radius`` along every bone of ``joints`` (T, J, 3), 21 for
    the 22-joint skeleton, ends at the joints.  ``bones``: (parent, child) pairs; by default the tree of the skeleton with J
    joints in ``motion_features.SKELETONS`` (the one forward kinematics walks).  ``margin`` / ``weight`` as ``capsule``."""
    P = torch.as_tensor(joints).detach().cpu().to(torch.float64)
    if P.dim() != 3 or P.shape[-1] != 3:
        raise ValueError(f"joints of shape {tuple(P.shape)} must be (T, J, 3)")
    if bones is None:
        from .motion_features import SKELETONS
        trees = {sk.joints: sk.parents for sk in SKELETONS.values()}
        if P.shape[1] not in trees:
            raise ValueError(f"no skeleton with {P.shape[1]} joints: give bones= as (parent, child) pairs")
        bones = [(p, c) for c, p in enumerate(trees[P.shape[1]]) if p >= 0]
    bones = [(int(p), int(c)) for p, c in bones]
    if any(not (0 <= p < P.shape[1] and 0 <= c < P.shape[1]) for p, c in bones):
        raise ValueError(f"bones must name joints in [0, {P.shape[1]})")
    return [moving_capsule(P[:, p], P[:, c], radius, margin=margin, weight=weight) for p, c in bones]


def track_distances(p: torch.Tensor, records: torch.Tensor) -> torch.Tensor:
    """d(R[t, k]; p[t, j]) of points ``p`` (T, J, 3) to the per-frame records (T, Km, REC): (T, J, Km) in p's dtype on p's
    device; 0 for padding.  Plain torch ops, every kind evaluated on every record and selected by the record's kind."""
    q = records.detach().to(p.device, p.dtype)[:, None]  # (T, 1, Km, REC)
    x = p[:, :, None]  # (T, J, 1, 3)
    kind = q[..., 0]
    d_sphere = (x - q[..., 4:7]).norm(dim=-1) - q[..., 7]
    e, v = q[..., 7:10] - q[..., 4:7], x - q[..., 4:7]
    den = (e * e).sum(-1)
    h = torch.where(den > 0, (v * e).sum(-1) / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(den)).clamp(0, 1)
    d_capsule = (v - h[..., None] * e).norm(dim=-1) - q[..., 10]
    c, s = q[..., 10], q[..., 11]
    dx, dz = x[..., 0] - q[..., 4], x[..., 2] - q[..., 6]
    loc = torch.stack([c * dx - s * dz, x[..., 1] - q[..., 5], s * dx + c * dz], -1)
    qq = loc.abs() - q[..., 7:10]
    d_box = qq.clamp(min=0).norm(dim=-1) + qq.max(dim=-1).values.clamp(max=0)
    d_half = (x * q[..., 4:7]).sum(-1) - q[..., 7]
    zero = torch.zeros_like(d_half)
    return torch.where(kind == SPHERE, d_sphere, torch.where(kind == CAPSULE, d_capsule, torch.where(
        kind == BOX, d_box, torch.where(kind == HALF_SPACE, d_half, zero))))


# ---- terrain: a height-map ground ----------------------------------------------------------------------
class Terrain:
    """A height field: ``heights`` (Gz, Gx) float32 on the CPU and ``record`` (8,) float64 = origin x, origin z, cos yaw,
    sin yaw, 1 / cell_x, 1 / cell_z, weight, margin.  Made by ``heightfield`` / ``ramp`` / ``stairs``."""

    def __init__(self, heights, record):
        self.heights, self.record = heights, record


def check_terrain(heights, record, name="terrain"):
    """``heights`` (..., Gz, Gx) and ``record`` (..., 8) as float32 tensors; ValueError for a grid under 2 or over MAX_GRID on
    either side, non-finite values, a cell <= 0 and a weight < 0."""
    h, r = torch.as_tensor(heights), torch.as_tensor(record)
    if h.dim() < 2 or not h.is_floating_point():
        raise ValueError(f"{name} heights of shape {tuple(h.shape)} must be floating point (..., Gz, Gx)")
    if not all(2 <= int(g) <= MAX_GRID for g in h.shape[-2:]):
        raise ValueError(f"{name} grid of {h.shape[-2]} x {h.shape[-1]} samples: 2 to {MAX_GRID} are allowed on either side")
    if r.shape[-1:] != (TERRAIN_REC,) or r.shape[:-1] != h.shape[:-2] or not r.is_floating_point():
        raise ValueError(f"{name} record of shape {tuple(r.shape)} must be floating point {tuple(h.shape[:-2]) + (TERRAIN_REC,)}")
    if not bool(torch.isfinite(h).all()) or not bool(torch.isfinite(r).all()):
        raise ValueError(f"{name} has non-finite values")
    if bool((r[..., 4:6] <= 0).any()):
        raise ValueError(f"{name}: a cell must be > 0")
    if bool((r[..., 6] < 0).any()):
        raise ValueError(f"{name}: the weight must be >= 0")
    return h.detach().to(torch.float32), r.detach().to(torch.float32)


def heightfield(heights, cell, origin=(0.0, 0.0), yaw=0.0, *, margin=0.0, weight=1.0) -> Terrain:
    """A terrain from ``heights`` (Gz, Gx) in metres: sample [k, i] stands at local (i cell_x, k cell_z), local = R_y(-yaw)
    (p_xz - origin).  ``cell``: a scalar or (cell_x, cell_z), metres > 0.  ``margin`` / ``weight`` as a primitive's.  ValueError
    for non-finite heights, cell <= 0, weight < 0 and a grid under 2 or over MAX_GRID on either side."""
    h = torch.as_tensor(heights.detach().cpu() if torch.is_tensor(heights) else np.asarray(heights, dtype=np.float64))
    if h.dim() != 2:
        raise ValueError(f"heights of shape {tuple(h.shape)} must be (Gz, Gx)")
    c = np.asarray(cell, dtype=np.float64).reshape(-1)
    if c.size not in (1, 2):
        raise ValueError("cell must be a scalar or (cell_x, cell_z)")
    cx, cz = (_positive(v, "cell") for v in (c[0], c[-1]))
    yaw, margin, weight = float(yaw), float(margin), float(weight)
    if not (math.isfinite(yaw) and math.isfinite(margin)):
        raise ValueError("yaw and margin must be finite")
    if not (math.isfinite(weight) and weight >= 0):
        raise ValueError(f"weight must be finite and >= 0, not {weight}")
    rec = torch.tensor(_vec(origin, 2, "origin") + [math.cos(yaw), math.sin(yaw), 1.0 / cx, 1.0 / cz, weight, margin],
                       dtype=torch.float64)
    hh, _ = check_terrain(h.to(torch.float64), rec)
    return Terrain(hh.contiguous(), rec)


def _corner(start, yaw, width):
    """The grid's corner for a strip of ``width`` centred on ``start`` = (x, z) that runs along local +X."""
    x, z = _vec(start, 2, "start")
    half = 0.5 * _positive(width, "width")
    c, s = math.cos(float(yaw)), math.sin(float(yaw))
    return (x - s * half, z - c * half)  # start + R_y(yaw) (0, 0, -width / 2)


def ramp(start, yaw, length, rise, width, *, margin=0.0, weight=1.0) -> Terrain:
    """A ramp of ``width`` metres centred on ``start`` = (x, z): height 0 at ``start`` and before it, rising linearly by ``rise``
    metres (negative: down) over ``length`` metres along R_y(yaw) (1, 0, 0), flat at ``rise`` behind.  A 2 x 2 grid."""
    length, rise = _positive(length, "length"), float(rise)
    if not math.isfinite(rise):
        raise ValueError("rise must be finite")
    return heightfield([[0.0, rise], [0.0, rise]], (length, _positive(width, "width")), _corner(start, yaw, width), yaw,
                       margin=margin, weight=weight)


def stairs(start, yaw, steps, rise, run, width, cell=0.05, *, margin=0.0, weight=1.0) -> Terrain:
    """``steps`` stairs of ``rise`` metres each (negative: down) and treads of ``run`` metres, ``width`` metres wide and centred
    on ``start`` = (x, z), climbing along R_y(yaw) (1, 0, 0): height 0 at ``start`` and before it, s ``rise`` on tread s, the top
    tread's height behind.  Rasterised at ``cell`` metres along the climb (``run`` is rounded to whole cells, two at least):
    every riser spans one cell, the first from ``start`` on."""
    steps = int(steps)
    if steps < 1:
        raise ValueError("steps must be >= 1")
    cell, rise = _positive(cell, "cell"), float(rise)
    if not math.isfinite(rise):
        raise ValueError("rise must be finite")
    per = max(2, int(round(_positive(run, "run") / cell)))
    i = np.arange(steps * per + 1)
    row = rise * np.minimum(steps, (i + per - 1) // per)
    return heightfield(np.stack([row, row]), (cell, _positive(width, "width")), _corner(start, yaw, width), yaw, margin=margin,
                       weight=weight)


def batch_terrain(terrain, N: int):
    """``terrain``, one ``Terrain`` shared by N samples or a list of one per sample, as ``(heights (N, Gz, Gx), records (N, 8))``
    float32 on the CPU: Gz and Gx the largest of the list, smaller grids padded by repeating their last row and column (which
    changes no height: past its edge a terrain continues flat)."""
    items = [terrain] * N if isinstance(terrain, Terrain) else list(terrain)
    if len(items) != N or not all(isinstance(t, Terrain) for t in items):
        raise ValueError(f"terrain must be one terrain made by heightfield / ramp / stairs, or a list of one per sample ({N})")
    if N == 0:
        return torch.zeros((0, 2, 2)), torch.zeros((0, TERRAIN_REC))
    gz, gx = max(t.heights.shape[0] for t in items), max(t.heights.shape[1] for t in items)
    hs = []
    for t in items:
        h = t.heights
        h = torch.cat([h, h[-1:].expand(gz - h.shape[0], -1)], 0)
        hs.append(torch.cat([h, h[:, -1:].expand(-1, gx - h.shape[1])], 1))
    return check_terrain(torch.stack(hs), torch.stack([t.record for t in items]))


def _terrain_height(p_x, p_z, h, r):
    """h(p) of points with coordinates ``p_x`` / ``p_z`` (...) over the grid ``h`` (Gz, Gx) with record ``r`` (8,), both in the
    points' dtype on their device."""
    gz, gx = h.shape
    dx, dz = p_x - r[0], p_z - r[1]
    u = ((r[2] * dx - r[3] * dz) * r[4]).clamp(0, gx - 1)
    v = ((r[3] * dx + r[2] * dz) * r[5]).clamp(0, gz - 1)
    i, k = u.floor().long().clamp(max=gx - 2), v.floor().long().clamp(max=gz - 2)
    fu, fv = u - i, v - k
    lo = h[k, i] + fu * (h[k, i + 1] - h[k, i])
    hi = h[k + 1, i] + fu * (h[k + 1, i + 1] - h[k + 1, i])
    return lo + fv * (hi - lo)


def terrain_height(terrain: Terrain, xz) -> torch.Tensor:
    """h at the points ``xz`` (..., 2) = (x, z): (...) in xz's dtype on its device.  Plain torch ops."""
    p = torch.as_tensor(xz)
    if p.shape[-1:] != (2,) or not p.is_floating_point():
        raise ValueError(f"xz of shape {tuple(p.shape)} must be floating point (..., 2)")
    return _terrain_height(p[..., 0], p[..., 1], terrain.heights.to(p.device, p.dtype), terrain.record.to(p.device, p.dtype))


def terrain_to_local(terrain: Terrain, position, yaw) -> Terrain:
    """A terrain given in the world, in the frame of a character at ``position`` = (x, z) turned by ``yaw`` (``to_local`` of the
    ground): the origin moved and the yaw reduced by ``yaw``; the heights are shared, only the record changes."""
    r = terrain.record.clone()
    o = to_local(torch.tensor([float(r[0]), 0.0, float(r[1])], dtype=torch.float64), position, yaw)
    cy, sy = math.cos(float(yaw)), math.sin(float(yaw))
    c, s = float(r[2]), float(r[3])
    r[0], r[1], r[2], r[3] = o[0], o[2], c * cy + s * sy, s * cy - c * sy
    return Terrain(terrain.heights, r)


def check_stand(stand, shape, name="stand"):
    """Stand weights as a float32 tensor of ``shape``; ValueError for another shape, non-finite or negative values."""
    s = torch.as_tensor(stand)
    if tuple(s.shape) != tuple(shape):
        raise ValueError(f"{name} of shape {tuple(s.shape)} must be {tuple(shape)}")
    s = s.detach().to(torch.float32)
    if not bool(torch.isfinite(s).all()) or bool((s < 0).any()):
        raise ValueError(f"{name} must be finite and >= 0")
    return s


def _terrain_args(terrain, stand, N, stand_shape, dev):
    """The grids, records and stand weights (None without) on the device, and the ctypes arguments between track_bounds and the
    sizes of the mdm_*_terrain_* calls."""
    hs, rec = batch_terrain(terrain, N)
    hs, rec = hs.to(dev).contiguous(), rec.to(dev).contiguous()
    st = None if stand is None else check_stand(stand, stand_shape).to(dev).contiguous()
    return (hs, rec, st), (hs.data_ptr(), rec.data_ptr(), hs.shape[2], hs.shape[1], L.ptr(st))


def _scene_args(scene, N, J, joint_radius, joint_weights, dev):
    rec = batch_scene(scene, N).to(dev).contiguous()
    jp = joint_params(J, joint_radius, joint_weights)[None].expand(N, -1, -1).to(dev).contiguous()
    return rec, jp


def _track_args(tracks, N, T, lengths, bounds, dev):
    """The (N, T, Km, REC) records on the device and their balls (None without the broad phase or without tracks)."""
    trk = batch_tracks(tracks, N, T, lengths)
    bnd = track_bounds(trk).to(dev).contiguous() if bounds and trk.shape[2] else None
    return trk.to(dev).contiguous(), bnd


def _target_args(targets, weights, shape, dev):
    """The targets of ``shape`` and the weights broadcast to it on the device, or (None, None) without either."""
    if (targets is None) != (weights is None):
        raise ValueError("targets and weights go together: give both or neither")
    if targets is None:
        return None, None
    tg = torch.as_tensor(targets).to(dev, torch.float32).contiguous()
    if tuple(tg.shape) != shape:
        raise ValueError(f"targets of shape {tuple(tg.shape)} must be {shape}")
    return tg, torch.broadcast_to(torch.as_tensor(weights).to(dev, torch.float32), shape).contiguous()


def _loss_grad(family, head, tail, trk=None, bnd=None, ground=()):
    """One call of mdm_{family}_{scene|tracks|terrain}_loss_grad, the lowest entry whose signature carries what is given:
    ``head`` up to the joint parameters, the (..., Km, REC) track records ``trk`` and their balls, the terrain arguments
    ``ground`` (on top of the tracks arguments), ``tail`` from the sizes on."""
    mid = () if trk is None else (trk.data_ptr() if trk.shape[-2] else 0, trk.shape[-2], L.ptr(bnd))
    name = f"mdm_{family}_{'terrain' if ground else 'scene' if trk is None else 'tracks'}_loss_grad"
    L.check(getattr(L.lib(), name)(*head, *mid, *ground, *tail), name)


@torch.no_grad()
def scene_loss_grad(x0: torch.Tensor, lengths, mean, std, scene, joint_radius=None, joint_weights=None, targets=None,
                    weights=None, tracks=None, bounds=True, terrain=None, stand=None):
    """Loss (B,) and gradient (B, T, F) of L_scene (module docstring), plus §14's target term when ``targets`` (B, T, J, 3)
    and ``weights`` are given, with respect to the normalised features ``x0`` (B, T, F) on a GPU, through
    ``mdm_joint_scene_loss_grad``.  ``scene``: one list of primitives, or one per sample; ``mean`` / ``std``: (F,) or (B, F).
    The gradient is exactly 0 in every column past 3 J and in every frame at or past ``lengths[b]``.  ``tracks`` (as
    ``batch_tracks`` takes them; ``scene`` may then be None) adds L_tracks through ``mdm_joint_tracks_loss_grad``, behind the
    broad phase of ``track_bounds`` (``bounds=False``: without it; the result is the same bit for bit).  ``terrain`` (as
    ``batch_terrain`` takes it; ``scene`` and ``tracks`` may then be None) adds L_terrain through
    ``mdm_joint_terrain_loss_grad``, with the stand weights ``stand`` (B, T, J) >= 0 (None: all 0)."""
    L.require_cuda(x0)
    if stand is not None and terrain is None:
        raise ValueError("stand weights need a terrain")
    dev = x0.device
    x = x0.detach().to(torch.float32).contiguous()
    if x.dim() != 3:
        raise ValueError(f"x0 of shape {tuple(x.shape)} must be (B, T, F)")
    B, T, F = x.shape
    J = joints_for_feats(F)
    rec, jp = _scene_args([] if scene is None else scene, B, J, joint_radius, joint_weights, dev)
    K = rec.shape[1]
    if not 1 <= T <= max_frames(F, K):
        raise ValueError(f"T = {T}: with {K} primitives the control kernels take 1 to {max_frames(F, K)} frames at F = {F}")
    tg, w = _target_args(targets, weights, (B, T, J, 3), dev)
    mean_t = _rows(mean, B, F, "mean").to(dev).contiguous()
    std_t = _rows(std, B, F, "std").to(dev).contiguous()
    ln = torch.as_tensor(lengths).to(dev, torch.int32).contiguous()
    if tuple(ln.shape) != (B,):
        raise ValueError(f"lengths must hold {B} entries")
    loss = torch.empty(B, device=dev)
    grad = torch.empty_like(x)
    head = (x.data_ptr(), ln.data_ptr(), mean_t.data_ptr(), std_t.data_ptr(), L.ptr(tg), L.ptr(w), rec.data_ptr() if K else 0, K,
            jp.data_ptr())
    tail = (B, T, F, loss.data_ptr(), grad.data_ptr(), L.stream_ptr())
    with torch.cuda.device(dev):
        trk = bnd = None
        if tracks is not None or terrain is not None:
            trk, bnd = _track_args([] if tracks is None else tracks, B, T, ln.cpu(), bounds, dev)
        keep, ground = ((), ()) if terrain is None else _terrain_args(terrain, stand, B, (B, T, J), dev)
        _loss_grad("joint", head, tail, trk, bnd, ground)
    return loss, grad


@torch.no_grad()
def canvas_scene_loss_grad(rows: torch.Tensor, motion_offsets, frame_rows, mean, std, scene, joint_radius=None,
                           joint_weights=None, targets=None, weights=None, tracks=None, bounds=True, terrain=None, stand=None):
    """``scene_loss_grad`` over the canvases of M long motions, as ``motion_control.canvas_loss_grad``: loss (M,) and gradient
    (total, F) dense in canvas order, through ``mdm_canvas_scene_loss_grad``.  ``scene``: one list of primitives, or one per
    motion, in the canvas frame; ``targets`` (total, J, 3) in canvas order and ``weights``, or neither.  Any canvas length.
    ``tracks``: one list of track stacks per motion, in canvas frames (or packed (total, Km, REC) records in canvas order),
    through ``mdm_canvas_tracks_loss_grad``; ``bounds`` as in ``scene_loss_grad``.  ``terrain``: one terrain, or one per motion,
    in the canvas frame, with ``stand`` (total, J) in canvas order or None, through ``mdm_canvas_terrain_loss_grad``."""
    L.require_cuda(rows)
    if stand is not None and terrain is None:
        raise ValueError("stand weights need a terrain")
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
    rec, jp = _scene_args([] if scene is None else scene, M, J, joint_radius, joint_weights, dev)
    K = rec.shape[1]
    tg, w = _target_args(targets, weights, (total, J, 3), dev)
    mean_t = _rows(mean, M, F, "mean").to(dev).contiguous()
    std_t = _rows(std, M, F, "std").to(dev).contiguous()
    off_d, fr_d = off.to(dev, torch.int32), fr.to(dev, torch.int32)
    loss = torch.zeros(M, device=dev)
    grad = torch.zeros((total, F), device=dev)
    ws = torch.empty(max(int(L.lib().mdm_canvas_control_workspace_floats(total, F)), 1), device=dev)
    head = (x.data_ptr(), off_d.data_ptr(), fr_d.data_ptr(), mean_t.data_ptr(), std_t.data_ptr(), L.ptr(tg), L.ptr(w),
            rec.data_ptr() if K else 0, K, jp.data_ptr())
    tail = (M, F, loss.data_ptr(), grad.data_ptr(), ws.data_ptr(), L.stream_ptr())
    with torch.cuda.device(dev):
        trk = bnd = None
        if tracks is not None or terrain is not None:
            trk = canvas_tracks([[] for _ in range(M)] if tracks is None else tracks, off)
            bnd = track_bounds(trk).to(dev).contiguous() if bounds and trk.shape[1] else None
            trk = trk.to(dev).contiguous()
        keep, ground = ((), ()) if terrain is None else _terrain_args(terrain, stand, M, (total, J), dev)
        _loss_grad("canvas", head, tail, trk, bnd, ground)
    return loss, grad


# ---- characters sampled together: every row avoids and reaches for its partners' current estimate ----------
class Contact(tuple):
    """One contact: (a, joint_a, b, joint_b, first, last, weight, meet), frames [first, last).  Made by ``contact``."""


def contact(a, joint_a, b, joint_b, frames, weight=1.0, meet=0.5) -> Contact:
    """Joint ``joint_a`` of character ``a`` and joint ``joint_b`` of character ``b`` meet in ``frames`` (a ``range`` of step 1 or
    consecutive frame numbers) at m = W_a + meet (W_b - W_a): ``meet`` 0 lets b do all the reaching, 0.5 is halfway, 1 lets a.
    ``weight`` >= 0 is the target weight of both.  ``a`` / ``b`` are character indices of a scene in
    ``DDPMTrainer.generate_together`` and batch rows in ``partner_tables``.  ValueError for a == b, negative indices, frames
    that are not consecutive or run backwards (``first > last``), a weight < 0 and a ``meet`` outside [0, 1] or non-finite."""
    a, joint_a, b, joint_b = (int(v) for v in (a, joint_a, b, joint_b))
    if min(a, joint_a, b, joint_b) < 0:
        raise ValueError("a contact's characters and joints must be >= 0")
    if a == b:
        raise ValueError("a contact joins two different characters")
    if isinstance(frames, range):
        if frames.step != 1:
            raise ValueError("a contact's frames must be consecutive (a range of step 1)")
        first, last = frames.start, frames.stop
    else:
        fr = [int(f) for f in frames]
        if any(y != x + 1 for x, y in zip(fr, fr[1:])):
            raise ValueError("a contact's frames must be consecutive")
        first, last = (fr[0], fr[-1] + 1) if fr else (0, 0)
    if first > last or first < 0:
        raise ValueError(f"a contact's frames must run forward from a frame >= 0 (first > last: {first} > {last})")
    weight, meet = float(weight), float(meet)
    if not (math.isfinite(weight) and weight >= 0):
        raise ValueError(f"weight must be finite and >= 0, not {weight}")
    if not (math.isfinite(meet) and 0.0 <= meet <= 1.0):
        raise ValueError(f"meet must lie in [0, 1], not {meet}")
    return Contact((a, joint_a, b, joint_b, int(first), int(last), weight, meet))


def skeleton_bones(J: int):
    """The (parent, child) pairs of the skeleton with J joints in ``motion_features.SKELETONS``: ``character_tracks``' default."""
    from .motion_features import SKELETONS
    trees = {sk.joints: sk.parents for sk in SKELETONS.values()}
    if J not in trees:
        raise ValueError(f"no skeleton with {J} joints: give bones= as (parent, child) pairs")
    return [(p, c) for c, p in enumerate(trees[J]) if p >= 0]


class PartnerTables:
    """The host half of ``mdm_partner_tracks``, made by ``partner_tables``: ``partner_rows`` (B, Pm) int32, ``bones`` (nb, 2)
    int32, ``placements`` (B, 4) float32 = x, z, cos yaw, sin yaw, ``contacts`` (Nc, 8) int32 words (row a, joint a, row b,
    joint b, first, last, the bits of meet as fp32, 0), ``weights`` (B, T, J, 3) float32, constant over a run (the static control
    weights plus every contact's), ``lengths`` (B,) int32, and the scalars ``radius``, ``margin``, ``weight``, ``Ks``, ``Km``,
    ``Pm``, ``nb``, ``B``, ``T``, ``J``; ``pose`` (B, 3) float64 keeps the x, z, yaw the placements were made from.  All on the CPU."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def partner_tables(scenes_rows, placements, lengths, bones=None, *, T, J, contacts=(), radius=0.08, margin=0.05, weight=5.0,
                   static_tracks=0, control_weights=None, avoid=True) -> PartnerTables:
    """The tables of characters sampled together.  ``scenes_rows``: one list of batch rows per scene (every row of a scene is
    a partner of every other; a row in no scene, or alone in one, has none); ``placements`` (B, 3) = x, z, yaw per row;
    ``lengths`` (B,); ``bones``: (parent, child) pairs, by default the skeleton's (``skeleton_bones(J)``); ``contacts``:
    ``contact(...)`` entries whose ``a`` / ``b`` are batch rows of one scene; ``radius`` / ``margin`` / ``weight``: of every partner
    capsule; ``static_tracks`` = Ks, the number of user tracks in front of the partner slots; ``control_weights`` (B, T, J, 3) or
    None: the static target weights the contacts must not land on; ``avoid=False``: no partner slots at all (Pm = 0), the
    scenes then only say which rows a contact may join.  Slot q of row b holds the q-th other row of its scene in
    the scene's order, -1 behind; bone i of slot q is track Ks + q nb + i.  A contact's weight is written on all three axes
    of (a, t, joint_a) and (b, t, joint_b) for first <= t < min(last, n_a, n_b); a side that does none of the reaching (a at
    ``meet`` 0, b at 1) carries weight 0: its target would be its own joint.  ValueError for a row outside [0, B) or in two
    scenes, Ks + Pm nb over MAX_TRACKS, a bone or contact joint outside [0, J), contact rows that are not two rows of one
    scene, a contact on a (row, frame, joint) with a non-zero static weight, two contacts on one (row, frame, joint), and
    non-finite placements, radius <= 0, weight < 0."""
    T, J, Ks = int(T), int(J), int(static_tracks)
    pl = np.asarray(placements.detach().cpu().numpy() if torch.is_tensor(placements) else placements, dtype=np.float64)
    if pl.ndim != 2 or pl.shape[1] != 3:
        raise ValueError(f"placements of shape {pl.shape} must be (B, 3) = x, z, yaw")
    if not np.isfinite(pl).all():
        raise ValueError("placements have non-finite values")
    B = pl.shape[0]
    ln = L.check_lengths(lengths, B, T, least=0).to(torch.int32)
    radius, margin, weight = _positive(radius, "radius"), float(margin), float(weight)
    if not math.isfinite(margin):
        raise ValueError("margin must be finite")
    if not (math.isfinite(weight) and weight >= 0):
        raise ValueError(f"weight must be finite and >= 0, not {weight}")
    bones = [(int(p), int(c)) for p, c in (skeleton_bones(J) if bones is None else bones)]
    if any(not (0 <= p < J and 0 <= c < J) for p, c in bones):
        raise ValueError(f"bones must name joints in [0, {J})")
    nb = len(bones)
    scene_of = {}
    scenes_rows = [[int(r) for r in rows] for rows in scenes_rows]
    for s, rows in enumerate(scenes_rows):
        for r in rows:
            if not 0 <= r < B:
                raise ValueError(f"scene {s} names row {r}: outside [0, {B})")
            if r in scene_of:
                raise ValueError(f"row {r} is in two scenes (or twice in one)")
            scene_of[r] = s
    Pm = max([len(rows) - 1 for rows in scenes_rows] + [0]) if avoid else 0
    if not 0 <= Ks <= MAX_TRACKS or Ks + Pm * nb > MAX_TRACKS:
        raise ValueError(f"{Ks} static tracks + {Pm} partners x {nb} bones = {Ks + Pm * nb} tracks a frame: at most {MAX_TRACKS} "
                         "are allowed; give a bones= subset (fewer capsules per partner)")
    prow = np.full((B, Pm), -1, dtype=np.int32)
    for rows in scenes_rows:
        for r in rows:
            others = [p for p in rows if p != r][:Pm]
            prow[r, :len(others)] = others
    w = torch.zeros((B, T, J, 3))
    if control_weights is not None:
        cw = torch.as_tensor(control_weights).detach().to("cpu", torch.float32)
        if tuple(cw.shape) != (B, T, J, 3):
            raise ValueError(f"control_weights of shape {tuple(cw.shape)} must be {(B, T, J, 3)}")
        w = cw.clone()
    taken = w.abs().sum(-1) != 0  # (B, T, J)
    table = np.zeros((len(contacts), 8), dtype=np.int32)
    for i, c in enumerate(contacts):
        if not isinstance(c, Contact):
            raise ValueError("contacts is a list of entries made by motion_scene.contact")
        a, ja, b, jb, first, last, cwt, meet = c
        if not (0 <= a < B and 0 <= b < B) or scene_of.get(a, -1) != scene_of.get(b, -2):
            raise ValueError(f"contact {i}: rows {a} and {b} must be two rows of one scene")
        if not (0 <= ja < J and 0 <= jb < J):
            raise ValueError(f"contact {i}: joints {ja} and {jb} must lie in [0, {J})")
        end = min(last, int(ln[a]), int(ln[b]))
        for row, joint, share in ((a, ja, meet), (b, jb, 1.0 - meet)):
            if first < end:
                if bool(taken[row, first:end, joint].any()):
                    raise ValueError(f"contact {i} lands on (row {row}, joint {joint}) in frames that carry a static control "
                                     "weight or another contact")
                taken[row, first:end, joint] = True
                w[row, first:end, joint] = cwt if share > 0 else 0.0
        table[i, :6] = (a, ja, b, jb, first, last)
        table[i, 6] = np.float32(meet).view(np.int32)
    place = np.stack([pl[:, 0], pl[:, 1], np.cos(pl[:, 2]), np.sin(pl[:, 2])], 1).astype(np.float32)
    return PartnerTables(partner_rows=torch.from_numpy(prow), bones=torch.tensor(bones, dtype=torch.int32).reshape(nb, 2),
                         placements=torch.from_numpy(place), pose=torch.from_numpy(pl.copy()), contacts=torch.from_numpy(table), weights=w, lengths=ln,
                         radius=radius, margin=margin, weight=weight, Ks=Ks, Km=Ks + Pm * nb, Pm=Pm, nb=nb, B=B, T=T, J=J)


def partner_scratch_floats(B: int, T: int, F: int) -> int:
    """Floats of the scratch ``mdm_partner_tracks`` needs next to the world joints."""
    return int(L.lib().mdm_partner_tracks_scratch_floats(B, T, F))


def partner_launch(x0, lengths, mean_rows, std_rows, tables: PartnerTables, dev_tables, world, scratch, tracks, bounds, targets):
    """One ``mdm_partner_tracks`` call on the current stream: every tensor is the caller's, on the device, float32 (int32
    lengths) and contiguous; ``dev_tables`` = (placements, partner_rows, contacts) of ``tables`` on the device, ``scratch``
    ``partner_scratch_floats`` floats.  Allocation
    free: the sampling runner calls it inside graph capture."""
    t = tables
    place, prow, cont = dev_tables
    B, T, F = x0.shape
    L.check(L.lib().mdm_partner_tracks(
        x0.data_ptr(), lengths.data_ptr(), mean_rows.data_ptr(), std_rows.data_ptr(), place.data_ptr(),
        prow.data_ptr() if t.Pm else 0, t.partner_rows.data_ptr() if t.Pm else 0, t.Pm, t.bones.data_ptr() if t.nb else 0, t.nb,
        t.radius, t.margin, t.weight, t.Ks, t.Km, cont.data_ptr() if len(t.contacts) else 0,
        t.contacts.data_ptr() if len(t.contacts) else 0, len(t.contacts), B, T, F, world.data_ptr(), scratch.data_ptr(),
        L.ptr(tracks), L.ptr(bounds),
        L.ptr(targets), L.stream_ptr()), "mdm_partner_tracks")


@torch.no_grad()
def partner_tracks(x0, lengths, mean, std, tables: PartnerTables, static_tracks=None, return_world=False):
    """The device call of characters sampled together on its own: from ``x0`` (B, T, F) on a GPU, ``mean`` / ``std`` (F,) or
    (B, F) and ``partner_tables``' result, ``(tracks (B, T, Km, REC), track_bounds (B, T, 4), targets (B, T, J, 3))`` as the
    tracks guidance takes them (``tables.weights`` are the targets' weights).  ``static_tracks``: the Ks user tracks as
    ``batch_tracks`` takes them (``tables.Ks`` of them).  ``return_world``: also the world joints (B, T, J, 3)."""
    L.require_cuda(x0)
    dev = x0.device
    x = x0.detach().to(torch.float32).contiguous()
    if x.dim() != 3:
        raise ValueError(f"x0 of shape {tuple(x.shape)} must be (B, T, F)")
    B, T, F = x.shape
    t = tables
    if (B, T, joints_for_feats(F)) != (t.B, t.T, t.J):
        raise ValueError(f"x0 of shape {tuple(x.shape)} does not fit tables made for B = {t.B}, T = {t.T}, J = {t.J}")
    ln = torch.as_tensor(lengths).flatten().to(torch.int32)
    if ln.numel() != B or not bool((ln.cpu() == t.lengths).all()):
        raise ValueError("lengths must be the lengths the tables were made for")
    tracks = torch.zeros((B, T, t.Km, REC), device=dev)
    if t.Ks:
        if static_tracks is None:
            raise ValueError(f"the tables reserve {t.Ks} static tracks: give static_tracks")
        st = batch_tracks(static_tracks, B, T, t.lengths)
        if st.shape[2] != t.Ks:
            raise ValueError(f"static_tracks hold {st.shape[2]} tracks, the tables reserve {t.Ks}")
        tracks[:, :, :t.Ks] = st.to(dev)
    elif static_tracks is not None:
        raise ValueError("static_tracks given, but the tables reserve none (static_tracks=0)")
    bounds = torch.empty((B, T, 4), device=dev)
    targets = torch.zeros((B, T, t.J, 3), device=dev)
    world = torch.empty((B, T, t.J, 3), device=dev)
    scratch = torch.empty(max(partner_scratch_floats(B, T, F), 1), device=dev)
    mean_t = _rows(mean, B, F, "mean").to(dev).contiguous()
    std_t = _rows(std, B, F, "std").to(dev).contiguous()
    dev_tables = tuple(v.to(dev).contiguous() for v in (t.placements, t.partner_rows, t.contacts))
    with torch.cuda.device(dev):
        partner_launch(x, ln.to(dev).contiguous(), mean_t, std_t, t, dev_tables, world, scratch, tracks if t.Km else None,
                       bounds if t.Km else None, targets)
    if not t.Km:
        bounds.fill_(-math.inf)
        bounds[..., :3] = 0.0
    return (tracks, bounds, targets, world) if return_world else (tracks, bounds, targets)


# ---- self-collision avoidance: every joint keeps out of the capsules of the character's own bones ----------
MAX_SELF_JOINTS, MAX_SELF_BONES = 32, 31
SELF_MAX_FRAMES = 64 * 1024 // 20  # mdm_self_max_frames(): the recovery's LDS holds five floats a frame


# Bone lengths as fractions of the body height, along the rest axes of ``motion_features.SKELETONS``: a look, not a measurement,
# like ``motion_mesh.BODY_RADII``.  t2m by joint name (the bone that ends in the joint), KIT by joint index.
_T2M_LENGTHS = {"pelvis": 0.0, "hip": 0.06, "knee": 0.235, "ankle": 0.24, "foot": 0.08, "spine1": 0.07, "spine2": 0.08, "spine3": 0.035,
                "neck": 0.125, "head": 0.06, "collar": 0.075, "shoulder": 0.07, "elbow": 0.155, "wrist": 0.15}
_KIT_LENGTHS = (0.0, 0.08, 0.08, 0.12, 0.12, 0.10, 0.155, 0.15, 0.10, 0.155, 0.15, 0.06, 0.235, 0.24, 0.05, 0.05, 0.06, 0.235, 0.24,
                0.05, 0.05)


def default_offsets(skeleton="t2m", height=1.7) -> np.ndarray:
    """Bone offsets (J, 3) float64 of a plain body of ``height`` (in the data's units: metres in HumanML3D) on the rest axes
    of ``skeleton`` ("t2m" or "kit"): what ``self_body`` and ``motion_mesh.capsule_body`` take when the user brings no
    skeleton of their own.  ValueError for another skeleton and a height that is not finite and > 0."""
    from .motion_features import SKELETONS
    height = _positive(height, "height")
    if skeleton == "t2m":
        from .motion_edit import SMPL_JOINTS
        lengths = [_T2M_LENGTHS[n.split("_")[-1]] for n in SMPL_JOINTS]
    elif skeleton == "kit":
        lengths = list(_KIT_LENGTHS)
    else:
        raise ValueError(f"default_offsets knows the skeletons 't2m' and 'kit', not {skeleton!r}")
    return SKELETONS[skeleton].raw_offsets.astype(np.float64) * (height * np.asarray(lengths))[:, None]


class SelfBody:
    """The body a character keeps out of, made by ``self_body``: ``bones`` (nb, 2) int32 (parent, child), ``bone_radius`` (nb,)
    float32, ``joint_params`` (J, 2) float32 = (r_j, u_j), ``allowed`` (J, nb) bool (bone i acts on joint j), ``pair_mask`` (J,)
    int32 (bit i of entry j = ``allowed[j, i]``), ``margin``, ``J`` and ``nb``.  All on the CPU."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def on(self, device):
        """(bone_radius, joint_params, pair_mask) on ``device``, contiguous: the device tables of the launches."""
        return tuple(v.to(device).contiguous() for v in (self.bone_radius, self.joint_params, self.pair_mask))


def _tree_hops(parents):
    """(J, J) hop counts between the joints of a tree given by its parents."""
    J = len(parents)
    hop = np.full((J, J), J, dtype=np.int64)
    np.fill_diagonal(hop, 0)
    for c, p in enumerate(parents):
        if p >= 0:
            hop[c, p] = hop[p, c] = 1
    for k in range(J):  # Floyd-Warshall: J <= 32
        hop = np.minimum(hop, hop[:, k:k + 1] + hop[k:k + 1, :])
    return hop


def segment_distances(p: torch.Tensor, bones) -> torch.Tensor:
    """The distance of every joint of ``p`` (..., J, 3) to the segment of every bone (u, v) of the same frame: (..., J, nb).  A
    bone without length is its point.  Plain torch ops."""
    bones = torch.as_tensor(bones).reshape(-1, 2).tolist()
    out = []
    for u, v in bones:
        a = p[..., u, :].unsqueeze(-2)
        e, w = p[..., v, :].unsqueeze(-2) - a, p - a
        den = (e * e).sum(-1)
        h = torch.where(den > 0, (w * e).sum(-1) / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(den)).clamp(0, 1)
        out.append((w - h[..., None] * e).norm(dim=-1))
    return torch.stack(out, -1)


def self_body(offsets, skeleton="t2m", radii=None, radius_scale=1.0, joint_radius=None, joint_weights=None, margin=0.02, hops=2,
              pairs=None, rest_joints=False) -> SelfBody:
    """The capsules a character keeps its own joints out of.  ``offsets`` (J, 3): the bone offsets of the skeleton, as
    ``motion_mesh.capsule_body`` takes them, or with ``rest_joints=True`` the joints of its rest pose.  Bone c >= 1 is the segment
    parent(c) -> c (bone index c - 1).  ``radii`` (J,), per bone as ``capsule_body``'s (entry 0, the pelvis sphere, only serves as
    the pelvis joint's default radius), in the offsets' units; default ``motion_mesh.BODY_RADII[skeleton]`` times the height of
    the rest pose; both times ``radius_scale``: the capsules are then those of ``capsule_body``.  ``joint_radius`` (J,): r_j,
    default the radius of joint j's own bone; ``joint_weights`` (J,): u_j, default 1.  ``margin``: m.  Which bone acts on which
    joint: ``pairs`` (J, J - 1) bool, or by default every pair (j, i) whose joint is more than ``hops`` tree edges from both
    ends of bone i and that does not penetrate in the rest pose at this margin (shoulder against neck, hip against the other
    hip).  ValueError for offsets of another shape or not finite, non-finite or non-positive radii or scale, a wrong shape,
    more than 32 joints, a skeleton without listed radii when ``radii`` is None, a non-finite margin and negative ``hops``."""
    from .motion_features import get_skeleton
    from .motion_mesh import BODY_RADII, rest_pose
    sk = get_skeleton(skeleton)
    J = int(sk.joints)
    if J > MAX_SELF_JOINTS:
        raise ValueError(f"a skeleton of {J} joints: self-collision takes at most {MAX_SELF_JOINTS}")
    off = np.asarray(offsets.detach().cpu().numpy() if torch.is_tensor(offsets) else offsets, dtype=np.float64)
    if off.shape != (J, 3) or not np.isfinite(off).all():
        raise ValueError(f"offsets of shape {off.shape} must be finite ({J}, 3)")
    rest = off - off[0] if rest_joints else rest_pose(off, sk)
    radius_scale = _positive(radius_scale, "radius_scale")
    if radii is None:
        name = skeleton if isinstance(skeleton, str) else next((k for k in BODY_RADII if get_skeleton(k) is sk), None)
        if name not in BODY_RADII:
            raise ValueError("radii are required for a skeleton that BODY_RADII does not list")
        radii = np.asarray(BODY_RADII[name], np.float64) * (rest[:, 1].max() - rest[:, 1].min())
    else:
        radii = np.asarray(radii.detach().cpu().numpy() if torch.is_tensor(radii) else radii, dtype=np.float64)
        if radii.shape != (J,):
            raise ValueError(f"radii of shape {radii.shape} must be ({J},)")
    radii = radii * radius_scale
    if not (np.isfinite(radii).all() and (radii > 0).all()):
        raise ValueError(f"radii must be {J} finite positive numbers")
    margin = float(margin)
    if not math.isfinite(margin):
        raise ValueError("margin must be finite")
    parents = [int(p) for p in sk.parents]
    bones = [(parents[c], c) for c in range(1, J)]
    nb = len(bones)
    jp = joint_params(J, radii if joint_radius is None else joint_radius, joint_weights)
    rho = torch.tensor(radii[1:], dtype=torch.float32)
    if pairs is not None:
        allowed = np.asarray(pairs.detach().cpu().numpy() if torch.is_tensor(pairs) else pairs)
        if allowed.shape != (J, nb) or allowed.dtype != np.bool_:
            raise ValueError(f"pairs of shape {allowed.shape} and dtype {allowed.dtype} must be bool ({J}, {nb})")
        allowed = allowed.copy()
    else:
        if isinstance(hops, bool) or int(hops) != hops or int(hops) < 0:
            raise ValueError(f"hops must be an integer >= 0, not {hops!r}")
        hop = _tree_hops(parents)
        ends = np.asarray(bones)
        far = (hop[:, ends[:, 0]] > int(hops)) & (hop[:, ends[:, 1]] > int(hops))  # (J, nb)
        d = segment_distances(torch.from_numpy(rest), bones).numpy()
        clear = margin + jp[:, 0].double().numpy()[:, None] + rho.double().numpy()[None] - d <= 0
        allowed = far & clear
    mask = (allowed.astype(np.int64) << np.arange(nb)[None]).sum(1).astype(np.int32)
    return SelfBody(bones=torch.tensor(bones, dtype=torch.int32).reshape(nb, 2), bone_radius=rho, joint_params=jp,
                    allowed=torch.from_numpy(allowed), pair_mask=torch.from_numpy(mask), margin=margin, J=J, nb=nb)


def _self_joints(joints, lengths, body):
    P = torch.as_tensor(joints)
    if P.dim() != 4 or tuple(P.shape[2:]) != (body.J, 3):
        raise ValueError(f"joints of shape {tuple(P.shape)} must be (B, T, {body.J}, 3)")
    ln = torch.as_tensor(lengths).flatten().to(torch.int32)
    if ln.numel() != P.shape[0]:
        raise ValueError(f"lengths must hold {P.shape[0]} entries")
    return P, ln


@torch.no_grad()
def self_push(joints, lengths, body: SelfBody):
    """``(push (B, T, J, 3), depth (B, T, J))`` of ``joints`` (B, T, J, 3) on a GPU against their own ``body``
    (``mdm_self_push``): push = sum_i pen_i n_i and depth = sum_i pen_i over the allowed bones, zero at and past a length."""
    P, ln = _self_joints(joints, lengths, body)
    L.require_cuda(P)
    dev = P.device
    P = P.detach().to(torch.float32).contiguous()
    B, T = P.shape[:2]
    push, depth = torch.zeros((B, T, body.J, 3), device=dev), torch.zeros((B, T, body.J), device=dev)
    rho, jp, mask = body.on(dev)
    with torch.cuda.device(dev):
        L.check(L.lib().mdm_self_push(P.data_ptr(), ln.to(dev).contiguous().data_ptr(), body.bones.data_ptr(), body.nb, rho.data_ptr(),
                                      jp.data_ptr(), mask.data_ptr(), body.margin, B, T, body.J, push.data_ptr(), depth.data_ptr(),
                                      L.stream_ptr()), "mdm_self_push")
    return push, depth


@torch.no_grad()
def self_penetration(joints, lengths, body: SelfBody):
    """How far a result violates its own body, per sample: ``(depth (B,), share (B,))``.  ``depth``: the deepest penetration
    of one joint's sphere into one allowed bone's capsule in metres, max(0, r_j + rho_i - d_i), the margin not counted;
    ``share``: the share of the sample's valid (t, j) inside some allowed capsule's margin.  Joints of weight 0 are ignored.
    Plain torch ops on the device the joints are on: the check for a result, like ``penetration``."""
    P, ln = _self_joints(joints, lengths, body)
    B, T = P.shape[:2]
    r = body.joint_params[:, 0].to(P.device, P.dtype)
    rho = body.bone_radius.to(P.device, P.dtype)
    on = (body.allowed & (body.joint_params[:, 1] > 0)[:, None]).to(P.device)
    depth, share = P.new_zeros(B), P.new_zeros(B)
    for b in range(B):
        n = min(max(int(ln[b]), 0), T)
        if n == 0:
            continue
        over = r[None, :, None] + rho[None, None] - segment_distances(P[b, :n], body.bones)  # (n, J, nb)
        depth[b] = torch.where(on[None], over.clamp(min=0), torch.zeros_like(over)).max()
        share[b] = (on[None] & (over + body.margin > 0)).any(-1).to(P.dtype).mean()
    return depth, share


def self_scratch_floats(B: int, T: int, F: int) -> int:
    """Floats of the scratch ``mdm_self_targets`` needs."""
    return int(L.lib().mdm_self_targets_scratch_floats(B, T, F))


def self_max_frames() -> int:
    """The longest T ``mdm_self_targets`` takes (the recovery's LDS limit)."""
    return int(L.lib().mdm_self_max_frames())


def self_launch(x0, lengths, mean_rows, std_rows, body: SelfBody, dev_tables, weight, static_targets, static_weights, joints,
                scratch, targets, weights):
    """One ``mdm_self_targets`` call on the current stream: every tensor is the caller's, on the device, float32 (int32 lengths)
    and contiguous; ``dev_tables`` = ``body.on(device)``, ``scratch`` ``self_scratch_floats`` floats, the static pair both or
    None.  Allocation free: the sampling runner calls it inside graph capture."""
    rho, jp, mask = dev_tables
    B, T, F = x0.shape
    L.check(L.lib().mdm_self_targets(
        x0.data_ptr(), lengths.data_ptr(), mean_rows.data_ptr(), std_rows.data_ptr(), body.bones.data_ptr(), body.nb, rho.data_ptr(),
        jp.data_ptr(), mask.data_ptr(), body.margin, float(weight), L.ptr(static_targets), L.ptr(static_weights), B, T, F,
        joints.data_ptr(), scratch.data_ptr(), targets.data_ptr(), weights.data_ptr(), L.stream_ptr()), "mdm_self_targets")


@torch.no_grad()
def self_targets(x0, lengths, mean, std, body: SelfBody, weight, static_targets=None, static_weights=None, return_joints=False):
    """The device call of self-collision avoidance on its own: from ``x0`` (B, T, F) on a GPU and ``mean`` / ``std`` (F,) or
    (B, F), ``(targets, weights)``, both (B, T, J, 3), as the guidance calls take them: P + push under weight * u_j where a
    joint penetrates, weight 0 elsewhere, and the static pair (B, T, J, 3), both or neither, wherever it carries a weight.
    ``return_joints``: also P (B, T, J, 3)."""
    L.require_cuda(x0)
    dev = x0.device
    x = x0.detach().to(torch.float32).contiguous()
    if x.dim() != 3 or joints_for_feats(x.shape[2]) != body.J:
        raise ValueError(f"x0 of shape {tuple(x.shape)} must be (B, T, F) with {body.J} joints")
    B, T, F = x.shape
    ln = torch.as_tensor(lengths).flatten().to(torch.int32)
    if ln.numel() != B:
        raise ValueError(f"lengths must hold {B} entries")
    if (static_targets is None) != (static_weights is None):
        raise ValueError("static_targets and static_weights go together: give both or neither")
    weight = float(weight)
    if not (math.isfinite(weight) and weight >= 0):
        raise ValueError(f"weight must be finite and >= 0, not {weight}")
    if T > self_max_frames():
        raise ValueError(f"T = {T}: self-collision takes at most {self_max_frames()} frames")
    sg = sw = None
    if static_targets is not None:
        sg, sw = (torch.as_tensor(v).detach().to(dev, torch.float32) for v in (static_targets, static_weights))
        if tuple(sg.shape) != (B, T, body.J, 3):
            raise ValueError(f"static_targets of shape {tuple(sg.shape)} must be {(B, T, body.J, 3)}")
        sw = expand_to_static(sw, sg.shape)
        sg = sg.contiguous()
    shape = (B, T, body.J, 3)
    joints, targets, weights = (torch.zeros(shape, device=dev) for _ in range(3))
    scratch = torch.empty(max(self_scratch_floats(B, T, F), 1), device=dev)
    mean_t = _rows(mean, B, F, "mean").to(dev).contiguous()
    std_t = _rows(std, B, F, "std").to(dev).contiguous()
    with torch.cuda.device(dev):
        self_launch(x, ln.to(dev).contiguous(), mean_t, std_t, body, body.on(dev), weight, sg, sw, joints, scratch, targets, weights)
    return (targets, weights, joints) if return_joints else (targets, weights)


def expand_to_static(w, shape):
    """Static target weights aligned on their leading dims to ``shape`` (B, T, J, 3), dense."""
    if w.dim() > 4 or tuple(w.shape) != tuple(shape)[:w.dim()]:
        raise ValueError(f"static_weights of shape {tuple(w.shape)} must lead {tuple(shape)}")
    return w.reshape(tuple(w.shape) + (1,) * (4 - w.dim())).expand(shape).contiguous()

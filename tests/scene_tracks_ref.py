"""Tracks (primitives whose record differs from frame to frame) restated in fp64 torch on top of
tests/scene_ref.py: the reference tests/test_scene_tracks_*.py hold the kernels and the host helpers against.  It reads packed
records (T, Km, 12) and shares no code with the product.

* ``tracks_loss``: L_tracks of a set of positions, ``scene_ref.scene_loss`` applied per frame to that frame's records;
* ``ref_tracks_loss_grad``: L_tracks plus the static scene's and §14's target term over
  ``test_motion_control_host.ref_positions`` and the gradient by autograd, with ``ref_scene_loss_grad``'s conventions;
* ``track_stats``: ``scene_ref.scene_stats`` per frame, reduced over the frames: the least jump distance per track and the
  share of (t, j) each track penalises;
* ``place_tracks``: records that follow the sample's own reference positions, so that they bite, each frame's record shifted
  along X until no penalised joint lies within ``JUMP_CLEAR`` of its jump set.
"""
import math

import torch

import scene_ref as R
from scene_ref import INF, JUMP_CLEAR, _f32
from test_motion_control_host import ref_positions


def tracks_loss(P, tracks, jp):
    """L_tracks of positions P (n, J, 3): sum_t scene_loss(P[t], tracks[t]).  tracks (>= n, Km, 12), jp (J, 2)."""
    loss = P.new_zeros(())
    for t in range(P.shape[0]):
        loss = loss + R.scene_loss(P[t:t + 1], tracks[t], jp)
    return loss


def ref_tracks_loss_grad(x0, lengths, mean, std, tracks, joint_params, scene=None, targets=None, weights=None):
    """fp64 loss (B,) and gradient (B, T, F) of L_tracks + L_scene + sum W (P - G)^2 (the latter two when given) with respect
    to the normalised x0.  mean / std (F,) or (B, F); tracks (B, T, Km, 12); scene (B, K, 12) or None; joint_params (B, J, 2)."""
    x0 = torch.as_tensor(x0).detach().double().cpu()
    B, T, F = x0.shape
    mean = torch.as_tensor(mean).double().cpu().reshape(-1, F).expand(B, F)
    std = torch.as_tensor(std).double().cpu().reshape(-1, F).expand(B, F)
    tracks, joint_params = tracks.double().cpu(), joint_params.double().cpu()
    if targets is not None:
        G = torch.as_tensor(targets).double().cpu()
        W = torch.broadcast_to(torch.as_tensor(weights).double().cpu(), G.shape)
    losses, grads = [], []
    for b in range(B):
        n = max(0, min(int(lengths[b]), T))
        x = x0[b].clone().requires_grad_(True)
        if n == 0:
            losses.append(torch.zeros((), dtype=torch.float64))
            grads.append(torch.zeros(T, F, dtype=torch.float64))
            continue
        P = ref_positions(x[:n], mean[b], std[b])
        loss = tracks_loss(P, tracks[b], joint_params[b])
        if scene is not None:
            loss = loss + R.scene_loss(P, scene[b].double().cpu(), joint_params[b])
        if targets is not None:
            w = W[b, :n]
            d = torch.where(w != 0, P - G[b, :n], torch.zeros_like(P))
            loss = loss + (w * d * d).sum()
        if loss.requires_grad:
            loss.backward()
        losses.append(loss.detach())
        grads.append(torch.zeros(T, F, dtype=torch.float64) if x.grad is None else x.grad.detach().clone())
    return torch.stack(losses), torch.stack(grads)


def track_stats(P, tracks, jp):
    """For positions P (n, J, 3) fp64 and records (>= n, Km, 12): (jump (Km,), share (Km,)).  jump[k]: the smallest jump
    distance over the (t, j) that track k penalises (inf when none); share[k]: the share of the n J pairs (t, j) it penalises."""
    Km = tracks.shape[1]
    jump, share = torch.full((Km,), INF, dtype=torch.float64), torch.zeros(Km, dtype=torch.float64)
    n = P.shape[0]
    for t in range(n):
        j, s = R.scene_stats(P[t:t + 1], tracks[t], jp)
        jump, share = torch.minimum(jump, j), share + s / n
    return jump, share


def _unit(g):
    v = torch.randn(3, generator=g, dtype=torch.float64)
    return v / v.norm()


def place_tracks(P, jp, Km, seed=0, T=None):
    """(T, Km, 12) records, fp32-exact in fp64, that follow the positions P (n, J, 3) of one sample.  With sp the per-axis std
    of P - P[:, :1] (the body's own extent) and s its mean, track k anchors to a seeded joint a_k at a seeded offset o_k of
    length 0.35 s, c = P[t, a_k] + o_k, phi = 0.3 t + k, weight 1 + 0.25 (k % 4), margin 0.02 (k % 3), kinds cycling with k % 5:
      0  a sphere at c of radius s;
      1  a capsule with ends c -+ s (cos phi, 0.5, sin phi) of radius 0.8 s;
      2  a box centred 0.4 sp_x further along X, half extents (0.5 sp_x, 1.5 sp_y, 1.2 sp_z), yaw 0.6 + 0.1 t;
      3  a half-space with normal ~ (0.2 sin phi, 1, 0.1 cos phi), offset n . P[t, 0] - 0.4 sp_y + 0.1 sin phi;
      4  a keep-in box at P[t, 0] + o_k, half extents 1.2 sp, yaw -0.4 + 0.05 t.
    Each frame's record is shifted by 0.01 m along X, at most 20 times, while a penalised joint lies within JUMP_CLEAR of its
    jump set.  Frames at or past n (up to T) repeat the last placed frame's records (a unit sphere without one): the kernels
    must not read them into anything."""
    g = torch.Generator().manual_seed(seed)
    n, J = P.shape[0], P.shape[1]
    T = n if T is None else T
    out = torch.zeros(T, Km, 12, dtype=torch.float64)
    if n:
        rel = (P - P[:, :1]).detach().double().reshape(-1, 3)
        sp = rel.std(0, unbiased=False).clamp(min=0.05)
        s = float(sp.mean())
    for k in range(Km):
        a_k = int(torch.randint(0, J, (1,), generator=g))
        o_k = _unit(g) * 0.35 * (s if n else 1.0)
        wgt, mar = 1.0 + 0.25 * (k % 4), 0.02 * (k % 3)
        for t in range(n):
            c, phi, kind = P[t, a_k].detach().double() + o_k, 0.3 * t + k, k % 5
            if kind == 0:
                q = R._record(R.SPHERE, 1, wgt, mar, c.tolist() + [s])
            elif kind == 1:
                e = s * torch.tensor([math.cos(phi), 0.5, math.sin(phi)], dtype=torch.float64)
                q = R._record(R.CAPSULE, 1, wgt, mar, (c - e).tolist() + (c + e).tolist() + [0.8 * s])
            elif kind == 2:
                cb, yaw = c + torch.tensor([0.4 * float(sp[0]), 0.0, 0.0], dtype=torch.float64), 0.6 + 0.1 * t
                q = R._record(R.BOX, 1, wgt, mar, cb.tolist() + [0.5 * float(sp[0]), 1.5 * float(sp[1]), 1.2 * float(sp[2])]
                              + [math.cos(yaw), math.sin(yaw)])
            elif kind == 3:
                nrm = torch.tensor([0.2 * math.sin(phi), 1.0, 0.1 * math.cos(phi)], dtype=torch.float64)
                nrm = nrm / nrm.norm()
                q = R._record(R.HALF_SPACE, 1, wgt, mar, nrm.tolist() + [float((nrm * P[t, 0].detach().double()).sum())
                                                                        - 0.4 * float(sp[1]) + 0.1 * math.sin(phi)])
            else:
                cb, yaw = P[t, 0].detach().double() + o_k, -0.4 + 0.05 * t
                q = R._record(R.BOX, -1, wgt, mar, cb.tolist() + (1.2 * sp).tolist() + [math.cos(yaw), math.sin(yaw)])
            for _ in range(20):
                jump, _ = R.scene_stats(P[t:t + 1].detach().double(), q[None], jp)
                if float(jump[0]) >= JUMP_CLEAR:
                    break
                for col in ((4, 7) if int(q[0]) == R.CAPSULE else (4,)):
                    q[col] = _f32(q[col] + 0.01)
            out[t, k] = q
        if n == 0:
            out[:, k] = R._record(R.SPHERE, 1, wgt, mar, [0.0, 0.0, 0.0, 1.0])
        else:
            out[n:, k] = out[n - 1, k]
    return out

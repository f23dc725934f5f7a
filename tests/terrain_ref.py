"""Terrain (a height-map ground) restated in fp64 torch on top of tests/scene_ref.py and
tests/scene_tracks_ref.py: the reference tests/test_terrain_*.py hold the kernels and the host helpers against.  It reads a
grid (Gz, Gx) and a record (8,) = origin x, origin z, cos yaw, sin yaw, 1 / cell_x, 1 / cell_z, weight, margin, and shares no
code with the product.

* ``height`` / ``clearance``: h(p), bilinear inside the grid, the nearest edge's height outside; e = p_y - h(p);
* ``terrain_loss``: L_terrain of a set of positions; ``ref_terrain_loss_grad``: L_terrain plus the scene's, the tracks' and
  §14's target term over ``test_motion_control_host.ref_positions`` and the gradient by autograd, with ``ref_loss_grad``'s
  conventions (the grid and S are data);
* ``line_distance``: for the penalised (t, j) the least distance, along the grid's x and along its z, to a grid line (where the
  slope of h jumps) or to the clamp edge, and the share of (t, j) each of the two terms penalises;
* ``place_terrain``: a grid built from the positions' own spread, so that both terms bite, its origin shifted by a fraction of
  a cell until every penalised joint is ``LINE_CLEAR`` away from the lines;
* ``positions_f32``: the reference positions computed in fp32, for the measurement ``LINE_CLEAR`` comes from.

LINE_CLEAR = 20 x POSITION_ERR.  POSITION_ERR is the largest |P_fp32 - P_fp64| over the inputs of tests/test_terrain_gpu.py
((B, T, F) = (1, 2, 263), (1, 2, 251), (3, 40, 263), (3, 40, 251), (2, 196, 263), every sample), measured on the CPU by
``python tests/terrain_ref.py``.
"""
import math

import torch

import scene_ref as R
import scene_tracks_ref as TR
from scene_ref import INF, _f32
from test_motion_control_host import motion_ref, ref_positions

POSITION_ERR = 6.853e-6  # metres, measured at (2, 196, 263); 2.4e-6 at T = 40, 1.7e-7 at T = 2
LINE_CLEAR = 20 * POSITION_ERR  # 1.371e-4 m
SHIFTS = 20  # origin shifts place_terrain may take


def _cells(P, grid, rec):
    """Cell coordinates of points P (..., 3) fp64: raw (ru, rv) and clamped (u, v)."""
    gz, gx = grid.shape
    dx, dz = P[..., 0] - rec[0], P[..., 2] - rec[1]
    ru = (rec[2] * dx - rec[3] * dz) * rec[4]
    rv = (rec[3] * dx + rec[2] * dz) * rec[5]
    return ru, rv, ru.clamp(0, gx - 1), rv.clamp(0, gz - 1)


def height(P, grid, rec):
    """h(p) of points P (..., 3) fp64 over grid (Gz, Gx) fp64 with record rec (8,) fp64; differentiable in P."""
    gz, gx = grid.shape
    _, _, u, v = _cells(P, grid, rec)
    i = u.detach().floor().long().clamp(max=gx - 2)
    k = v.detach().floor().long().clamp(max=gz - 2)
    fu, fv = u - i, v - k
    return ((1 - fv) * ((1 - fu) * grid[k, i] + fu * grid[k, i + 1]) + fv * ((1 - fu) * grid[k + 1, i] + fu * grid[k + 1, i + 1]))


def clearance(P, grid, rec):
    return P[..., 1] - height(P, grid, rec)


def terrain_loss(P, grid, rec, jp, S=None):
    """L_terrain of positions P (n, J, 3): sum_{t, j} u_j a (max(0, m + r_j - e)^2 + S[t, j] max(0, e - r_j - m)^2).
    jp (J, 2) = (radius, weight) per joint; S (>= n, J) or None (all 0)."""
    grid, rec, jp = grid.double(), rec.double(), jp.double()
    d = rec[7] + jp[:, 0] - clearance(P, grid, rec)
    loss = (jp[:, 1] * rec[6] * d.clamp(min=0) ** 2).sum()
    if S is not None:
        loss = loss + (jp[:, 1] * rec[6] * S[:P.shape[0]].double() * (-d).clamp(min=0) ** 2).sum()
    return loss


def ref_terrain_loss_grad(x0, lengths, mean, std, grid, rec, joint_params, stand=None, scene=None, tracks=None, targets=None,
                          weights=None):
    """fp64 loss (B,) and gradient (B, T, F) of L_terrain + L_scene + L_tracks + sum W (P - G)^2 (the latter three when given)
    with respect to the normalised x0.  mean / std (F,) or (B, F); grid (B, Gz, Gx); rec (B, 8); joint_params (B, J, 2); stand
    (B, T, J) or None; scene (B, K, 12) or None; tracks (B, T, Km, 12) or None."""
    x0 = torch.as_tensor(x0).detach().double().cpu()
    B, T, F = x0.shape
    mean = torch.as_tensor(mean).double().cpu().reshape(-1, F).expand(B, F)
    std = torch.as_tensor(std).double().cpu().reshape(-1, F).expand(B, F)
    joint_params = joint_params.double().cpu()
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
        loss = terrain_loss(P, grid[b], rec[b], joint_params[b], None if stand is None else stand[b])
        if scene is not None:
            loss = loss + R.scene_loss(P, scene[b].double().cpu(), joint_params[b])
        if tracks is not None:
            loss = loss + TR.tracks_loss(P, tracks[b].double().cpu(), joint_params[b])
        if targets is not None:
            w = W[b, :n]
            d = torch.where(w != 0, P - G[b, :n], torch.zeros_like(P))
            loss = loss + (w * d * d).sum()
        if loss.requires_grad:
            loss.backward()
        losses.append(loss.detach())
        grads.append(torch.zeros(T, F, dtype=torch.float64) if x.grad is None else x.grad.detach().clone())
    return torch.stack(losses), torch.stack(grads)


def line_distance(P, grid, rec, jp, S=None):
    """For positions P (n, J, 3) fp64: (dx, dz, share_below, share_above).  dx / dz: over the (t, j) either term penalises, the
    least distance in metres along the grid's x / z to where the slope of h jumps: the nearest grid line for a joint over the
    grid, the clamp edge for a joint beside it (inf when nothing is penalised).  share_below / share_above: the share of (t, j)
    the keep-above term and the stand term penalise.  A joint of weight 0 is never penalised, nor is any with a = 0."""
    grid, rec, jp = grid.double(), rec.double(), jp.double()
    if P.numel() == 0:
        return INF, INF, 0.0, 0.0
    P = P.detach().double()
    gz, gx = grid.shape
    d = rec[7] + jp[:, 0] - clearance(P, grid, rec)
    live = (jp[:, 1] * rec[6] > 0)[None].expand(d.shape)
    below = live & (d > 0)
    above = live & (d < 0) & ((S[:P.shape[0]].double() > 0) if S is not None else torch.zeros_like(live))
    hit = below | above
    ru, rv, _, _ = _cells(P, grid, rec)

    def axis(r, g, inv):
        frac = r - r.floor()
        inside = torch.minimum(frac, 1 - frac)
        return torch.where(r < 0, -r, torch.where(r > g - 1, r - (g - 1), inside)) / inv

    ddx, ddz = axis(ru, gx, rec[4]), axis(rv, gz, rec[5])
    if not bool(hit.any()):
        return INF, INF, 0.0, 0.0
    return float(ddx[hit].min()), float(ddz[hit].min()), float(below.double().mean()), float(above.double().mean())


def outside_sides(P, grid, rec):
    """How many joints of P (n, J, 3) lie beside the grid past its low-x, high-x, low-z and high-z edge."""
    gz, gx = grid.shape
    ru, rv, _, _ = _cells(P.detach().double(), grid.double(), rec.double())
    return int((ru < 0).sum()), int((ru > gx - 1).sum()), int((rv < 0).sum()), int((rv > gz - 1).sum())


def place_terrain(P, jp, S, Gx, Gz, cell=None, yaw=0.0, seed=0, corner=False, weight=1.5, margin=0.02):
    """A grid (Gz, Gx) and record (8,), fp32-exact in fp64, placed from the positions P (n, J, 3) of one sample.  The heights
    are the median of P_y plus a seeded smooth wave of amplitude 0.6 std(P_y) plus seeded noise of 0.2 std(P_y), so that
    joints lie under and over the ground.  ``cell`` = (cell_x, cell_z) metres; None: the grid spans 0.8 of the positions'
    spread (2 std) along each axis, so that joints lie beside it on every side.  The grid is centred on the median of P_xz;
    ``corner``: its low corner (True) or its high corner ("high") stands there instead (a grid far larger than the motion:
    joints beside it past two edges, and over its first or its last cells).  The
    origin is then shifted by (0.37, 0.29) of a cell, at most SHIFTS times, while a penalised joint lies within LINE_CLEAR of a
    grid line or a clamp edge along x or z.  Returns (grid, rec, shifts taken); shifts == SHIFTS + 1 when none cleared."""
    g = torch.Generator().manual_seed(seed)
    pts = P.detach().double().reshape(-1, 3) if P.numel() else torch.zeros(1, 3, dtype=torch.float64)
    med = pts.median(0).values
    sp = pts.std(0, unbiased=False).clamp(min=0.1) if pts.shape[0] > 1 else torch.full((3,), 0.5, dtype=torch.float64)
    if cell is None:
        cell = (0.8 * 2 * float(sp[0]) / (Gx - 1), 0.8 * 2 * float(sp[2]) / (Gz - 1))
    cx, cz = float(cell[0]), float(cell[1])
    ii, kk = torch.arange(Gx, dtype=torch.float64), torch.arange(Gz, dtype=torch.float64)
    ph = torch.rand(4, generator=g, dtype=torch.float64) * 2 * math.pi
    wave = 0.6 * torch.sin(ii[None] * cx / float(sp[0]) + ph[0]) * torch.cos(kk[:, None] * cz / float(sp[2]) + ph[1])
    grid = _f32(med[1] + float(sp[1]) * (wave + 0.2 * (torch.rand(Gz, Gx, generator=g, dtype=torch.float64) - 0.5)))
    c, s = math.cos(yaw), math.sin(yaw)
    full = ((Gx - 1) * cx, (Gz - 1) * cz)
    half = full if corner == "high" else (0.0, 0.0) if corner else (0.5 * full[0], 0.5 * full[1])
    # origin = median - R_y(yaw) (half_x, 0, half_z): the grid's centre (or corner) over the median
    ox, oz = float(med[0]) - (c * half[0] + s * half[1]), float(med[2]) - (-s * half[0] + c * half[1])
    rec = None
    for shift in range(SHIFTS + 1):
        lx, lz = 0.37 * shift * cx, 0.29 * shift * cz
        rec = _f32([ox + c * lx + s * lz, oz - s * lx + c * lz, c, s, 1.0 / cx, 1.0 / cz, weight, margin])
        dx, dz, _, _ = line_distance(P, grid, rec, jp, S)
        if min(dx, dz) >= LINE_CLEAR:
            return grid, rec, shift
    return grid, rec, SHIFTS + 1


def positions_f32(x, mean, std):
    """``ref_positions`` in fp32: recover_from_ric(x * std + mean) with every tensor and the default dtype float32."""
    J = (x.shape[-1] + 1) // 12
    return motion_ref.recover_from_ric(x.float() * std.float() + mean.float(), J)


if __name__ == "__main__":  # the measurement POSITION_ERR states
    from test_motion_control_gpu import _stats

    worst = 0.0
    for B, T, F in ((1, 2, 263), (1, 2, 251), (3, 40, 263), (3, 40, 251), (2, 196, 263)):
        gen = torch.Generator().manual_seed(B * 1000 + T + F)  # the draws of test_motion_scene_gpu._case
        x0 = torch.randn(B, T, F, generator=gen) * 0.7
        mean, std = _stats(F, B, B + T)
        err = max(float((positions_f32(x0[b], mean[b], std[b]).double() - ref_positions(x0[b], mean[b], std[b])).abs().max())
                  for b in range(B))
        print(f"(B, T, F) = ({B}, {T}, {F}): largest |P_fp32 - P_fp64| = {err:.3e} m")
        worst = max(worst, err)
    print(f"POSITION_ERR (largest) = {worst:.3e} m; LINE_CLEAR = 20 x = {20 * worst:.3e} m")

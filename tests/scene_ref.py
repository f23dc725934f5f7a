"""Scene constraints restated in fp64 torch: the reference tests/test_motion_scene_*.py hold the kernels and
the host helpers against.  It reads packed primitive records (K, 12) = kind, sigma, weight, margin, eight parameters (a box:
centre, half extents, cos yaw, sin yaw) and shares no code with the product.

* ``distances``: the four signed distances; ``scene_loss``: L_scene of a set of positions;
* ``ref_scene_loss_grad``: L_scene (plus §14's target term) over ``test_motion_control_host.ref_positions`` and its gradient
  by autograd, with ``ref_loss_grad``'s conventions;
* ``scene_stats``: for a set of positions the distance of every penalised (t, j, k) to that primitive's jump set (where the
  gradient of d jumps), and the share of (t, j) each primitive penalises;
* ``place_scene``: primitives placed from the positions of a sample (one of each kind plus one keep-in box, cycled for more),
  shifted along X until no penalised joint lies within ``JUMP_CLEAR`` of a jump set.
"""
import torch

from test_motion_control_host import ref_positions

PAD, SPHERE, CAPSULE, BOX, HALF_SPACE = 0, 1, 2, 3, 4
JUMP_CLEAR = 1e-3  # metres: about 20 x the fp32 position error at the extents of the test motions
INF = float("inf")


def _box_q(p, q):
    c, s = q[10], q[11]
    dx, dz = p[..., 0] - q[4], p[..., 2] - q[6]
    loc = torch.stack([c * dx - s * dz, p[..., 1] - q[5], s * dx + c * dz], -1)
    return loc, loc.abs() - q[7:10]


def distance(p, q):
    """d(p) of points p (..., 3) fp64 to the primitive of record q (12,) fp64."""
    kind = int(q[0])
    if kind == SPHERE:
        return ((p - q[4:7]) ** 2).sum(-1).sqrt() - q[7]
    if kind == CAPSULE:
        e, v = q[7:10] - q[4:7], p - q[4:7]
        den = float((e * e).sum())
        h = ((v * e).sum(-1) / den).clamp(0, 1) if den > 0 else torch.zeros_like(v[..., 0])
        return ((v - h[..., None] * e) ** 2).sum(-1).sqrt() - q[10]
    if kind == BOX:
        _, qq = _box_q(p, q)
        return (qq.clamp(min=0) ** 2).sum(-1).sqrt() + qq.max(-1).values.clamp(max=0)
    if kind == HALF_SPACE:
        return (p * q[4:7]).sum(-1) - q[7]
    raise ValueError(f"kind {kind}")


def scene_loss(P, rec, jp):
    """L_scene of positions P (n, J, 3): sum_{t, j} u_j sum_k a_k max(0, m_k + r_j - sigma_k d_k(P[t, j]))^2.  rec (K, 12),
    jp (J, 2) = (radius, weight) per joint; padding records are skipped."""
    rec, jp = rec.double(), jp.double()
    loss = P.new_zeros(())
    for q in rec:
        if int(q[0]) == PAD:
            continue
        v = (q[3] + jp[:, 0] - q[1] * distance(P, q)).clamp(min=0)
        loss = loss + (jp[:, 1] * q[2] * v * v).sum()
    return loss


def ref_scene_loss_grad(x0, lengths, mean, std, scene, joint_params, targets=None, weights=None):
    """fp64 loss (B,) and gradient (B, T, F) of L_scene + sum W (P - G)^2 (the latter with targets) with respect to the
    normalised x0.  mean / std (F,) or (B, F); scene (B, K, 12); joint_params (B, J, 2)."""
    x0 = torch.as_tensor(x0).detach().double().cpu()
    B, T, F = x0.shape
    mean = torch.as_tensor(mean).double().cpu().reshape(-1, F).expand(B, F)
    std = torch.as_tensor(std).double().cpu().reshape(-1, F).expand(B, F)
    scene, joint_params = scene.double().cpu(), joint_params.double().cpu()
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
        loss = scene_loss(P, scene[b], joint_params[b])
        if targets is not None:
            w = W[b, :n]
            d = torch.where(w != 0, P - G[b, :n], torch.zeros_like(P))
            loss = loss + (w * d * d).sum()
        if loss.requires_grad:
            loss.backward()
        losses.append(loss.detach())
        grads.append(torch.zeros(T, F, dtype=torch.float64) if x.grad is None else x.grad.detach().clone())
    return torch.stack(losses), torch.stack(grads)


def jump_distance(p, q):
    """A lower bound, exact in the generic case, of the distance of points p (..., 3) to the set where the gradient of the
    primitive's d jumps: a sphere's centre, a capsule's axis (the segment), nowhere for a half-space.  A box's d is C1
    outside the box; inside, its gradient jumps where the two largest of q = |local p| - h tie (every q_a - q_b is
    sqrt(2)-Lipschitz and a path to a tie of two others crosses a tie with the largest, so (q1 - q2) / sqrt(2) bounds the
    distance) and on the mid-plane of the axis of the largest q (distance |local p| there); a point outside is at least d
    away from either as well."""
    kind = int(q[0])
    if kind == SPHERE:
        return ((p - q[4:7]) ** 2).sum(-1).sqrt()
    if kind == CAPSULE:
        return distance(p, q) + q[10]
    if kind == HALF_SPACE:
        return torch.full(p.shape[:-1], INF, dtype=p.dtype)
    loc, qq = _box_q(p, q)
    top = qq.sort(-1, descending=True)
    inside = torch.minimum((top.values[..., 0] - top.values[..., 1]) / 2 ** 0.5,
                           loc.abs().gather(-1, top.indices[..., :1])[..., 0])
    return torch.maximum(inside, distance(p, q).clamp(min=0))


def scene_stats(P, rec, jp):
    """For positions P (n, J, 3) fp64: (jump (K,), share (K,)).  jump[k]: the smallest jump distance over the (t, j) that
    primitive k penalises (inf when it penalises none); share[k]: the share of (t, j) it penalises.  A joint of weight 0
    is never penalised."""
    rec, jp = rec.double(), jp.double()
    K = rec.shape[0]
    jump, share = torch.full((K,), INF, dtype=torch.float64), torch.zeros(K, dtype=torch.float64)
    if P.numel() == 0:
        return jump, share
    for k, q in enumerate(rec):
        if int(q[0]) == PAD or float(q[2]) == 0:
            continue
        hit = ((q[3] + jp[:, 0] - q[1] * distance(P, q)) > 0) & (jp[:, 1] > 0)
        share[k] = hit.double().mean()
        if bool(hit.any()):
            jump[k] = jump_distance(P, q)[hit].min()
    return jump, share


def _f32(v):
    return torch.as_tensor(v, dtype=torch.float64).float().double()


def _record(kind, sigma, weight, margin, params):
    return _f32([kind, sigma, weight, margin] + list(params) + [0.0] * (8 - len(params)))


def place_scene(P, jp, K=5, seed=0):
    """K primitive records (K, 12), fp32-exact in fp64, placed from the positions P (n, J, 3) of one sample at their median
    +- a fraction of their spread: a sphere, a capsule, a yawed box, a half-space and a keep-in box, in that order and
    cycled (with seeded offsets) for K > 5.  A primitive with a penalised joint within JUMP_CLEAR of its jump set is shifted by
    0.01 m along X, at most 20 times."""
    g = torch.Generator().manual_seed(seed)
    pts = P.detach().double().reshape(-1, 3) if P.numel() else torch.zeros(1, 3, dtype=torch.float64)
    med = pts.median(0).values
    sp = pts.std(0, unbiased=False).clamp(min=0.1) if pts.shape[0] > 1 else torch.full((3,), 0.5, dtype=torch.float64)
    out = []
    for k in range(K):
        j = (torch.rand(3, generator=g, dtype=torch.float64) - 0.5) * (0.0 if k < 5 else 0.6)  # offsets of the later rounds
        wgt, mar = 1.0 + 0.25 * (k % 4), 0.02 * (k % 3)
        kind = k % 5
        if kind == 0:
            c = med + sp * (torch.tensor([0.5, 0.2, -0.3]) + j)
            q = _record(SPHERE, 1, wgt, mar, c.tolist() + [1.2 * float(sp.mean())])
        elif kind == 1:
            a = med + sp * (torch.tensor([-0.7, -1.5, 0.3]) + j)
            b = a + sp * torch.tensor([0.1, 3.0, 0.0])
            q = _record(CAPSULE, 1, wgt, mar, a.tolist() + b.tolist() + [0.9 * float(sp[0])])
        elif kind == 2:
            c = med + sp * (torch.tensor([0.2, -0.5, -0.6]) + j)
            yaw = 0.6 + float(j[0])
            # a wall, thinnest along its own X whatever the spreads (a long walk spreads far more in X and Z than in Y): the
            # mid-plane of the thinnest axis belongs to the jump set, and only a shift along X moves this one
            hx = 0.4 * float(sp[0])
            q = _record(BOX, 1, wgt, mar, c.tolist() + [hx, max(1.5 * float(sp[1]), 1.2 * hx), max(1.2 * float(sp[2]), 1.2 * hx)]
                        + [float(torch.cos(torch.tensor(yaw))), float(torch.sin(torch.tensor(yaw)))])
        elif kind == 3:
            nrm = torch.tensor([0.2, 1.0, 0.1], dtype=torch.float64) + 0.3 * j
            nrm = nrm / nrm.norm()
            q = _record(HALF_SPACE, 1, wgt, mar, nrm.tolist() + [float((nrm * med).sum() - 0.4 * sp[1])])
        else:
            c = med + sp * 0.3 * j
            yaw = -0.4 + float(j[1])
            q = _record(BOX, -1, wgt, mar, c.tolist() + (sp * 1.2).tolist()
                        + [float(torch.cos(torch.tensor(yaw))), float(torch.sin(torch.tensor(yaw)))])
        for _ in range(20):
            jump, _ = scene_stats(P, q[None], jp)
            if float(jump[0]) >= JUMP_CLEAR:
                break
            for col in ((4, 7) if int(q[0]) == CAPSULE else (4,)):
                q[col] = _f32(q[col] + 0.01)
        out.append(q)
    return torch.stack(out) if out else torch.zeros(0, 12, dtype=torch.float64)

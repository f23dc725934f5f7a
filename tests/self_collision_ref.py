"""fp64 restatement of self-collision avoidance, for tests/test_self_collision_host.py and
tests/test_self_collision_gpu.py: the distance of every joint to every bone's segment, the push and the depth, the mask rule,
the merge into targets and weights, L_self with the segment ends detached, the x0 hook of ``sampler_ref.loop_ref`` and the
placement of the kernel cases (poses made from a skeleton's rest offsets, perturbed and with limbs folded towards the trunk,
so that joints really sit inside capsules)."""
import functools

import numpy as np
import torch

from conftest import pkg
from test_motion_control_host import ref_positions


# ---- the definition --------------------------------------------------------------------------------------------------------
def segment(P, bones):
    """For joints P (..., J, 3) fp64 and bones [(u, v)]: d (..., J, nb), the distance of every joint to every bone's segment of
    the same frame, and n (..., J, nb, 3) = (P - c) / d with c the closest point, 0 where d < 1e-12.  The segment ends are
    data: they are detached, so that autograd sees the gradient with the bones held fixed."""
    ends = P.detach()
    ds, ns = [], []
    for u, v in bones:
        a = ends[..., u, :].unsqueeze(-2)
        e = ends[..., v, :].unsqueeze(-2) - a
        w = P - a
        ee = (e * e).sum(-1)
        h = torch.where(ee > 0, (w * e).sum(-1) / torch.where(ee > 0, ee, torch.ones_like(ee)), torch.zeros_like(ee)).clamp(0, 1)
        r = w - h.detach()[..., None] * e
        rr = (r * r).sum(-1)
        d = torch.where(rr > 0, torch.where(rr > 0, rr, torch.ones_like(rr)).sqrt(), torch.zeros_like(rr))  # no 0 * inf in autograd
        ds.append(d)
        ns.append(torch.where((d >= 1e-12)[..., None], r / d.clamp(min=1e-300)[..., None], torch.zeros_like(r)))
    return torch.stack(ds, -1), torch.stack(ns, -2)


def _tables(body):
    return ([tuple(b) for b in body.bones.tolist()], body.bone_radius.double(), body.joint_params.double(), body.allowed)


def pens(P, body):
    """pen (..., J, nb) = max(0, m + r_j + rho_i - d_i) over the allowed pairs (0 elsewhere), d and n of ``segment``."""
    bones, rho, jp, allowed = _tables(body)
    d, n = segment(P, bones)
    raw = body.margin + jp[:, 0][:, None] + rho[None] - d
    return torch.where(allowed, raw.clamp(min=0), torch.zeros_like(raw)), d, n, raw


def push_depth(P, lens, body):
    """push (B, T, J, 3) = sum_i pen_i n_i and depth (B, T, J) = sum_i pen_i in fp64, zero at and past a length."""
    P = torch.as_tensor(P).double()
    pen, _, n, _ = pens(P, body)
    live = (torch.arange(P.shape[1])[None] < torch.as_tensor(lens).reshape(-1, 1))[..., None]
    return (pen[..., None] * n).sum(-2) * live[..., None], pen.sum(-1) * live


def merge(P, push, depth, lens, body, weight, static_targets=None, static_weights=None):
    """targets and weights (B, T, J, 3): the static pair wherever one of its three weights is not zero and in every frame at or
    past the length (zeros without one), elsewhere P + push under weight u_j where depth > 0 and under 0 where not."""
    P = torch.as_tensor(P).double()
    u = body.joint_params[:, 1].double()
    tg = P + push
    w = (torch.where(depth > 0, weight * u[None, None], torch.zeros_like(depth)))[..., None].expand_as(tg).clone()
    live = (torch.arange(P.shape[1])[None] < torch.as_tensor(lens).reshape(-1, 1))[..., None, None]
    if static_targets is None:
        return tg * live, w * live
    sg, sw = static_targets.double(), static_weights.double()
    user = (sw != 0).any(-1, keepdim=True) | ~live
    return torch.where(user, sg, tg), torch.where(user, sw, w)


def l_self(P, body, weight):
    """L_self of the valid frames P (n, J, 3): a sum_{t, j} u_j sum_i pen_i^2, the segment ends detached."""
    pen = pens(P, body)[0]
    return weight * (body.joint_params[:, 1].double()[None, :, None] * pen * pen).sum()


def ref_mask(parents, rest, radii, joint_radius, margin, hops):
    """The default mask, restated: pair (j, i) of joint j and bone i = (parent(i + 1), i + 1) is allowed iff j is more than
    ``hops`` tree edges from both ends and m + r_j + rho_i - d_i <= 0 in the rest pose."""
    J = len(parents)
    nbr = [[] for _ in range(J)]
    for c, p in enumerate(parents):
        if p >= 0:
            nbr[c].append(p), nbr[p].append(c)
    hop = np.full((J, J), 10 ** 6)
    for s in range(J):  # breadth first
        hop[s, s], todo = 0, [s]
        while todo:
            a = todo.pop(0)
            for b in nbr[a]:
                if hop[s, b] > hop[s, a] + 1:
                    hop[s, b] = hop[s, a] + 1
                    todo.append(b)
    bones = [(parents[c], c) for c in range(1, J)]
    d = segment(torch.as_tensor(rest).double(), bones)[0].numpy()
    out = np.zeros((J, J - 1), dtype=bool)
    for j in range(J):
        for i, (u, v) in enumerate(bones):
            out[j, i] = hop[j, u] > hops and hop[j, v] > hops and margin + joint_radius[j] + radii[i + 1] - d[j, i] <= 0
    return out


def stats(P, lens, body):
    """Per sample of P (B, T, J, 3): (share of the valid (t, j) that penetrate some allowed capsule, the least distance of a
    penetrating pair to its bone's axis, the least |m + r_j + rho_i - d_i| over the allowed pairs: the distance to pen = 0)."""
    P = torch.as_tensor(P).double()
    out = []
    for b in range(P.shape[0]):
        n = int(lens[b])
        pen, d, _, raw = pens(P[b, :n], body)
        on = body.allowed[None].expand_as(pen)
        out.append((float((pen > 0).any(-1).double().mean()), float(d[pen > 0].min()) if bool((pen > 0).any()) else float("inf"),
                    float(raw[on].abs().min())))
    return out


# ---- placement: real poses, perturbed and folded ---------------------------------------------------------------------------
def _rodrigues(axis, angle):
    a = axis / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def _pose(sk, off, rs, spread, fold):
    """One frame: forward kinematics of the offsets under seeded joint rotations, small everywhere (``spread`` radians) and
    large, towards or through the trunk, at the limbs' second and third joints with probability ``fold``."""
    J = sk.joints
    G = [np.eye(3)] * J
    P = np.zeros((J, 3))
    limb = {c[k] for n, c in enumerate(sk.chains) if n != 2 for k in (1, 2, 3) if k < len(c)}  # chain 2 is the spine
    for chain in sk.chains:
        for a, b in zip(chain[:-1], chain[1:]):
            R = _rodrigues(rs.randn(3), spread * rs.randn())
            if b in limb and rs.rand() < fold:
                R = _rodrigues(rs.randn(3), rs.uniform(-2.6, 2.6)) @ R
            G[b] = G[a] @ R
            P[b] = P[a] + G[b] @ off[b]
    return P


def poses(skeleton, body, B, T, seed, spread=0.25, fold=0.8, clear=1.2e-3):
    """(B, T, J, 3) fp64 poses of ``skeleton``'s default offsets, the root at height 1 over the origin.  A frame is drawn
    again until every allowed pair of it lies at least ``clear`` from pen = 0 and every penetrating pair at least ``clear``
    from its bone's axis: the kernel tests compare an fp32 kernel with fp64 away from where the push jumps."""
    MS, MF = pkg("motion_scene"), pkg("motion_features")
    sk = MF.get_skeleton(skeleton)
    off = MS.default_offsets(skeleton)
    rs = np.random.RandomState(seed)
    out = np.zeros((B, T, sk.joints, 3))
    for b in range(B):
        for t in range(T):
            for _ in range(200):
                P = torch.from_numpy(_pose(sk, off, rs, spread, fold))
                pen, d, _, raw = pens(P, body)
                if float(raw[body.allowed].abs().min()) >= clear and (not bool((pen > 0).any()) or float(d[pen > 0].min()) >= clear):
                    break
            else:
                raise AssertionError("no well-conditioned frame in 200 draws")
            out[b, t] = P.numpy() + np.array([0.0, 1.0, 0.0])
    return torch.from_numpy(out)


def rows_of(P, mean, std, seed):
    """Normalised fp32 feature rows (B, T, F) whose ``recover_from_ric(x0 * std + mean)`` is the poses P (B, T, J, 3) moved
    rigidly, frame by frame, along a seeded root path: zero-heading rows (root height in column 3, the joints in the ric
    columns) with seeded heading and root velocities in columns 0 - 2 and noise in the columns that do not steer."""
    B, T, J, _ = P.shape
    F = mean.shape[-1]
    g = torch.Generator().manual_seed(seed)
    rows = torch.randn(B, T, F, generator=g, dtype=torch.float64) * 0.3
    rows[..., 0] = torch.randn(B, T, generator=g, dtype=torch.float64) * 0.02
    rows[..., 1:3] = torch.randn(B, T, 2, generator=g, dtype=torch.float64) * 0.03
    rows[..., 3] = P[:, :, 0, 1]
    rows[..., 4:4 + 3 * (J - 1)] = P[:, :, 1:].reshape(B, T, -1)
    return ((rows - mean.double()[:, None]) / std.double()[:, None]).float()


def ref_joints(x0, lens, mean, std):
    """P (B, T, J, 3) fp64 = recover_from_ric(x0 * std + mean) of every row's valid frames, zero past them."""
    x0 = torch.as_tensor(x0).detach().double().cpu()
    B, T, F = x0.shape
    out = torch.zeros(B, T, (F + 1) // 12, 3, dtype=torch.float64)
    for b in range(B):
        n = max(0, min(int(lens[b]), T))
        if n:
            out[b, :n] = ref_positions(x0[b, :n], torch.as_tensor(mean)[b], torch.as_tensor(std)[b]).detach()
    return out


# ---- the cases of the kernel tests: shared by the host and the GPU file, left unchanged ------------------------------------
LENGTHS = {(1, 2): (2,), (3, 40): (40, 28, 17), (2, 196): (196, 150)}
CASES = [(B, T, F) for (B, T) in LENGTHS for F in (263, 251)]
SKELETON = {263: "t2m", 251: "kit"}
RADIUS_SCALE = {263: 1.3, 251: 1.8}
WEIGHT = 5.0


def _stats(F, B, seed):
    """mean / std (B, F) as tests/test_motion_control_gpu.py draws them."""
    g = torch.Generator().manual_seed(seed)
    mean = torch.randn(B, F, generator=g) * 0.2
    std = torch.rand(B, F, generator=g) + 0.5
    std[:, 0] *= 0.1
    mean[:, 0] *= 0.1
    return mean, std


@functools.lru_cache(maxsize=None)
def body_of(F, radius_scale=None):
    MS = pkg("motion_scene")
    name = SKELETON[F]
    return MS.self_body(MS.default_offsets(name), name, radius_scale=RADIUS_SCALE[F] if radius_scale is None else radius_scale)


@functools.lru_cache(maxsize=None)
def case(B, T, F):
    """Poses, the rows that give them, statistics, lengths, the body, static targets (one on a penetrating joint of every
    sample, some elsewhere) and the fp64 reference: P from the fp32 rows, push, depth, targets and weights."""
    body = body_of(F)
    lens = torch.tensor(LENGTHS[(B, T)])
    mean, std = _stats(F, B, B + T)
    pose = poses(SKELETON[F], body, B, T, seed=B * 1000 + T + F)
    x0 = rows_of(pose, mean, std, seed=T + F)
    P = ref_joints(x0, lens, mean, std)
    push, depth = push_depth(P, lens, body)
    sg, sw = torch.zeros(B, T, body.J, 3), torch.zeros(B, T, body.J, 3)
    g = torch.Generator().manual_seed(F + T)
    for b in range(B):
        hit = torch.nonzero(depth[b] > 0)
        t, j = hit[len(hit) // 2].tolist()  # a penetrating (t, j): the user's target wins there
        sg[b, t, j], sw[b, t, j] = torch.randn(3, generator=g), torch.tensor([1.5, 0.0, 0.25])
        sg[b, :, 0], sw[b, :, 0, 0], sw[b, :, 0, 2] = torch.randn(T, 3, generator=g), 1.0, 1.0  # a root path, past the length too
    tg, w = merge(P, push, depth, lens, body, WEIGHT)
    tgs, ws = merge(P, push, depth, lens, body, WEIGHT, sg, sw)
    return dict(x0=x0, mean=mean, std=std, lens=lens, body=body, pose=pose, P=P, push=push, depth=depth, static=(sg, sw),
                targets=tg, weights=w, targets_static=tgs, weights_static=ws, J=body.J)


# ---- the restated x0 hook of tests/sampler_ref.loop_ref --------------------------------------------------------------------
def guidance_hook(lengths, ctl, body, weight, mask=None, seen=None):
    """``x0_hook`` of ``sampler_ref.loop_ref``: from every row's x0 (after clipping and the edit blend) this step's targets and
    weights, merged with the static ``control_joints`` / ``control_weights`` of ``ctl`` and held fixed, then ``control_iters``
    autograd steps down the target term (plus L_scene with a ``control_scene``).  ``seen`` collects per call and row (share of
    (t, j) penalised, least distance of a penalised pair to its bone's axis)."""
    import scene_ref as R
    from test_motion_control_host import ref_loss_grad
    one_minus_m = 1.0 if mask is None else 1.0 - mask.double()
    sg, sw = ctl.get("control_joints"), ctl.get("control_weights")

    def hook(x0):
        P = ref_joints(x0, lengths, ctl["control_mean"], ctl["control_std"])
        push, depth = push_depth(P, lengths, body)
        tg, w = merge(P, push, depth, lengths, body, weight, sg, None if sw is None else torch.broadcast_to(sw, sg.shape))
        if seen is not None:
            seen.extend((s, d) for s, d, _ in stats(P, lengths, body))
        for _ in range(ctl["control_iters"]):
            if ctl.get("control_scene") is not None:
                _, gr = R.ref_scene_loss_grad(x0, lengths, ctl["control_mean"], ctl["control_std"], ctl["control_scene"],
                                              ctl["control_joint_params"], tg, w)
            else:
                _, gr = ref_loss_grad(x0, lengths, ctl["control_mean"], ctl["control_std"], tg, w)
            x0 = x0 - ctl["control_scale"] * one_minus_m * gr
        return x0

    return hook

"""fp64 restatement of characters sampled together, for tests/test_partners_host.py and
tests/test_partners_gpu.py: the world joints W_b = to_world(recover_from_ric(x0[b] * std + mean)), the capsule record of every
bone of every partner in a row's own frame, the meeting points of the contacts and the targets they give, all from one x0 of
the whole batch, so that nothing depends on an order among the rows."""
import torch

from conftest import pkg
from test_motion_control_host import ref_positions

CAPSULE = 2


def world_joints(x0, lens, mean, std, pose):
    """W_b (n_b, J, 3) fp64 per row: ``ref_positions`` of the row's first n_b frames, then ``motion_scene.to_world`` at the
    row's ``pose`` = (x, z, yaw)."""
    MS = pkg("motion_scene")
    x0 = torch.as_tensor(x0).detach().double().cpu()
    B, T, F = x0.shape
    J = (F + 1) // 12
    out = []
    for b in range(B):
        n = max(0, min(int(lens[b]), T))
        if n == 0:
            out.append(torch.zeros(0, J, 3, dtype=torch.float64))
            continue
        P = ref_positions(x0[b, :n], torch.as_tensor(mean)[b], torch.as_tensor(std)[b]).detach()
        out.append(MS.to_world(P, pose[b, :2].tolist(), float(pose[b, 2])))
    return out


def local_of(W, pose_b):
    return pkg("motion_scene").to_local(W, pose_b[:2].tolist(), float(pose_b[2]))


def partner_records(W, lens, tables, static=None):
    """The (B, T, Km, 12) fp64 records: ``static`` (B, T, Ks, 12) in front, then per slot and bone the keep-out capsule with
    ends L_b(W_p[t, u]), L_b(W_p[t, v]) for t < min(n_b, n_p), twelve zeros elsewhere."""
    t = tables
    rec = torch.zeros(t.B, t.T, t.Km, 12, dtype=torch.float64)
    if t.Ks:
        rec[:, :, :t.Ks] = torch.as_tensor(static).double()
    for b in range(t.B):
        for q in range(t.Pm):
            p = int(t.partner_rows[b, q])
            n = min(int(lens[b]), int(lens[p])) if p >= 0 else 0
            if n <= 0:
                continue
            Lp = local_of(W[p][:n], t.pose[b])
            for i, (u, v) in enumerate(t.bones.tolist()):
                r = rec[b, :n, t.Ks + q * t.nb + i]
                r[:, 0], r[:, 1], r[:, 2], r[:, 3] = CAPSULE, 1.0, t.weight, t.margin
                r[:, 4:7], r[:, 7:10], r[:, 10] = Lp[:, u], Lp[:, v], t.radius
    return rec


def meeting_points(W, lens, contact):
    """(frames, m): the frames first <= t < min(last, n_a, n_b) of one contact and its meeting points (len(frames), 3) in the
    world."""
    a, ja, b, jb, first, last, _, meet = contact
    end = min(last, int(lens[a]), int(lens[b]))
    fr = list(range(first, max(first, end)))
    if not fr:
        return fr, torch.zeros(0, 3, dtype=torch.float64)
    wa, wb = W[a][fr, ja], W[b][fr, jb]
    return fr, wa + meet * (wb - wa)


def contact_targets(W, lens, tables, contacts):
    """targets (B, T, J, 3) fp64 (zero where no contact lands) and the bool (B, T, J) map of the entries the contacts write."""
    t = tables
    tg = torch.zeros(t.B, t.T, t.J, 3, dtype=torch.float64)
    hit = torch.zeros(t.B, t.T, t.J, dtype=torch.bool)
    for c in contacts:
        fr, m = meeting_points(W, lens, c)
        if fr:
            for row, joint in ((c[0], c[1]), (c[2], c[3])):
                tg[row, fr, joint] = local_of(m, t.pose[row])
                hit[row, fr, joint] = True
    return tg, hit


def ref_partner(x0, lens, mean, std, tables, contacts=(), static=None):
    """(world joints per row, records, targets, hit) of one x0 of the whole batch."""
    W = world_joints(x0, lens, mean, std, tables.pose)
    tg, hit = contact_targets(W, lens, tables, contacts)
    return W, partner_records(W, lens, tables, static), tg, hit


def near_share(P_b, rec_b, n, reach):
    """The share of row b's (t, j), t < n, that lie within ``reach`` of some partner capsule's surface: the placement check."""
    MS = pkg("motion_scene")
    if n == 0:
        return 0.0
    d = MS.track_distances(P_b[:n], rec_b[:n])  # (n, J, Km), 0 for padding
    live = (rec_b[:n, :, 0] != 0)[:, None]
    return float(((d < reach) & live).any(-1).double().mean())


# ---- the cases of the kernel tests: shared by the host and the GPU file, left unchanged ----------------------------------
import functools  # noqa: E402

LENGTHS = {(3, 2): (2, 2, 1), (4, 40): (40, 28, 40, 17), (2, 196): (196, 150)}
RADIUS, MARGIN, WEIGHT = 0.3, 0.05, 5.0
CASES = [(B, T, F, layout, Ks) for (B, T) in ((3, 2), (4, 40)) for F in (263, 251) for layout in ("pairs", "trio")
         for Ks in (0, 3)] + [(2, 196, 263, "pairs", 3)]


def _stats(F, B, seed):
    """mean / std (B, F) as tests/test_motion_control_gpu.py draws them."""
    g = torch.Generator().manual_seed(seed)
    mean = torch.randn(B, F, generator=g) * 0.2
    std = torch.rand(B, F, generator=g) + 0.5
    std[:, 0] *= 0.1
    mean[:, 0] *= 0.1
    return mean, std


def static_tracks(T):
    """Three user tracks in a character's own frame: a ball, a bar and a rising floor (a half-space: the frame's ball is +inf
    while it is live; it is absent in the last frame)."""
    MS = pkg("motion_scene")
    t = torch.arange(T, dtype=torch.float64)
    c = torch.stack([0.5 + 0.01 * t, torch.ones_like(t), 0.2 - 0.01 * t], 1)
    active = torch.ones(T, dtype=torch.bool).numpy()
    active[-1] = False
    return [MS.moving_sphere(c, 0.3, margin=0.05, weight=2.0),
            MS.moving_capsule(c + torch.tensor([1.0, -1.0, 0.0]), c + torch.tensor([1.0, 1.0, 0.5]), 0.2, margin=0.1),
            MS.moving_half_space((0.0, 1.0, 0.0), -2.0 + 0.001 * t, active=active)]


@functools.lru_cache(maxsize=None)
def case(B, T, F, layout, Ks):
    """x0, statistics, lengths, poses that overlap the bodies, the tables, the contacts and the fp64 reference.  "pairs": rows
    (0, 1) and (2, 3) are scenes of two (a last odd row is alone); "trio": rows (0, 1, 2) are one scene and every partner is a
    bone subset, so that Km reaches 24 with Ks = 0."""
    MS = pkg("motion_scene")
    J = (F + 1) // 12
    gen = torch.Generator().manual_seed(B * 1000 + T + F)
    x0 = torch.randn(B, T, F, generator=gen) * 0.7
    mean, std = _stats(F, B, B + T)
    mean[:, 1:3] *= 0.1  # slow roots: the seeded "bodies", clouds of joints some metres across, stay on top of each other
    std[:, 1:3] *= 0.1
    lens = torch.tensor(LENGTHS[(B, T)])
    pose = torch.tensor([[0.25 * b, -0.15 * b, 0.7 * b] for b in range(B)], dtype=torch.float64)
    if layout == "pairs":
        scenes = [list(range(i, min(i + 2, B))) for i in range(0, B, 2)]
        bones = MS.skeleton_bones(J)
    else:
        scenes = [[0, 1, 2]] + [[b] for b in range(3, B)]
        bones = MS.skeleton_bones(J)[:(24 - Ks) // 2][:12]
    contacts = [MS.contact(0, J - 1, 1, J - 2, range(0, T), weight=2.0, meet=0.3)]
    if B >= 4 and layout == "pairs":
        contacts.append(MS.contact(3, 5, 2, J - 1, range(3, 30), weight=1.0, meet=0.0))
    if layout == "trio":
        contacts.append(MS.contact(2, 3, 0, 7, range(1, T), weight=0.5, meet=1.0))
    tables = MS.partner_tables(scenes, pose, lens, bones, T=T, J=J, contacts=contacts, radius=RADIUS, margin=MARGIN, weight=WEIGHT,
                               static_tracks=Ks)
    static = MS.batch_tracks(static_tracks(T), B, T) if Ks else None
    W, rec, tg, hit = ref_partner(x0, lens, mean, std, tables, contacts, static)
    return dict(x0=x0, mean=mean, std=std, lens=lens, pose=pose, scenes=scenes, bones=bones, contacts=contacts, tables=tables,
                static=static, W=W, rec=rec, tg=tg, hit=hit, J=J)


# ---- the restated x0 hook of tests/sampler_ref.loop_ref ------------------------------------------------------------------
def guidance_hook(lengths, ctl, tables, contacts, mask=None, seen=None):
    """``x0_hook`` of ``sampler_ref.loop_ref``: from the whole batch's x0 (after clipping and the edit blend) every row's partner
    records and contact targets, held fixed, then ``control_iters`` autograd steps down L + L_scene + L_tracks
    (``scene_tracks_ref.ref_tracks_loss_grad``).  ``ctl``: the control_* kwargs (CPU tensors); the target weights are the
    tables'.  ``seen`` collects per call and row (share of (t, j) a partner record penalises, least distance of a penalised
    joint to a capsule axis)."""
    import scene_tracks_ref as TR
    MS = pkg("motion_scene")
    one_minus_m = 1.0 if mask is None else 1.0 - mask.double()
    t = tables
    jp = ctl["control_joint_params"].double()
    static_targets = ctl.get("control_joints")

    def hook(x0):
        W = world_joints(x0, lengths, ctl["control_mean"], ctl["control_std"], t.pose)
        rec = partner_records(W, lengths, t)
        tg, hit = contact_targets(W, lengths, t, contacts)
        if static_targets is not None:
            tg = torch.where(hit[..., None], tg, static_targets.double())
        if seen is not None:
            for b in range(t.B):
                n = int(lengths[b])
                P = local_of(W[b], t.pose[b])
                d = MS.track_distances(P, rec[b, :n])  # (n, J, Km)
                q = rec[b, :n][:, None]
                pen = (q[..., 0] != 0) & (q[..., 2] > 0) & (q[..., 3] + jp[b, None, :, None, 0] - d > 0) & (jp[b, None, :, None, 1] > 0)
                jump = TR.track_stats(P, rec[b, :n], jp[b])[0]
                seen.append((float(pen.any(-1).double().mean()), float(jump.min())))
        for _ in range(ctl["control_iters"]):
            _, gr = TR.ref_tracks_loss_grad(x0, lengths, ctl["control_mean"], ctl["control_std"], rec, jp, ctl.get("control_scene"),
                                            tg, t.weights)
            x0 = x0 - ctl["control_scale"] * one_minus_m * gr
        return x0

    return hook

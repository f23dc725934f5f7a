"""GPU: exact reach (mdm_limb_pin) against its restatement tests/limb_pin_ref.py.

* parity of joints, the error report and its counts: t2m and KIT, all four limbs and the arms alone, B = 3, T = 40, lengths
  40 / 2 / 1; an interval, single keyframes, two pin frames closer than blend; blend 0, 5 and 12; targets NaN under weight 0;
* frames and lengths: T = 300 with a pin interval across frames 255 | 256, targets beyond reach, n = 1 and 2, no pins at all,
  NaN past every length, every sample equal to its own run at B = 1, T = length;
* rotations from motion_to_joints_fk on the rows joints_to_motion makes of a reach clip: parity of R', R' offset + parent =
  joint, R'^T R' = I, untouched rotations bit-equal;
* through a tiny trainer: pin_targets on generate_joints (with fix_feet and from_rotations), generate_rotations and
  generate_long_joints equals pin_limbs by hand on the same seed's unpinned result; generate_bvh changes the pinned limbs'
  channels only;
* bad arguments on the device path.

Tolerances.  A case's yardstick is the error of the restatement's all-fp32 form against its fp64 form on the same inputs, for
the quantity compared; GATE = 4 x that, the convention of tests/test_foot_skate_gpu.py.  A quantity whose yardstick is 0 is
compared bit for bit.  Nothing is gated against the kernel's own output, and no entry is left out: the clips keep the margins
that limb_pin_ref.reach_clip asserts.  tests/test_limb_pin_host.py shows that each likely mistake lies >= 100 gates away.
"""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from conftest import pkg

import limb_pin_ref as LP
import test_motion_features_gpu as TF
import test_motion_fk_gpu as TK

pytestmark = pytest.mark.gpu

GATE = 4.0
_MEMO = {}


def case(name, what="parity", arms=False):
    """Inputs are built once and shared; nothing writes to them.  -> (sk, limbs, joints, targets, weights, lengths)."""
    if (name, what, arms) not in _MEMO:
        sk = TF.ref_skel(name)
        limbs = LP.limbs_of(sk)
        if what == "parity":
            if arms:
                limbs = limbs[2:]
                got = LP.parity_case(sk, name, limbs, {0: LP.PARITY_PINS[2], 1: LP.PARITY_PINS[3]}, nan=True)
            else:
                got = LP.parity_case(sk, name, nan=True)
            _MEMO[name, what, arms] = (sk, limbs) + got
        else:
            j, G, W = getattr(LP, what)(sk)
            _MEMO[name, what, arms] = (sk, limbs, j[None], G[None], W[None], [len(j)])
    return _MEMO[name, what, arms]


def held(what, got, w32, w64):
    """got against the fp64 form within GATE x the fp32 form's own error; bit for bit where that error is 0."""
    yard = float(np.abs(w32.astype(np.float64) - w64).max()) if w64.size else 0.0
    err = float(np.abs(got.astype(np.float64) - w64).max()) if w64.size else 0.0
    print(f"{what}: measured {err:.3g} yardstick {yard:.3g}")
    if yard == 0.0:
        assert np.array_equal(got, w32), what
    else:
        assert err <= GATE * yard, (what, err, yard)
    return err, yard


def compare(name, limbs, j, lens, G, W, blend, what, rotations=None, limb_arg=None):
    P = pkg("postprocess")
    w64 = LP.pin_limbs(limbs, j, lens, G, W, blend=blend, ft=np.float64, rotations=rotations)
    w32 = LP.pin_limbs(limbs, j, lens, G, W, blend=blend, ft=np.float32, rotations=rotations)
    rot = None if rotations is None else torch.from_numpy(rotations).cuda()
    res = P.pin_limbs(torch.from_numpy(j).cuda(), lens, torch.from_numpy(G), torch.from_numpy(W), skeleton=name, limbs=limb_arg,
                      blend=blend, rotations=rot, return_error=True)
    out, (err, counts) = res[0].cpu().numpy(), res[-1]
    nl = len(limbs)
    assert out.shape == j.shape and out.dtype == np.float32 and err.shape == (len(lens), nl, 2, 2) and counts.shape == (len(lens), nl, 2)
    for b, n in enumerate(lens):
        assert not out[b, n:].any()
    held(f"{what} joints", out, w32[0], w64[0])
    held(f"{what} error report", err.cpu().numpy(), w32[2], w64[2])
    assert np.array_equal(counts.cpu().numpy(), w64[3]) and np.array_equal(w32[3], w64[3]), what
    kept = [x for x in range(j.shape[2]) if x not in [int(y) for q in limbs for y in q[1:]]]
    inside = np.arange(j.shape[1])[None, :, None, None] < np.asarray(lens)[:, None, None, None]
    assert np.array_equal(out[:, :, kept], np.where(inside, j[:, :, kept], 0)), what  # the rest of the body: every bit
    for b, n in enumerate(lens):  # and every (frame, limb) that no pin frame is near
        pin = LP.pin_flags(W[b, :n], limbs)
        act = LP.deltas(j[b, :n].astype(np.float64), G[b, :n], pin, limbs, blend, np.float64)[1]
        for l, q in enumerate(limbs):
            cols = [int(x) for x in q[1:] if x >= 0]
            assert np.array_equal(out[b, :n][~act[:, l]][:, cols], j[b, :n][~act[:, l]][:, cols]), (what, b, l)
    if rotations is not None:
        r = res[1].cpu().numpy()
        held(f"{what} rotations", r, w32[1], w64[1])
        return out, r, w32, w64
    return out, None, w32, w64


@pytest.mark.parametrize("arms", [False, True], ids=["all", "arms"])
@pytest.mark.parametrize("name", ["t2m", "kit"])
def test_parity(name, arms):
    """An interval with a keyframe 4 frames behind it, a single keyframe, two keyframes 4 apart; lengths 40 / 2 / 1; NaN under
    weight 0; weights on a root path, on knees / elbows and on one coordinate of an end joint pin nothing."""
    sk, limbs, j, G, W, lens = case(name, arms=arms)
    assert np.isnan(G).any()
    for blend in (0, 5, 12):
        out, _, w32, w64 = compare(name, limbs, j, lens, G, W, blend, f"{name} {'arms' if arms else 'all'} blend {blend}",
                                   limb_arg=["right_arm", "left_arm"] if arms else None)
        assert w64[3][0, :, 0].min() >= 1 and not w64[3][:, :, 1].any() and w64[2][:, :, 1].max() <= 1e-12 * LP.SCALE[name]


@pytest.mark.parametrize("what", ["long_clip", "clamped_clip"])
def test_frames(what):
    """More frames than threads with a pin interval across 255 | 256; targets beyond reach."""
    sk, limbs, j, G, W, lens = case("t2m", what)
    out, _, w32, w64 = compare("t2m", limbs, j, lens, G, W, 5, what)
    if what == "clamped_clip":
        assert w64[3][0, :, 1].tolist() == [0, 8, 10, 0] and w64[2][0, 1:3, 1, 1].min() > 0.1  # not met where out of reach


def test_no_pins_come_back_bit_for_bit():
    P = pkg("postprocess")
    sk, limbs, j, G, W, lens = case("t2m")
    jt = torch.from_numpy(j).cuda()
    rot = torch.randn(3, 40, 22, 3, 3, generator=torch.Generator().manual_seed(0)).cuda()
    W0 = W.copy()
    for q in limbs:  # every weight stays but one coordinate of each end joint: no pin frame is left
        W0[:, :, q[2], 1] = 0
    assert (W0 > 0).any()
    out, r, (err, counts) = P.pin_limbs(jt, None, torch.full(G.shape, float("nan")), torch.from_numpy(W0), rotations=rot,
                                        return_error=True)
    assert torch.equal(out, jt) and torch.equal(r, rot) and not err.any() and not counts.any()


@pytest.mark.parametrize("n", [1, 2])
def test_the_shortest(n):
    sk, limbs, j, G, W, lens = case("t2m")
    b = lens.index(n)
    for T in sorted({n, 2}):
        compare("t2m", limbs, j[b:b + 1, :T], [n], G[b:b + 1, :T], W[b:b + 1, :T], 5, f"n = {n} T = {T}")


def test_lengths():
    """NaN past every length changes nothing, and every sample equals its own run at B = 1, T = length."""
    P = pkg("postprocess")
    sk, limbs, j, G, W, lens = case("t2m")
    rot = torch.randn(3, 40, 22, 3, 3, generator=torch.Generator().manual_seed(1)).cuda()
    jt, gt, wt = torch.from_numpy(j).cuda(), torch.from_numpy(G).clone(), torch.from_numpy(W).clone()
    clean = P.pin_limbs(jt, lens, gt, wt, rotations=rot, return_error=True)
    for b, n in enumerate(lens):
        for t in (jt, gt, wt, rot):
            t[b, n:] = float("nan")
    o, r, (e, c) = P.pin_limbs(jt, lens, gt.cuda(), wt.cuda(), rotations=rot, return_error=True)
    for got, want in zip((o, r, e, c), (clean[0], clean[1]) + clean[2]):
        assert torch.equal(got, want)
    for b, n in enumerate(lens):
        assert not o[b, n:].any() and not r[b, n:].any()
        o1, r1, (e1, c1) = P.pin_limbs(jt[b:b + 1, :n], None, gt[b:b + 1, :n], wt[b:b + 1, :n], rotations=rot[b:b + 1, :n],
                                       return_error=True)
        assert torch.equal(o1[0], o[b, :n]) and torch.equal(r1[0], r[b, :n]) and torch.equal(e1[0], e[b]) and torch.equal(c1[0], c[b]), b


@pytest.mark.parametrize("name", ["t2m", "kit"])
def test_rotations(name):
    MF, P = pkg("motion_features"), pkg("postprocess")
    sk = TF.ref_skel(name)
    limbs = LP.limbs_of(sk)
    clip, G, W = LP.reach_clip(sk, limbs, 25, 4, {0: range(4, 10), 2: range(8, 16), 3: [20]}, scale=LP.SCALE[name], blends=(5,))
    F = 12 * sk.J - 1
    rows = MF.joints_to_motion(torch.from_numpy(clip).cuda()[None], skeleton=name)
    fj, fr, off = P.motion_to_joints_fk(rows, np.zeros(F, np.float32), np.ones(F, np.float32), skeleton=name, sigma=0.0,
                                        return_rotations=True, return_offsets=True)
    j, R, off = fj.cpu().numpy(), fr.cpu().numpy(), off[0].cpu().numpy().astype(np.float64)
    G2, W2 = (G[None, :24] + (j - clip[None, :24])).astype(np.float32), W[None, :24]  # the targets move with the joints
    LP.check_margins(limbs, j[0], G2[0], W2[0], 5)  # the inputs, not the kernel's output
    out, r, w32, w64 = compare(name, limbs, j, [24], G2, W2, 5, f"{name} fk", rotations=R)
    turned = [int(y) for q in limbs for y in q[1:] if y >= 0]
    kept = [x for x in range(sk.J) if x not in turned]
    assert np.array_equal(r[:, :, kept], R[:, :, kept])
    assert np.abs(r[:, :, turned] - R[:, :, turned]).max() > 1e-3  # and the limbs' did turn
    par = np.asarray(sk.parents)

    def residuals(jo, ro):
        jo, ro = np.asarray(jo, np.float64), np.asarray(ro, np.float64)
        bone = np.einsum("ntjab,jb->ntja", ro[:, :, turned], off[turned]) + jo[:, :, par[turned]] - jo[:, :, turned]
        orth = np.einsum("ntjab,ntjac->ntjbc", ro[:, :, turned], ro[:, :, turned]) - np.eye(3)
        return float(np.abs(bone).max()), float(np.abs(orth).max())

    (e_bone, e_orth), (y_bone, y_orth) = residuals(out, r), residuals(w32[0], w32[1])
    print(f"{name} R' offset + parent - joint: measured {e_bone:.3g} yardstick {y_bone:.3g}; R'^T R' - I: measured {e_orth:.3g} "
          f"yardstick {y_orth:.3g}")
    assert e_bone <= GATE * y_bone and e_orth <= GATE * y_orth


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _pad(clips, T):
    x = torch.zeros((len(clips), T) + tuple(clips[0].shape[1:]), device=clips[0].device)
    for i, c in enumerate(clips):
        x[i, :c.shape[0]] = c
    return x


def _channel_owners(text):
    """The node name of every MOTION column of a BVH text, and the MOTION rows."""
    head, motion = text.split("MOTION")
    owners, name = [], None
    for line in head.splitlines():
        m = re.match(r"\s*(ROOT|JOINT)\s+(\S+)", line)
        if m:
            name = m.group(2)
        m = re.match(r"\s*CHANNELS\s+(\d+)", line)
        if m:
            owners += [name] * int(m.group(1))
    rows = np.asarray([[float(v) for v in ln.split()] for ln in motion.splitlines()[3:] if ln.strip()])
    assert rows.shape[1] == len(owners)
    return owners, rows, head


def test_through_the_trainer():
    P, MR_ = pkg("postprocess"), pkg("motion_rig")
    tr = TF._tiny_trainer()
    mean, std = TK._mean_std(263, 22, 12)
    mean[-4:], std[-4:] = 0.5, 1.0
    caps, lens = ["a", "b", "c", "d"], torch.tensor([16, 16, 12, 9])
    ll = lens.tolist()
    g = torch.randn(4, 16, 22, 3, generator=torch.Generator().manual_seed(5)) * 0.3 + torch.tensor([0.0, 0.9, 0.0])
    w = torch.zeros(4, 16, 22)
    w[0, 4:9, 21], w[1, 7, 20], w[1, 10, 8], w[2, 2:6, 7], w[3, 8, 21] = 1.0, 2.0, 1.0, 0.5, 1.0  # wrists and ankles
    w[:, :, 0] = 0.3                                                                              # and the pelvis: no pin
    opts = dict(seed=0, sampler="ddim", sample_steps=5, batch_size=2, control_joints=g, control_weights=w)
    lim = P.limbs("t2m")

    def same(got, want):
        return all(_bits(a, want[i, :n]) for i, (a, n) in enumerate(zip(got, ll)))

    # generate_joints: after the temporal filter
    plain = tr.generate_joints(caps, lens, 263, mean, std, **opts)
    fixed = tr.generate_joints(caps, lens, 263, mean, std, pin_targets=True, pin_blend=3, **opts)
    want, (err, counts) = P.pin_limbs(_pad(plain, 16), lens, g, w, blend=3, return_error=True)
    assert same(fixed, want) and all(not _bits(a, b) for a, b in zip(fixed, plain))
    assert counts[:, :, 0].sum().item() == 5 + 2 + 4 + 1
    # after fix_feet: the pin has the last word
    feet = tr.generate_joints(caps, lens, 263, mean, std, fix_feet=True, blend=3, **opts)
    both = tr.generate_joints(caps, lens, 263, mean, std, fix_feet=True, blend=3, pin_targets=True, **opts)
    assert same(both, P.pin_limbs(_pad(feet, 16), lens, g, w, blend=5))
    # from_rotations composes
    fk = tr.generate_joints(caps, lens, 263, mean, std, from_rotations=True, **opts)
    fkp = tr.generate_joints(caps, lens, 263, mean, std, from_rotations=True, pin_targets=True, **opts)
    assert same(fkp, P.pin_limbs(_pad(fk, 16), lens, g, w))
    # generate_rotations: the rotations go through
    res0 = tr.generate_rotations(caps, lens, 263, mean, std, **opts)
    res = tr.generate_rotations(caps, lens, 263, mean, std, pin_targets=True, **opts)
    wj, wr = P.pin_limbs(_pad([v[0] for v in res0], 16), lens, g, w, rotations=_pad([v[1] for v in res0], 16))
    for i, n in enumerate(ll):
        assert _bits(res[i][0], wj[i, :n]) and _bits(res[i][1], wr[i, :n]) and _bits(res[i][2], res0[i][2])
    # a long motion of two segments: one pass over the canvas, targets in canvas frames
    scripts = [[("a", 16), ("b", 16)]]
    cg, cw = [torch.randn(28, 22, 3, generator=torch.Generator().manual_seed(6)) * 0.3], [torch.zeros(28, 22)]
    cw[0][10:15, 20], cw[0][26, 21] = 1.0, 1.0  # across the overlap (frames 12 .. 15), and near the end
    lopts = dict(overlap=4, seed=4, sampler="ddim", sample_steps=5, control_joints=cg, control_weights=cw)
    base = tr.generate_long_joints(scripts, 263, mean, std, **lopts)[0]
    lj = tr.generate_long_joints(scripts, 263, mean, std, pin_targets=True, **lopts)[0]
    assert lj.shape == (28, 22, 3) and _bits(lj, P.pin_limbs(base[None], None, cg[0][None], cw[0][None])[0]) and not _bits(lj, base)
    # BVH: only the pinned limbs' channels change
    only = dict(opts, control_weights=torch.zeros(4, 16, 22))
    only["control_weights"][:, 4:9, 21] = 1.0  # the right wrist
    t0 = tr.generate_bvh(caps, lens, 263, mean, std, **only)
    t1 = tr.generate_bvh(caps, lens, 263, mean, std, pin_targets=True, **only)
    rig = MR_.rig_of("t2m")
    arm = {rig.names[k] for k in range(rig.n_nodes) if rig.joint_of[k] in lim["right_arm"][:3]}
    assert len(arm) == 3
    for a, b in zip(t0, t1):
        (own, r0, h0), (_, r1, h1) = _channel_owners(a), _channel_owners(b)
        assert h0 == h1 and r0.shape == r1.shape
        moved = {own[k] for k in np.flatnonzero((r0 != r1).any(0))}
        assert moved and moved <= arm, moved
    with pytest.raises(ValueError, match="pin_targets"):
        tr.generate_joints(caps, lens, 263, mean, std, pin_targets=True, seed=0, sampler="ddim", sample_steps=5)
    with pytest.raises(ValueError, match="pin needs dim_pose"):
        tr.generate_joints(caps, lens, 263, mean, std, joints_num=21, pin_targets=True, **opts)


def test_bad_arguments_on_the_device_path():
    P, L = pkg("postprocess"), pkg("_lib")
    lib = L.lib()
    j = torch.zeros(2, 8, 22, 3, device="cuda")
    g, w = torch.zeros_like(j), torch.zeros_like(j)
    o, sc = torch.empty_like(j), torch.empty(2, 8, 8, 3, device="cuda")
    rot = torch.zeros(2, 8, 22, 3, 3, device="cuda")
    table = np.ascontiguousarray(list(P.limbs("t2m").values()), np.int32)

    def call(joints=j, targets=g, weights=w, limbs=table, nl=None, J=22, blend=5, B=2, T=8, rin=None, out=o, rout=None, scratch=sc):
        p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())  # noqa: E731
        lp = None if limbs is None else limbs.ctypes.data_as(C.c_void_p)
        return lib.mdm_limb_pin(p(joints), None, p(targets), p(weights), lp, C.c_int32(len(limbs) if nl is None else nl),
                                C.c_int32(J), C.c_int32(blend), C.c_int32(B), C.c_int32(T), p(rin), p(out), p(rout), None, None,
                                p(scratch), C.c_void_p(L.stream_ptr()))

    def tab(*rows):
        return np.ascontiguousarray(rows, np.int32)

    ARG, UNSUPPORTED = 1, 3
    assert call() == 0 and call(rin=rot, rout=torch.empty_like(rot)) == 0 and call(B=0) == 0 and call(limbs=table[2:]) == 0
    assert call(limbs=tab((2, 5, 8, 11), (2, 4, 7, 10))) == 0  # two limbs may share a root
    for kw in (dict(joints=None), dict(targets=None), dict(weights=None), dict(limbs=None, nl=4), dict(out=None), dict(scratch=None),
               dict(T=0), dict(blend=-1), dict(B=-1), dict(nl=0), dict(limbs=np.zeros((9, 4), np.int32), nl=9), dict(J=2), dict(J=33),
               dict(rin=rot), dict(rout=rot), dict(out=j), dict(out=g), dict(out=w), dict(rin=rot, rout=rot),
               dict(limbs=tab((2, 5, 22, -1))), dict(limbs=tab((2, 5, 8, -2))), dict(limbs=tab((-1, 5, 8, 11))),
               dict(limbs=tab((2, 5, 5, 11))), dict(limbs=tab((2, 5, 8, 2))), dict(limbs=tab((2, 5, 8, 11), (1, 4, 8, -1))),
               dict(limbs=tab((2, 5, 8, 11), (8, 1, 4, -1))), dict(limbs=tab((2, 5, 8, 11), (1, 4, 7, 10)), J=11)):
        assert call(**kw) == ARG, kw
    assert call(T=P.limb_pin_max_frames() + 1) == UNSUPPORTED  # returns before any launch
    assert P.limb_pin_max_frames() >= P.foot_skate_max_frames()
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        P.pin_limbs(j.cpu(), None, g, w)                                # a CPU tensor
    with pytest.raises(ValueError):
        P.pin_limbs(j, None, g[:, :7], w)
    with pytest.raises(ValueError):
        P.pin_limbs(j, None, g, w, rotations=rot.cpu())
    with pytest.raises(ValueError):
        P.pin_limbs(j, [8, 9], g, w)

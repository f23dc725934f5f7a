"""CPU: exact reach's restatement (tests/limb_pin_ref.py) does what §28 promises, tells the likely mistakes from
the truth on the GPU tests' inputs, ``postprocess.limbs`` / ``check_pin_limbs`` name the limbs and reject bad arguments, and the
trainer hands the call's own targets to the output chain.  No device."""
import types

import numpy as np
import pytest
import torch

from conftest import pkg

import limb_pin_ref as LP
from test_foot_skate_host import fk_rotation_inputs, ref_skel

GATE = 4.0


def bone(j, a, b):
    return np.linalg.norm(np.asarray(j, np.float64)[..., a, :] - np.asarray(j, np.float64)[..., b, :], axis=-1)


@pytest.mark.parametrize("name", ["t2m", "kit"])
def test_what_exact_reach_promises(name):
    sk = ref_skel(name)
    limbs = LP.limbs_of(sk)
    j, G, W, lens = LP.parity_case(sk, name, nan=True)
    moved = sorted(int(x) for q in limbs for x in q[1:] if x >= 0)
    kept = [x for x in range(sk.J) if x not in moved]
    for blend in (0, 5, 12):
        out, _, err, counts = LP.pin_limbs(limbs, j, lens, G, W, blend=blend)
        assert np.isfinite(out).all()  # NaN under weight 0 is never read
        for b, n in enumerate(lens):
            pin = LP.pin_flags(W[b, :n], limbs)
            _, act = LP.deltas(j[b, :n].astype(np.float64), G[b, :n], pin, limbs, blend, np.float64)
            assert np.array_equal(counts[b, :, 0], pin.sum(0)) and not counts[b, :, 1].any()
            for l, q in enumerate(limbs):
                ts = np.flatnonzero(pin[:, l])
                assert np.abs(out[b, ts, q[2]] - G[b, ts, q[2]]).max(initial=0) <= 1e-12 * LP.SCALE[name]  # on the target
                for a_, b_ in ((q[0], q[1]), (q[1], q[2])) + (((q[2], q[3]),) if q[3] >= 0 else ()):
                    assert np.abs(bone(out[b, :n], a_, b_) - bone(j[b, :n], a_, b_)).max() <= 1e-12 * LP.SCALE[name]
                idle = ~act[:, l]
                cols = [int(x) for x in q[1:] if x >= 0]
                assert np.array_equal(out[b, :n][idle][:, cols], j[b, :n][idle][:, cols].astype(np.float64))  # every bit
                if blend == 0:
                    assert np.array_equal(act[:, l], pin[:, l])  # nothing changes outside the pin frames
            assert np.array_equal(out[b, :n, kept], j[b, :n, kept].astype(np.float64))  # the rest of the body: every bit
            assert not out[b, n:].any()
        assert err[0, :, 0, 0].min() > 0.03 * LP.SCALE[name] and err[:, :, 1].max() <= 1e-12 * LP.SCALE[name]
        assert (err[..., 1] >= err[..., 0]).all()  # max >= mean
    o32 = LP.pin_limbs(limbs, j, lens, G, W, blend=12, ft=np.float32)[0]
    assert o32.dtype == np.float32 and 0 < np.abs(o32 - out).max() < 1e-5 * LP.SCALE[name]


def test_the_pin_flag_reads_the_weights_alone():
    sk = ref_skel("t2m")
    limbs = LP.limbs_of(sk)
    j, G, W = LP.reach_clip(sk, limbs, 40, 1, LP.PARITY_PINS)
    pin = LP.pin_flags(W, limbs)
    assert {l: np.flatnonzero(pin[:, l]).tolist() for l in range(4)} == {l: sorted(f) for l, f in LP.PARITY_PINS.items()}
    assert (W[:, 0, [0, 2]] > 0).all() and (W[:, limbs[0][1]] > 0).all()  # a root path and targets on knees: not pins
    assert ((W[:, limbs[0][2]] > 0).sum(-1) == 1).any()                   # a height on an ankle: not a pin
    want = LP.pin_clip(limbs, j, G, W, 5)[0]
    W2, G2 = W.copy(), G.copy()
    W2[W2 > 0] = 0.1 + 3.0 * np.random.RandomState(0).rand(int((W2 > 0).sum())).astype(np.float32)  # magnitudes do not matter
    G2[W == 0] = np.nan
    assert np.array_equal(LP.pin_clip(limbs, j, G2, W2, 5)[0], want)
    none = LP.pin_clip(limbs, j, G2, np.zeros_like(W), 5, rotations=np.ones((40, sk.J, 3, 3), np.float32))
    assert np.array_equal(none[0], j.astype(np.float64)) and (none[1] == 1).all() and not none[2].any() and not none[3].any()


def test_blend_weights_and_their_sums():
    sk = ref_skel("t2m")
    limbs = LP.limbs_of(sk)
    j, G, W = LP.reach_clip(sk, limbs, 40, 1, LP.PARITY_PINS)
    p = j.astype(np.float64)
    pin = LP.pin_flags(W, limbs)
    d, act = LP.deltas(p, G, pin, limbs, 5, np.float64)
    l, e = 3, limbs[3][2]  # the left arm: pin frames 20 and 24, the three frames between them hear both
    dL, dR = G[20, e] - p[20, e], G[24, e] - p[24, e]
    assert np.array_equal(d[20, l], dL) and np.array_equal(d[24, l], dR)
    fade = lambda k: 1 - (3 * (k / 6) ** 2 - 2 * (k / 6) ** 3)  # noqa: E731
    for t in (21, 22, 23):
        wl, wr = fade(t - 20), fade(24 - t)
        assert wl + wr > 1.0
        assert np.allclose(d[t, l], (wl * dL + wr * dR) / (wl + wr), rtol=0, atol=1e-15)
    for k in range(1, 6):  # one neighbour: the weights sum to less than 1 and are not normalised
        assert np.allclose(d[20 - k, l], fade(k) * dL, rtol=0, atol=1e-15) and np.allclose(d[24 + k, l], fade(k) * dR, rtol=0, atol=1e-15)
    assert act[15:30, l].all() and not act[:15, l].any() and not act[30:, l].any() and not d[:15, l].any()
    dw, _ = LP.deltas(p, G, pin, limbs, 5, np.float64, wrong="unnormalised")
    assert np.abs(dw[22, l] - d[22, l]).max() > 1e-3
    d0, act0 = LP.deltas(p, G, pin, limbs, 0, np.float64)
    assert np.array_equal(act0, pin) and not d0[~pin].any()


def test_out_of_reach_the_limb_goes_as_far_as_it_goes():
    sk = ref_skel("t2m")
    limbs = LP.limbs_of(sk)
    j, G, W = LP.clamped_clip(sk)
    out, _, err, counts = LP.pin_clip(limbs, j, G, W, 5)
    assert counts[:, 1].tolist() == [0, 8, 10, 0] and counts[:, 0].tolist() == [1, 14, 16, 0]
    for l in (1, 2):
        q = limbs[l]
        full = bone(j, q[0], q[1]) + bone(j, q[1], q[2])
        assert np.abs(bone(out, q[0], q[2]) / full).max() <= 1 - 1e-4 + 1e-12
        assert err[l, 1, 1] > 0.1 and err[l, 1, 0] < err[l, 0, 0]  # not met, yet nearer
        for a_, b_ in ((q[0], q[1]), (q[1], q[2])):
            assert np.abs(bone(out, a_, b_) - bone(j, a_, b_)).max() <= 1e-12
    assert err[0, 1, 1] <= 1e-12


@pytest.mark.parametrize("name", ["t2m", "kit"])
def test_wrong_variants_lie_far_from_the_truth(name):
    """On the GPU tests' inputs every mistake of LP.WRONG lies >= 100 gates (gate = 4 x the fp32 form's own error) away."""
    sk = ref_skel(name)
    limbs = LP.limbs_of(sk)
    j, G, W, lens = LP.parity_case(sk, name)
    kw = dict(blend=12)
    o64 = LP.pin_limbs(limbs, j, lens, G, W, ft=np.float64, **kw)[0]
    gate = GATE * np.abs(LP.pin_limbs(limbs, j, lens, G, W, ft=np.float32, **kw)[0] - o64).max()
    assert 0 < gate < 1e-5 * LP.SCALE[name]
    for w in LP.WRONG:
        if w == "q_right":
            continue
        far = np.abs(LP.pin_limbs(limbs, j, lens, G, W, ft=np.float64, wrong=w, **kw)[0] - o64).max() / gate
        print(name, w, f"{far:.3g} gates")
        assert far >= 100, (w, far)
    fj, fr, G2, W2 = fk_case(sk, name)
    r64 = LP.pin_clip(limbs, fj, G2, W2, 5, np.float64, fr)[1]
    gate = GATE * np.abs(LP.pin_clip(limbs, fj, G2, W2, 5, np.float32, fr)[1] - r64).max()
    far = np.abs(LP.pin_clip(limbs, fj, G2, W2, 5, np.float64, fr, wrong="q_right")[1] - r64).max() / gate
    print(name, "q_right", f"{far:.3g} gates")
    assert gate > 0 and far >= 100, far


def fk_case(sk, name):
    """The construction of the GPU rotation test's inputs on the CPU restatements: a reach clip's joints, global rotations
    and offsets as the forward kinematics of its own feature rows gives them, the targets moved along with the joints."""
    limbs = LP.limbs_of(sk)
    j, G, W = LP.reach_clip(sk, limbs, 25, 4, {0: range(4, 10), 2: range(8, 16), 3: [20]}, scale=LP.SCALE[name], blends=(5,))
    fj, fr, _ = fk_rotation_inputs(sk, name, j)
    fj, fr = fj[0], fr[0]
    G2 = (G[:len(fj)] + (fj - j[:len(fj)])).astype(np.float32)
    LP.check_margins(limbs, fj, G2, W[:len(fj)], 5)
    return fj, fr, G2, W[:len(fj)]


def test_rotations_turn_with_the_bones():
    sk = ref_skel("t2m")
    limbs = LP.limbs_of(sk)
    j, G, W = LP.reach_clip(sk, limbs, 25, 4, {0: range(4, 10), 2: range(8, 16), 3: [20]}, blends=(5,))
    fj, fr, off = fk_rotation_inputs(sk, "t2m", j)
    fj, fr, off = fj[0], fr[0], np.asarray(off[0], np.float64)
    G2 = (G[:len(fj)] + (fj - j[:len(fj)])).astype(np.float32)
    out, R, _, _ = LP.pin_clip(limbs, fj, G2, W[:len(fj)], 5, np.float64, fr)
    turned = sorted(int(x) for q in limbs for x in q[1:] if x >= 0)
    par = np.asarray(sk.parents)
    res = np.einsum("tjab,jb->tja", R[:, turned], off[turned]) + out[:, par[turned]] - out[:, turned]
    before = np.einsum("tjab,jb->tja", fr[:, turned].astype(np.float64), off[turned]) + fj[:, par[turned]] - fj[:, turned]
    assert np.abs(res).max() <= np.abs(before).max() + 1e-7  # R' offset + parent = joint as well as it held going in
    assert np.abs(np.einsum("tjab,tjac->tjbc", R[:, turned], R[:, turned]) - np.eye(3)).max() < 1e-5
    kept = [x for x in range(sk.J) if x not in turned]
    assert np.array_equal(R[:, kept], fr[:, kept].astype(np.float64)) and np.abs(R[:, turned] - fr[:, turned]).max() > 1e-3


def test_generator_margins_hold_for_every_gpu_case():
    """reach_clip asserts its margins itself; this builds every clip the GPU tests use, here on the CPU."""
    for name in ("t2m", "kit"):
        sk = ref_skel(name)
        LP.parity_case(sk, name)
        LP.parity_case(sk, name, nan=True)
        LP.parity_case(sk, name, LP.limbs_of(sk)[2:], {0: LP.PARITY_PINS[2], 1: LP.PARITY_PINS[3]})
        fk_case(sk, name)
    sk = ref_skel("t2m")
    limbs = LP.limbs_of(sk)
    j, G, W = LP.long_clip(sk)
    pin = LP.pin_flags(W, limbs)
    assert pin[250:263, 2].all() and not pin[249, 2] and not pin[263, 2]  # one interval across frames 255 | 256
    LP.clamped_clip(sk)
    with pytest.raises(AssertionError, match="reach"):   # and it does refuse
        LP.reach_clip(sk, limbs, 40, 1, LP.PARITY_PINS, offset=0.5)
    with pytest.raises(AssertionError, match="bend"):
        LP.reach_clip(sk, limbs, 40, 1, LP.PARITY_PINS, stretch=0.9985, offset=0.001)
    with pytest.raises(AssertionError, match="weights"):
        LP.check_margins(limbs, j, G, np.where(W > 0, 0.05, 0).astype(np.float32), 5)


def test_limbs_by_name():
    P, MF = pkg("postprocess"), pkg("motion_features")
    assert P.limbs("t2m") == dict(right_leg=(2, 5, 8, 11), left_leg=(1, 4, 7, 10), right_arm=(17, 19, 21, -1), left_arm=(16, 18, 20, -1))
    assert P.limbs("kit") == dict(right_leg=(12, 13, 14, 15), left_leg=(17, 18, 19, 20), right_arm=(5, 6, 7, -1), left_arm=(8, 9, 10, -1))
    assert tuple(P.limbs("t2m")) == P.LIMB_NAMES == LP.LIMB_NAMES
    for name in ("t2m", "kit"):
        assert np.array_equal(np.asarray(list(P.limbs(name).values())), LP.limbs_of(ref_skel(name)))
        legs = P.leg_joints(MF.SKELETONS[name])  # the legs of remove_foot_skate
        assert sorted(legs) == sorted([P.limbs(name)["right_leg"], P.limbs(name)["left_leg"]])
    with pytest.raises(ValueError):
        P.limbs("smpl")


def test_check_pin_limbs_value_errors():
    P, MF = pkg("postprocess"), pkg("motion_features")
    sk = MF.SKELETONS["t2m"]
    j = torch.zeros(2, 8, 22, 3, device="meta")  # not a CPU tensor; nothing here reads its values
    g, w = torch.zeros(2, 8, 22, 3), torch.ones(2, 8, 22, 3)
    ok = P.check_pin_limbs(j, [8, 3], g, w, torch.zeros(2, 8, 22, 3, 3, device="meta"), sk)
    assert ok[0].shape == (2, 8, 22, 3) and ok[5].dtype == np.int32 and ok[5].tolist() == [list(v) for v in P.limbs("t2m").values()]
    for shape in ((2,), (2, 8), (2, 8, 22), (2, 1, 22, 1), (2, 8, 22, 3)):  # as control_weights broadcast
        assert P.check_pin_limbs(j, None, g, torch.ones(shape), None, sk)[3].shape == (2, 8, 22, 3)
    assert P.check_pin_limbs(j, None, g, w, None, sk, limbs=["left_arm", (2, 5, 8)])[5].tolist() == [[16, 18, 20, -1], [2, 5, 8, -1]]
    assert P.check_pin_limbs(j, None, g, w, None, sk, limbs="right_leg")[5].tolist() == [[2, 5, 8, 11]]
    one = P.check_pin_limbs(j[0], None, g[0], torch.ones(8), None, sk)
    assert one[0].shape == (1, 8, 22, 3) and one[3].shape == (1, 8, 22, 3)
    nan_w = w.clone()
    nan_w[1, 3:] = float("nan")
    P.check_pin_limbs(j, [8, 3], g, nan_w, None, sk)  # frames past a length are never read
    nan_w[0, 0, 0, 0] = float("nan")
    bad = [dict(joints=torch.zeros(2, 8, 21, 3, device="meta")), dict(joints=torch.zeros(2, 0, 22, 3, device="meta")),
           dict(joints=torch.zeros(8, 3, device="meta")), dict(lengths=[8]), dict(lengths=[8, 0]), dict(lengths=[8, 9]),
           dict(targets=torch.zeros(2, 7, 22, 3)), dict(targets=torch.zeros(2, 8, 22)), dict(targets=torch.zeros(1, 8, 22, 3)),
           dict(targets=torch.zeros(2, 8, 22, 3, dtype=torch.int64)),
           dict(weights=torch.ones(8)), dict(weights=torch.ones(2, 8, 22, 3, 1)), dict(weights=torch.ones(2, 8, 22, 2)),
           dict(weights=torch.ones(8, 22, 3)), dict(weights=-w), dict(weights=nan_w), dict(weights=w * float("inf")),
           dict(rotations=torch.zeros(2, 8, 22, 3, device="meta")), dict(rotations=torch.zeros(2, 8, 22, 3, 3)),
           dict(blend=-1), dict(blend=1.5), dict(joints=torch.zeros(2, 8, 22, 3)),
           dict(limbs=[]), dict(limbs=["right_leg"] * 9), dict(limbs=["right_hand"]), dict(limbs=[(2, 5)]), dict(limbs=[(2, 5, 22)]),
           dict(limbs=[(2, 5, 8, -2)]), dict(limbs=[(2, 5, -1, 11)]), dict(limbs=[(2, 5, 5, 11)]), dict(limbs=[(2, 5, 8, 2)]),
           dict(limbs=["right_leg", (1, 4, 8)]), dict(limbs=["right_leg", (8, 1, 4)]), dict(limbs=["right_leg", "right_leg"]),
           dict(joints=torch.zeros(1, P.limb_pin_max_frames() + 1, 22, 3, device="meta"), lengths=None,
                targets=torch.zeros(1, P.limb_pin_max_frames() + 1, 22, 3), weights=torch.ones(1))]
    for kw in bad:
        args = dict(joints=j, lengths=[8, 3], targets=g, weights=w, rotations=None, sk=sk)
        args.update(kw)
        with pytest.raises(ValueError):
            P.check_pin_limbs(**args)
    assert P.limb_pin_max_frames() >= P.foot_skate_max_frames() >= pkg("trainer").MAX_JOINTS_FRAMES


def test_pin_pair_over_the_padded_batch():
    MO = pkg("motion_outputs")
    g = torch.arange(2 * 10 * 22 * 3, dtype=torch.float32).reshape(2, 10, 22, 3)
    w = torch.rand(2, 10, 22, generator=torch.Generator().manual_seed(0))
    a, b = MO.pin_pair((g, w), 2, 8, 22)  # targets over T_max = 10, the padded batch has 8 frames
    assert a.shape == b.shape == (2, 8, 22, 3) and torch.equal(a, g[:, :8]) and torch.equal(b, w[:, :8, :, None].expand(2, 8, 22, 3))
    a, b = MO.pin_pair((g, w), 2, 12, 22)  # a batch padded past the targets: weight 0 there
    assert torch.equal(a[:, :10], g) and not b[:, 10:].any() and not a[:, 10:].any()
    a, b = MO.pin_pair(([g[0, :7], g[1]], [torch.ones(7), w[1]]), 2, 10, 22)  # canvases: one pair per motion
    assert torch.equal(a[0, :7], g[0, :7]) and bool((b[0, :7] == 1).all()) and not b[0, 7:].any() and torch.equal(a[1], g[1])
    for bad in ((g, None), (g,), (g[:1], w), (g[..., :2], w), (g, w[:, :9]), ([g[0]], [w[0]]), ([g[0], g[1]], w)):
        with pytest.raises(ValueError):
            MO.pin_pair(bad, 2, 10, 22)
    assert MO.pin_kw(None, 7) == {} and MO.pin_kw((g, w), 7) == dict(pin=(g, w), pin_blend=7)


class Seen(Exception):
    pass


def test_the_trainer_hands_on_the_calls_own_targets(monkeypatch):
    """No HIP library: generation and the output chain are stand-ins; what reaches joints_batch is what the call was given."""
    Tr, MO = pkg("trainer"), pkg("motion_outputs")
    tr = Tr.DDPMTrainer.__new__(Tr.DDPMTrainer)
    tr.encoder = types.SimpleNamespace(num_frames=16, eval=lambda: None)
    tr.device = "cpu"
    seen = {}

    def gen(caption, m_lens, dim_pose, batch_size=8, **kw):
        seen["gen"] = kw
        return [torch.zeros(16, dim_pose) for _ in caption]

    def gen_long(scripts, dim_pose, **kw):
        seen["gen"] = kw
        return [torch.zeros(28, dim_pose), torch.zeros(12, dim_pose)]

    def stub(motions, lens, dim_pose, mean, std, joints_num, sigma, from_rotations=False, offsets=None, return_rotations=False,
             fix_feet=False, blend=5, **kw):
        seen["out"] = dict(kw, lens=list(lens), fix_feet=fix_feet, from_rotations=from_rotations)
        raise Seen

    tr.generate = tr.generate_bucketed = gen
    tr.generate_long = gen_long
    monkeypatch.setattr(MO, "joints_batch", stub)
    mean, std = np.zeros(263, np.float32), np.ones(263, np.float32)
    caps, lens = ["a", "b"], torch.tensor([16, 12])
    g, w = torch.randn(2, 16, 22, 3, generator=torch.Generator().manual_seed(0)), torch.ones(2, 16, 22)
    calls = [lambda **k: tr.generate_joints(caps, lens, 263, mean, std, **k),
             lambda **k: tr.generate_joints(caps, lens, 263, mean, std, bucketed=True, fix_feet=True, **k),
             lambda **k: tr.generate_rotations(caps, lens, 263, mean, std, **k),
             lambda **k: tr.generate_bvh(caps, lens, 263, mean, std, **k),
             lambda **k: tr.generate_frames(caps, lens, 263, mean, std, **k),
             lambda **k: tr.generate_gif(caps, lens, 263, mean, std, **k)]
    for call in calls:
        with pytest.raises(ValueError, match="pin_targets=True pins the call's own control_joints / control_weights"):
            call(pin_targets=True)
        with pytest.raises(ValueError, match="pin_targets"):
            call(pin_targets=True, control_joints=g)
        with pytest.raises(Seen):  # off by default: nothing about pins reaches the output chain
            call(control_joints=g, control_weights=w)
        assert "pin" not in seen["out"] and "pin_blend" not in seen["out"] and seen["gen"]["control_joints"] is g
        with pytest.raises(Seen):
            call(pin_targets=True, pin_blend=3, control_joints=g, control_weights=w)
        assert seen["out"]["pin"][0] is g and seen["out"]["pin"][1] is w and seen["out"]["pin_blend"] == 3
        assert seen["out"]["lens"] == [16, 12] and seen["gen"]["control_joints"] is g and "pin_targets" not in seen["gen"]
    # long motions: one canvas pair per motion
    scripts = [[("a", 16), ("b", 16)], [("c", 12)]]
    cg, cw = [torch.zeros(28, 22, 3), torch.zeros(12, 22, 3)], [torch.ones(28), torch.ones(12, 22)]
    for call in (lambda **k: tr.generate_long_joints(scripts, 263, mean, std, overlap=4, **k),
                 lambda **k: tr.generate_long_bvh(scripts, 263, mean, std, overlap=4, **k),
                 lambda **k: tr.generate_long_gif(scripts, 263, mean, std, overlap=4, **k)):
        with pytest.raises(ValueError, match="pin_targets"):
            call(pin_targets=True)
        with pytest.raises(Seen):
            call(control_joints=cg, control_weights=cw)
        assert "pin" not in seen["out"]
        with pytest.raises(Seen):
            call(pin_targets=True, control_joints=cg, control_weights=cw)
        assert seen["out"]["pin"][0] is cg and seen["out"]["pin"][1] is cw and seen["out"]["pin_blend"] == 5
        assert seen["out"]["lens"] == [28, 12] and seen["gen"]["control_joints"] is cg and "pin_targets" not in seen["gen"]
    # several characters: each stage's targets are already in the character's own frame
    MS = pkg("motion_scene")
    world = torch.randn(16, 22, 3, generator=torch.Generator().manual_seed(1))
    scene = [dict(caption="a", length=16, position=(1.0, -2.0), yaw=0.5, control_joints=world, control_weights=torch.ones(16, 22))]
    with pytest.raises(Seen):
        tr.generate_together([scene], 263, mean, std, pin_targets=True, pin_blend=2)
    tg, wt = seen["out"]["pin"]
    assert torch.equal(tg[0], MS.to_local(world, (1.0, -2.0), 0.5)) and tuple(wt.shape) == (1, 16, 22, 3) and bool((wt == 1).all())
    assert seen["out"]["pin_blend"] == 2 and seen["gen"]["control_joints"] is tg
    with pytest.raises(ValueError, match="pin_targets"):
        tr.generate_together([[dict(caption="a", length=16)]], 263, mean, std, pin_targets=True)
    stages = []
    monkeypatch.setattr(MO, "joints_batch", lambda motions, lens, *a, **kw: (stages.append(kw), (torch.zeros(len(lens), 16, 22, 3), None, None, lens))[1])
    tr.generate_together([[dict(caption="a", length=16), scene[0]]], 263, mean, std, pin_targets=True, bones=[(0, 3)])
    assert "pin" not in stages[0] and torch.equal(stages[1]["pin"][0], tg)  # a stage without targets runs without pins

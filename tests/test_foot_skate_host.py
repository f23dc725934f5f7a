"""CPU: the foot-skate clean-up's restatement (tests/foot_skate_ref.py) does what §18 promises, tells the likely
mistakes from the truth on the GPU tests' inputs, and ``postprocess.check_foot_skate`` rejects bad arguments.  No device."""
import numpy as np
import pytest
import torch

from conftest import pkg

import foot_skate_ref as FS
import motion_features_ref as MR
import motion_fk_ref as FR

GATE = 4.0
HALF = np.full(4, 0.5, np.float32)


def ref_skel(name):
    sk = pkg("motion_features").SKELETONS[name]
    return MR.skeleton_from_tables(sk.chains, sk.raw_offsets, sk.face, sk.feet, sk.legs)


def bones(j, sk):
    j = np.asarray(j, np.float64)
    return np.linalg.norm(j[..., 1:, :] - j[..., np.asarray(sk.parents[1:]), :], axis=-1)


def fk_rotation_inputs(sk, name, clip):
    """Joints, global rotations and offsets of a walk clip as the forward kinematics of its own feature rows gives them (the
    CPU restatements of joints_to_motion and motion_to_joints_fk): the construction of the GPU rotation test's inputs."""
    rows, _ = MR.joints_to_motion(sk, [clip.astype(np.float64)], feet_thre=FS.FEET_THRE[name])
    F = rows.shape[-1]
    return FR.motion_to_joints_fk(sk, rows, np.zeros(F, np.float32), np.ones(F, np.float32))


@pytest.mark.parametrize("name", ["t2m", "kit"])
def test_what_the_clean_up_promises(name):
    sk = ref_skel(name)
    j, v, lens = FS.parity_case(sk, name)
    legs = FS.legs_of(sk)
    moved = sorted(x for leg in legs for x in leg[1:])
    kept = [x for x in range(sk.J) if x not in moved]
    for blend in (0, 5, 12):
        out, _, slide, pairs = FS.remove_foot_skate(sk, j, lens, v, HALF, blend=blend)
        for b, n in enumerate(lens):
            assert np.abs(bones(out[b, :n], sk) - bones(j[b, :n], sk)).max() <= 1e-12
            assert np.array_equal(out[b, :n, kept], j[b, :n, kept].astype(np.float64))  # hips and upper body: every bit
            assert not out[b, n:].any()
        assert pairs[0].min() >= 10 and not pairs[2].any()  # a clip of one frame has no pair
        assert slide[0, 0].min() > 1e-3                      # the clip does skate
        assert slide[0, 1, [0, 2]].max() <= 1e-12, slide[0]  # ankles: pinned
        assert (slide[0, 1] <= slide[0, 0]).all()            # toes: aimed, no worse than before
    # fp32 form: the same to rounding
    o32 = FS.remove_foot_skate(sk, j, lens, v, HALF, blend=12, ft=np.float32)[0]
    assert o32.dtype == np.float32 and 0 < np.abs(o32 - out).max() < 1e-5 * FS.SCALE[name]


def test_heights_of_pinned_ankles_move_only_with_the_reach():
    """The targets keep their heights: where the target is in reach the ankle's height is the input's."""
    sk = ref_skel("t2m")
    j, v, lens = FS.parity_case(sk, "t2m")
    out = FS.remove_foot_skate(sk, j, lens, v, HALF, blend=5)[0]
    for leg in FS.legs_of(sk):
        assert np.abs(out[0, :, leg[2], 1] - j[0, :, leg[2], 1]).max() <= 1e-12


def test_a_clip_without_contact_comes_back_unchanged():
    sk = ref_skel("t2m")
    j, v = FS.walk_clip(sk, 24, 7, contact=False)
    assert not FS.value_labels(v, HALF).any()
    R = np.random.RandomState(0).randn(24, sk.J, 3, 3).astype(np.float32)
    for ft in (np.float64, np.float32):
        out, rot, slide, pairs = FS.clean_clip(sk, j, FS.value_labels(v, HALF), 5, ft, R)
        assert np.array_equal(out, j.astype(ft)) and np.array_equal(rot, R.astype(ft)) and not slide.any() and not pairs.any()


def test_weight_normalisation_matters_in_a_gap_shorter_than_blend():
    sk = ref_skel("t2m")
    j, v, lens = FS.parity_case(sk, "t2m")
    lab = FS.value_labels(v[0], HALF)
    gaps = [t for t in range(1, 23) if not lab[t, 0] and lab[:t, 0].any() and lab[t:, 0].any()]
    assert 0 < len(gaps) < 5  # the ankle's swing: shorter than blend 5, so both neighbours weigh in
    d, act = FS.deltas(sk, j[0].astype(np.float64), lab, 5, np.float64)
    dw, _ = FS.deltas(sk, j[0].astype(np.float64), lab, 5, np.float64, wrong="unnormalised")
    assert act[gaps, 0].all() and np.abs(d[gaps, 0] - dw[gaps, 0]).max() > 1e-4
    wsum = [FS._fade(k, 5, np.float64) + FS._fade(len(gaps) + 1 - k, 5, np.float64) for k in range(1, len(gaps) + 1)]
    assert max(wsum) > 1.0
    d0, act0 = FS.deltas(sk, j[0].astype(np.float64), lab, 0, np.float64)
    assert not act0[gaps, 0].any() and not d0[gaps, 0].any()  # blend 0: no change outside the runs


@pytest.mark.parametrize("ft", [np.float64, np.float32])
def test_straight_leg_fallback(ft):
    """An axis-aligned straight leg: the knee's own bend direction is exactly 0 in both precisions, so world +Z decides, and
    world +X where the leg lies along Z."""
    sk = ref_skel("t2m")
    jh, jk, ja, jt = FS.legs_of(sk)[0]
    lab = np.zeros((1, 4), bool)
    lab[0, 0] = True  # a run of one frame: the anchor is the ankle itself, the target is where it is
    for down, want in (((0, -1, 0), (0, 0, 1)), ((0, 0, 1), (1, 0, 0))):
        down, want = np.asarray(down, np.float32), np.asarray(want, np.float64)
        j = np.zeros((1, sk.J, 3), np.float32)
        j[0, jh] = (0.25, 1.0, -0.5)
        j[0, jk], j[0, ja] = j[0, jh] + 0.5 * down, j[0, jh] + 1.0 * down
        j[0, jt] = j[0, ja] + np.asarray((0.125, 0, 0), np.float32)
        diag = {}
        out = FS.clean_clip(sk, j, lab, 0, ft, diag=diag)[0]
        assert diag["bend"][0] == 0.0
        k = out[0, jk].astype(np.float64) - j[0, jh]
        side = k - (k @ down.astype(np.float64)) * down
        assert np.linalg.norm(side) > 1e-3 and np.allclose(side / np.linalg.norm(side), want, atol=1e-6)
        assert abs(np.linalg.norm(k) - 0.5) < 1e-6 and np.isfinite(out).all()
        assert abs(np.linalg.norm(out[0, ja] - j[0, jh]) - 0.9999) < 1e-6  # the straight leg is beyond the reach clamp


@pytest.mark.parametrize("name", ["t2m", "kit"])
def test_wrong_variants_lie_far_from_the_truth(name):
    """On the GPU tests' inputs every mistake of FS.WRONG lies >= 100 gates (gate = 4 x the fp32 form's own error) away."""
    sk = ref_skel(name)
    j, v, lens = FS.parity_case(sk, name)
    kw = dict(values=v, thre=HALF, blend=12)
    o64 = FS.remove_foot_skate(sk, j, lens, ft=np.float64, **kw)[0]
    gate = GATE * np.abs(FS.remove_foot_skate(sk, j, lens, ft=np.float32, **kw)[0] - o64).max()
    assert 0 < gate < 1e-5 * FS.SCALE[name]
    for w in FS.WRONG:
        if w == "q_right":
            continue
        far = np.abs(FS.remove_foot_skate(sk, j, lens, ft=np.float64, wrong=w, **kw)[0] - o64).max() / gate
        print(name, w, f"{far:.3g} gates")
        assert far >= 100, (w, far)
    # rotations: the inputs of the GPU rotation test
    clip, vals = FS.walk_clip(sk, 25, 4, scale=FS.SCALE[name])
    fj, fr, _ = fk_rotation_inputs(sk, name, clip)
    lab = FS.value_labels(vals[:24], HALF)
    FS.check_margins(sk, fj[0], lab, 5)
    r64 = FS.clean_clip(sk, fj[0], lab, 5, np.float64, fr[0])[1]
    gate = GATE * np.abs(FS.clean_clip(sk, fj[0], lab, 5, np.float32, fr[0])[1] - r64).max()
    far = np.abs(FS.clean_clip(sk, fj[0], lab, 5, np.float64, fr[0], wrong="q_right")[1] - r64).max() / gate
    print(name, "q_right", f"{far:.3g} gates")
    assert gate > 0 and far >= 100, far


def test_generator_margins_hold_for_every_gpu_case():
    """walk_clip asserts its margins itself; this builds every clip the GPU tests use, here on the CPU."""
    for name in ("t2m", "kit"):
        sk = ref_skel(name)
        FS.parity_case(sk, name)
    sk = ref_skel("t2m")
    j, v = FS.long_clip(sk)
    lab = FS.value_labels(v, HALF)
    assert lab[240:270, 0].all() and not lab[239, 0] and not lab[270, 0]  # one run across frames 255 | 256
    j, v = FS.whole_clip(sk)
    assert FS.value_labels(v, HALF)[:, [0, 2]].all()
    FS.clamped_clip(sk)


def test_check_foot_skate_value_errors():
    P, MF = pkg("postprocess"), pkg("motion_features")
    sk = MF.SKELETONS["t2m"]
    j = torch.zeros(2, 8, 22, 3)
    ok = P.check_foot_skate(j, [8, 3], torch.zeros(2, 8, 4), torch.zeros(2, 8, 22, 3, 3), sk)
    assert ok[0].shape == (2, 8, 22, 3) and ok[3].tolist() == [0.5] * 4 and ok[4] == 0.002
    mean, std = np.zeros(263), np.full(263, 2.0)
    mean[-4:] = 0.25
    thre = P.check_foot_skate(j, None, (torch.zeros(2, 8, 263), mean, std), None, sk)[3]
    assert thre.dtype == torch.float32 and thre.tolist() == [0.125] * 4
    assert P.leg_joints(sk) == ((1, 4, 7, 10), (2, 5, 8, 11))
    assert P.leg_joints(MF.SKELETONS["kit"]) == ((17, 18, 19, 20), (12, 13, 14, 15))
    bad = [dict(joints=torch.zeros(2, 8, 21, 3)), dict(joints=torch.zeros(2, 0, 22, 3)), dict(lengths=[8]), dict(lengths=[8, 0]),
           dict(lengths=[8, 9]), dict(contacts=torch.zeros(2, 8, 3)), dict(contacts=torch.zeros(2, 7, 4)),
           dict(contacts=(torch.zeros(2, 8, 251), mean, std)), dict(contacts=(torch.zeros(2, 8, 263), mean[:10], std)),
           dict(contacts=(torch.zeros(2, 8, 263), mean, np.zeros(263))), dict(contacts=(torch.zeros(2, 8, 263), mean)),
           dict(rotations=torch.zeros(2, 8, 22, 3)), dict(blend=-1), dict(blend=1.5), dict(feet_thre=-1.0),
           dict(contacts=torch.zeros(2, 8, 4), contact_thre=float("nan")),
           dict(joints=torch.zeros(1, P.foot_skate_max_frames() + 1, 22, 3), lengths=None)]
    for kw in bad:
        args = dict(joints=j, lengths=[8, 3], contacts=None, rotations=None, sk=sk)
        args.update(kw)
        with pytest.raises(ValueError):
            P.check_foot_skate(**args)
    import copy
    odd = copy.copy(sk)
    odd.feet = (sk.feet[1], sk.feet[0], sk.feet[2], sk.feet[3])  # toe and ankle swapped: no such leg
    with pytest.raises(ValueError, match="chain"):
        P.check_foot_skate(j, None, None, None, odd)
    assert P.foot_skate_max_frames() >= pkg("trainer").MAX_JOINTS_FRAMES

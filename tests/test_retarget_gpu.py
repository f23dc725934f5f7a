"""GPU: rig retargeting (mdm_retarget_channels): joints, rotations and offsets -> the channels of a given
hierarchy -> BVH text on that hierarchy, read back by the text-only BVH reader of tests/rig_ref.py.

* the four cases of tests/golden/motion_fk.npz (through motion_to_joints_fk on the rows, sigma 0, on the golden file's offsets
  with left and right evened, tests/retarget_ref.even_offsets) on the synthetic targets of tests/retarget_ref.py, every Euler
  order on one of them, with and without leg IK: the joints and the global matrices that the reader rebuilds, the globals
  output, and the properties (bone directions, the root, the ankles);
* retiming 20 -> 30 and 20 -> 10; lengths: zeros past length_out, nothing past a length is read, every sample equals its run
  alone, num = den and ::2 bit for bit;
* the same rest pose copies the rotations; the written files come back through bvh_to_joints; after the foot-skate clean-up;
  through the trainer.

Tolerances.  GATE = 4 x a yardstick, the project's convention (§19): the yardstick of a case is how far the all-fp32 restatement's
file (tests/retarget_ref.py) reads back from the fp64 restatement's, on the same inputs and over the whole batch, for joints and
for global matrices separately; both texts are read by the same fp64 reader.  Nothing is gated against the kernel's output.
A unit direction is a difference of two read-back positions over a bone's length: its gate is twice the joints' over the
target's shortest copied bone.  tests/test_retarget_host.py shows that each of seven mistakes lies >= 100 gates away.
"""
import functools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, pkg

import retarget_ref as TR
import rig_ref as RR
from test_retarget_host import GATE, LENS, properties, target

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def fk(name):
    """A golden case through motion_to_joints_fk: (skeleton, raw rest axes, joints, rotations, offsets on the device; read-only)."""
    z = np.load(os.path.join(GOLDEN, "motion_fk.npz"))
    skel = name.split("_")[0]
    j, r, o = pkg("postprocess").motion_to_joints_fk(
        torch.from_numpy(z[f"{name}_rows"]).cuda(), z[f"{skel}_mean"], z[f"{skel}_std"], LENS,
        torch.from_numpy(TR.even_offsets(skel, z[f"{skel}_offsets"]).astype(np.float32)), skeleton=skel, sigma=0.0,
        return_rotations=True, return_offsets=True)
    return skel, pkg("motion_features").get_skeleton(skel).raw_offsets, j, r, o


@functools.lru_cache(maxsize=None)
def fixed(name):
    """``fk(name)`` after the foot-skate clean-up."""
    z = np.load(os.path.join(GOLDEN, "motion_fk.npz"))
    skel, raw, j, r, o = fk(name)
    rows = torch.from_numpy(z[f"{name}_rows"]).cuda()
    j2, r2 = pkg("postprocess").remove_foot_skate(j, LENS, (rows, z[f"{skel}_mean"], z[f"{skel}_std"]), rotations=r)
    return skel, raw, j2, r2, o


@functools.lru_cache(maxsize=None)
def truth_of(key, name, order="ZXY", num=1, den=1, leg_ik=False, clean=False):
    skel, raw, j, r, o = (fixed if clean else fk)(name)
    return TR.yardstick(pkg("motion_rig"), target(key, skel)[0], raw, j.cpu().numpy(), r.cpu().numpy(), o.cpu().numpy(), LENS,
                        order, num, den, leg_ik)


def read_channels(tg, chan, lens_out, order="ZXY"):
    MRig = pkg("motion_rig")
    chan = chan.cpu()
    return [TR.read_back(MRig.target_bvh_text(tg, chan[b], int(n), 0.05, euler=order), tg) for b, n in enumerate(lens_out)]


def worst(got, want):
    return (max(float(np.abs(g[0] - w[0]).max()) for g, w in zip(got, want)),
            max(float(np.abs(g[2] - w[2]).max()) for g, w in zip(got, want)))


def shortest_bone(tg):
    return min(float(np.linalg.norm(tg.joint_rest[tg.src[n]] - tg.rest[n])) for n in range(tg.n_nodes) if tg.kind[n] == 1)


CASES = [("b", "t2m_noisy", o) for o in RR.ORDERS] + [(k, "t2m_noisy", "ZXY") for k in "acdef"] + \
        [("b", "t2m_clean", "ZXY"), ("a", "kit_clean", "ZXY"), ("a", "kit_noisy", "ZXY")]


@pytest.mark.parametrize("key,name,order", CASES)
def test_channels_of_the_golden_cases(key, name, order):
    MRig = pkg("motion_rig")
    skel, raw, j, r, o = fk(name)
    tg, _ = target(key, skel)
    N = tg.n_nodes
    for leg_ik in (False, True):
        truth, yj, yg = truth_of(key, name, order, 1, 1, leg_ik)
        chan, lens_out, glob = MRig.retarget_to_rig(j, r, LENS, tg, offsets=o, skeleton=skel, euler=order, leg_ik=leg_ik,
                                                    return_globals=True)
        assert chan.shape == (3, 24, 3 + 3 * N) and glob.shape == (3, 24, N, 3, 3) and lens_out.tolist() == LENS
        got = read_channels(tg, chan, LENS, order)
        ej, eg = worst(got, truth)
        # the globals output at the source frames is what the reader rebuilds (no retiming here)
        eo = max(float(np.abs(glob[b, :n].cpu().numpy() - truth[b][2]).max()) for b, n in enumerate(LENS))
        e_dir, e_root, e_ank, out, total, side = properties(tg, skel, j.cpu().numpy().astype(np.float64), o.cpu().numpy(), got,
                                                            GATE * yj, leg_ik)
        print(key, name, order, "leg_ik", leg_ik, f"joints {ej:.3g} (yardstick {yj:.3g})  globals {eg:.3g} / output {eo:.3g} "
              f"(yardstick {yg:.3g})  direction {e_dir:.3g} root {e_root:.3g} ankle {e_ank:.3g} unreachable {out}/{total} "
              f"knee side {side:.3g}")
        assert ej <= GATE * yj and eg <= GATE * yg and eo <= GATE * yg, (ej, yj, eg, eo, yg)
        assert e_dir <= 2 * GATE * yj / shortest_bone(tg) and e_root <= GATE * yj, (e_dir, e_root, yj)
        if leg_ik:
            assert e_ank <= GATE * yj and side > 0, (e_ank, yj, side)
        elif key != "a":
            assert e_ank > 100 * GATE * yj, (e_ank, yj)
    default, _ = MRig.retarget_to_rig(j, r, LENS, tg, offsets=o, skeleton=skel, euler=order)
    assert tg.leg_ok and torch.equal(default, chan)                    # leg IK is the default where the legs are mapped


@pytest.mark.parametrize("key", ["b", "d"])
def test_retiming(key):
    MRig = pkg("motion_rig")
    skel, raw, j, r, o = fk("t2m_noisy")
    tg, _ = target(key)
    chan, lens_out = MRig.retarget_to_rig(j, r, LENS, tg, offsets=o)
    for kw in (dict(fps_out=20), dict(fps=30, fps_out=30.0)):
        same, m = MRig.retarget_to_rig(j, r, LENS, tg, offsets=o, **kw)
        assert torch.equal(same, chan) and m.tolist() == LENS, kw       # num = den: the frames themselves
    half, m = MRig.retarget_to_rig(j, r, LENS, tg, offsets=o, fps_out=10)
    assert m.tolist() == [12, 1, 1] and half.shape[1] == 12
    for b, n in enumerate(m.tolist()):
        assert torch.equal(half[b, :n], chan[b, ::2][:n]) and not half[b, n:].any()
    x = j.cpu().numpy().astype(np.float64)
    for fps_out, num, den in ((30, 3, 2), (10, 1, 2)):
        truth, yj, yg = truth_of(key, "t2m_noisy", "ZXY", num, den, True)
        out, m = MRig.retarget_to_rig(j, r, LENS, tg, offsets=o, fps_out=fps_out)
        assert m.tolist() == [(n - 1) * num // den + 1 for n in LENS] and out.shape[1] == max(m.tolist())
        got = read_channels(tg, out, m.tolist())
        ej, eg = worst(got, truth)
        # the properties hold on the output frames that are source frames (between two of them a slerp stands)
        whole = [[k for k in range(n) if k * den % num == 0] for n in m.tolist()]
        at = [[k * den // num for k in ks] for ks in whole]
        sub = [tuple(a[ks] for a in g) for g, ks in zip(got, whole)]
        e_dir, e_root, e_ank, _, _, side = properties(tg, "t2m", x, o.cpu().numpy(), sub, GATE * yj, True, frames=at)
        print(key, "20 ->", fps_out, f"joints {ej:.3g} (yardstick {yj:.3g})  globals {eg:.3g} (yardstick {yg:.3g})  direction "
              f"{e_dir:.3g} root {e_root:.3g} ankle {e_ank:.3g}")
        assert ej <= GATE * yj and eg <= GATE * yg, (fps_out, ej, yj, eg, yg)
        assert e_dir <= 2 * GATE * yj / shortest_bone(tg) and e_root <= GATE * yj and e_ank <= GATE * yj and side > 0


def test_lengths():
    MRig = pkg("motion_rig")
    skel, raw, j, r, o = fk("t2m_noisy")
    tg, _ = target("b")
    for fps_out in (None, 30):
        chan, lens_out, glob = MRig.retarget_to_rig(j, r, LENS, tg, offsets=o, fps_out=fps_out, return_globals=True)
        assert chan.shape[1] == int(lens_out.max()) and bool(torch.isfinite(chan).all()) and bool(torch.isfinite(glob).all())
        jn, rn = j.clone(), r.clone()
        for b, n in enumerate(LENS):
            jn[b, n:], rn[b, n:] = float("nan"), float("nan")
        chan2, _, glob2 = MRig.retarget_to_rig(jn, rn, LENS, tg, offsets=o, fps_out=fps_out, return_globals=True)
        assert torch.equal(chan2, chan) and torch.equal(glob2, glob)                       # nothing past a length is read
        for b, (n, m) in enumerate(zip(LENS, lens_out.tolist())):
            assert not chan[b, m:].any() and not glob[b, n:].any()                          # zeros past the lengths
            one, m1, g1 = MRig.retarget_to_rig(j[b:b + 1, :n], r[b:b + 1, :n], None, tg, offsets=o[b:b + 1], fps_out=fps_out,
                                               return_globals=True)
            assert m1.tolist() == [m] and one.shape == (1, m, chan.shape[2])               # T = 1 among them
            assert torch.equal(one[0], chan[b, :m]) and torch.equal(g1[0], glob[b, :n]), (fps_out, b)


def test_the_same_rest_pose_copies_the_rotations():
    MRig = pkg("motion_rig")
    skel, raw, j, r, o = fk("t2m_noisy")
    tg, _ = target("a2")
    _, _, yg = truth_of("a2", "t2m_noisy")
    _, _, glob = MRig.retarget_to_rig(j, r, LENS, tg, offsets=o, leg_ik=False, return_globals=True)
    worst_g = 0.0
    for b, n in enumerate(LENS):
        for node in range(tg.n_nodes):
            res = tg.res[node]
            if res >= 0 and tg.kind[res] == 1:
                worst_g = max(worst_g, float((glob[b, :n, node] - r[b, :n, tg.src[res]]).abs().max()))
    print(f"globals against R[jc] {worst_g:.3g} (yardstick {yg:.3g})")
    assert worst_g <= GATE * yg


@pytest.mark.parametrize("key,up", [("b", "Y"), ("e", "Z")])
def test_the_written_file_comes_back_through_the_import(key, up):
    """bvh_to_joints on the written text gives the joints the text-only reader gives.  Yardstick: the reader run in fp32 on the
    same text against itself in fp64 (the import kernel's arithmetic is fp32)."""
    MRig = pkg("motion_rig")
    skel, raw, j, r, o = fk("t2m_noisy")
    tg, _ = target(key)
    chan, lens_out = MRig.retarget_to_rig(j, r, LENS, tg, offsets=o)
    texts = [MRig.target_bvh_text(tg, chan[b].cpu(), n, 0.05) for b, n in enumerate(LENS)]
    back = MRig.bvh_to_joints(texts, joint_map="mixamo", fps_out=None, up=up)
    ej = yj = 0.0
    for b, text in enumerate(texts):
        bvh = RR.parse_bvh(text)
        want = TR.read_back(text, tg)[0] @ tg.basis.T                                      # the importer turns by basis
        p32 = RR.bvh_fk(bvh, np.float32)[0][:, tg.pick].astype(np.float64) @ tg.basis.T
        yj = max(yj, float(np.abs(p32 - want).max()))
        ej = max(ej, float(np.abs(back[b].cpu().numpy() - want).max()))
    print(key, f"round trip joints {ej:.3g} (yardstick {yj:.3g})")
    assert ej <= GATE * yj, (ej, yj)
    # and in our world it is the source on the target's proportions: the root path is s x[0]
    s = TR.scale_of(tg, o[0].cpu().numpy().astype(np.float64))
    assert float(np.abs(back[0][:, 0].cpu().numpy() - s * j[0, :, 0].cpu().numpy()).max()) <= GATE * (yj + truth_of(key, "t2m_noisy", leg_ik=True)[1])


def test_after_the_foot_skate_clean_up():
    MRig = pkg("motion_rig")
    skel, raw, j2, r2, o = fixed("t2m_noisy")
    assert not torch.equal(j2, fk("t2m_noisy")[2])
    tg, _ = target("b")
    truth, yj, yg = truth_of("b", "t2m_noisy", leg_ik=True, clean=True)
    chan, _ = MRig.retarget_to_rig(j2, r2, LENS, tg, offsets=o)
    got = read_channels(tg, chan, LENS)
    ej, eg = worst(got, truth)
    e_dir, e_root, e_ank, out, total, side = properties(tg, skel, j2.cpu().numpy().astype(np.float64), o.cpu().numpy(), got,
                                                        GATE * yj, True)
    print(f"cleaned: joints {ej:.3g} (yardstick {yj:.3g})  globals {eg:.3g} (yardstick {yg:.3g})  ankle {e_ank:.3g} "
          f"unreachable {out}/{total}")
    assert ej <= GATE * yj and eg <= GATE * yg and e_ank <= GATE * yj and side > 0


def test_through_the_trainer(tmp_path):
    import test_motion_features_gpu as TF
    import test_motion_fk_gpu as TK
    MRig = pkg("motion_rig")
    tr = TF._tiny_trainer()
    tg, text_b = target("b")
    mean, std = TK._mean_std(263, 22, 12)
    caps, lens = ["a", "b", "c", "d"], [16, 16, 12, 9]   # batches of two: the denoiser takes even T
    opts = dict(seed=0, sampler="ddim", sample_steps=5, batch_size=2, fix_feet=True)
    path = str(tmp_path / "a.bvh")
    texts = tr.generate_bvh(caps, torch.tensor(lens), 263, mean, std, fps_out=30, paths=[path, None, None, None],
                            target_rig=text_b, target_joint_map="mixamo", **opts)
    res = tr.generate_rotations(caps, torch.tensor(lens), 263, mean, std, **opts)
    assert len(texts) == 4 and open(path).read() == texts[0]
    for i, n in enumerate(lens):
        jo, ro, of = res[i]
        chan, m = MRig.retarget_to_rig(jo[None], ro[None], None, tg, offsets=of, fps_out=30)
        assert texts[i] == MRig.target_bvh_text(tg, chan[0].cpu(), int(m[0]), 1 / 30)      # the hand-made pipeline's text
        bvh = RR.parse_bvh(texts[i], np.float32)
        assert bvh.names == tg.names and bvh.frames == (n - 1) * 3 // 2 + 1 and abs(bvh.frame_time - 1 / 30) < 1e-9
    no_ik = tr.generate_bvh(caps[:2], torch.tensor(lens[:2]), 263, mean, std, target_rig=tg, leg_ik=False, euler="XYZ", **opts)
    chan, m = MRig.retarget_to_rig(res[0][0][None], res[0][1][None], None, tg, offsets=res[0][2], leg_ik=False, euler="XYZ")
    assert no_ik[0] == MRig.target_bvh_text(tg, chan[0].cpu(), 16, 0.05, euler="XYZ") and no_ik[0] != texts[0]
    with pytest.raises(ValueError, match="scale"):
        tr.generate_bvh(caps, torch.tensor(lens), 263, mean, std, target_rig=text_b, scale=100.0, **opts)
    # a long motion
    scripts = [[("a", 16), ("b", 16)]]
    lopts = dict(overlap=4, seed=4, sampler="ddim", sample_steps=5)
    (text,) = tr.generate_long_bvh(scripts, 263, mean, std, fps_out=30, target_rig=text_b, **lopts)
    bvh = RR.parse_bvh(text, np.float32)
    assert bvh.names == tg.names and bvh.frames == (28 - 1) * 3 // 2 + 1
    (plain,) = tr.generate_long_bvh(scripts, 263, mean, std, fps_out=30, **lopts)
    own = RR.parse_bvh(plain, np.float32)
    shared = [k for k in range(bvh.frames) if k * 2 % 3 == 0]
    # the same motion on the other character: the root path is the plain export's, rescaled (one s for the whole clip)
    ours, theirs = bvh.values[shared, :3].astype(np.float64), own.values[shared, :3].astype(np.float64)
    s_fit = float((ours * theirs).sum() / (theirs * theirs).sum())
    assert own.names == MRig.rig_of("t2m").names and s_fit > 0
    assert np.abs(ours - s_fit * theirs).max() <= 1e-5 * np.abs(ours).max()


def test_bad_arguments_on_the_device_path():
    MRig, L = pkg("motion_rig"), pkg("_lib")
    tg, _ = target("b")
    j, r, o = torch.zeros(2, 8, 22, 3, device="cuda"), torch.zeros(2, 8, 22, 3, 3, device="cuda"), torch.ones(22, 3)
    with pytest.raises(ValueError):
        MRig.retarget_to_rig(j, r, [8, 9], tg, offsets=o)
    with pytest.raises(ValueError):
        MRig.retarget_to_rig(j, r, None, tg, offsets=o, skeleton="kit")
    for a, b in ((j, r.cpu()), (j.cpu(), r), (j.cpu(), r.cpu())):
        with pytest.raises(L.MdmError):
            MRig.retarget_to_rig(a, b, None, tg, offsets=o)                                # no eager fallback

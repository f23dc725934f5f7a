"""GPU: rig export (mdm_rig_channels): rotations -> rig channels -> BVH text, read back by a BVH reader.

* the four cases of tests/golden/motion_fk.npz (joints and rotations from motion_to_joints_fk on the rows, sigma 0, the shared
  offsets): the joints and the global matrices that the reader rebuilds from the exported text, and the local quaternions;
* lengths: zeros past length_out, nothing past a length is read, every sample equals its run alone, T = 1;
* retiming: 1 / 1 and 20 -> 10 bit for bit, 20 -> 30 and 20 -> 60 against the fp64 slerp, a constant-angular-velocity clip
  against its analytic rotations;
* after the foot-skate clean-up the text gives the pinned joints; through the trainer: generate_bvh, generate_long_bvh.

Tolerances.  GATE = 4 x a yardstick, as tests/test_motion_fk_gpu.py has it: the yardstick of a case is how far the all-fp32
restatement (tests/rig_ref.py) lies from what the case compares with, on the same inputs and over the whole batch, measured for
the rebuilt joints and for the rebuilt global matrices separately; both texts are read by the same fp64 reader.  What a case
compares with is the fp64 restatement, but for the analytic clip (its analytic local rotations) and the foot-skate case (the
pinned joints themselves, which close over their rotations only to fp32).  Nothing is gated against the kernel's output.
tests/test_motion_rig_host.py shows that each of six mistakes lies >= 1e4 gates away.
"""
import functools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, pkg

import rig_ref as RR

pytestmark = pytest.mark.gpu

GATE = 4.0
LENS = [24, 2, 1]
CASES = [("t2m_noisy", o) for o in RR.ORDERS] + [(c, "ZXY") for c in ("t2m_clean", "kit_clean", "kit_noisy")]


@functools.lru_cache(maxsize=None)
def fk(name):
    """A golden case through motion_to_joints_fk: (skeleton, offsets fp32, joints, rotations on the device; read-only)."""
    z = np.load(os.path.join(GOLDEN, "motion_fk.npz"))
    skel = name.split("_")[0]
    off = z[f"{skel}_offsets"]
    j, r = pkg("postprocess").motion_to_joints_fk(torch.from_numpy(z[f"{name}_rows"]).cuda(), z[f"{skel}_mean"], z[f"{skel}_std"],
                                                  LENS, torch.from_numpy(off), skeleton=skel, sigma=0.0, return_rotations=True)
    return skel, off, j, r


@functools.lru_cache(maxsize=None)
def truth_of(name, order="ZXY", num=1, den=1):
    """-> (per sample the fp64 restatement's (joints, globals) read back from its text, yardstick joints, yardstick globals)."""
    skel, off, j, r = fk(name)
    MRig = pkg("motion_rig")
    return RR.yardstick(MRig.bvh_text, MRig.rig_of(skel), off, j.cpu().numpy(), r.cpu().numpy(), LENS, order, 1.0, num, den)


def read_channels(rig, off, chan, lens_out, order="ZXY", scale=1.0):
    """Device channels (B, T_out, C) -> per sample (joints, globals) that the fp64 reader rebuilds from the exported text."""
    MRig = pkg("motion_rig")
    chan = chan.cpu()
    return [RR.read_back(MRig.bvh_text(rig, off, chan[b], int(n), 0.05, euler=order, scale=scale), rig)
            for b, n in enumerate(lens_out)]


def worst(got, want):
    return (max(float(np.abs(g[0] - w[0]).max()) for g, w in zip(got, want)),
            max(float(np.abs(g[1] - w[1]).max()) for g, w in zip(got, want)))


@pytest.mark.parametrize("name,order", CASES)
def test_channels_of_the_golden_cases(name, order):
    MRig = pkg("motion_rig")
    skel, off, j, r = fk(name)
    rig = MRig.rig_of(skel)
    truth, yj, yg = truth_of(name, order)
    chan, lens_out, quat = MRig.rotations_to_rig(j, r, LENS, skeleton=skel, euler=order, return_quaternions=True)
    N = rig.n_nodes
    assert chan.shape == (3, 24, 3 + 3 * N) and quat.shape == (3, 24, N, 4) and lens_out.tolist() == LENS
    ej, eg = worst(read_channels(rig, off, chan, LENS, order), truth)
    print(name, order, f"joints {ej:.3g} (yardstick {yj:.3g})  globals {eg:.3g} (yardstick {yg:.3g})")
    assert ej <= GATE * yj and eg <= GATE * yg, (ej, yj, eg, yg)
    # the local quaternions: unit to 4 ulp, canonical, and down the tree they give the same global matrices
    q = quat.cpu().numpy().astype(np.float64)
    eq = 0.0
    for b, n in enumerate(LENS):
        assert np.abs(np.linalg.norm(q[b, :n], axis=-1) - 1).max() <= 4 * np.finfo(np.float32).eps and (q[b, :n, :, 0] >= 0).all()
        L, G = RR.quaternion_to_matrix(q[b, :n]), [None] * N
        for node, p in enumerate(rig.parent):
            G[node] = L[:, node] if p < 0 else G[p] @ L[:, node]
        eq = max(eq, float(np.abs(np.stack(G, 1) - truth[b][1]).max()))
    print(name, order, f"globals from the quaternions {eq:.3g}")
    assert eq <= GATE * yg, (eq, yg)


def test_lengths():
    MRig = pkg("motion_rig")
    skel, off, j, r = fk("t2m_noisy")
    for fps_out in (None, 30):
        chan, lens_out, quat = MRig.rotations_to_rig(j, r, LENS, fps_out=fps_out, return_quaternions=True)
        assert chan.shape[1] == int(lens_out.max()) and bool(torch.isfinite(chan).all())
        jn, rn = j.clone(), r.clone()
        for b, n in enumerate(LENS):
            jn[b, n:], rn[b, n:] = float("nan"), float("nan")
        chan2, _, quat2 = MRig.rotations_to_rig(jn, rn, LENS, fps_out=fps_out, return_quaternions=True)
        assert torch.equal(chan2, chan) and torch.equal(quat2, quat)                      # nothing past a length is read
        for b, (n, m) in enumerate(zip(LENS, lens_out.tolist())):
            assert not chan[b, m:].any() and not quat[b, m:].any()                         # zeros past length_out
            one, m1, q1 = MRig.rotations_to_rig(j[b:b + 1, :n], r[b:b + 1, :n], None, fps_out=fps_out, return_quaternions=True)
            assert m1.tolist() == [m] and one.shape == (1, m, chan.shape[2])              # T = 1 among them
            assert torch.equal(one[0], chan[b, :m]) and torch.equal(q1[0], quat[b, :m]), (fps_out, b)


def test_retiming():
    MRig = pkg("motion_rig")
    skel, off, j, r = fk("t2m_clean")
    rig = MRig.rig_of(skel)
    chan, lens_out = MRig.rotations_to_rig(j, r, LENS)
    for kw in (dict(fps_out=20), dict(fps=30, fps_out=30.0), dict(fps=12.5, fps_out=12.5)):
        same, m = MRig.rotations_to_rig(j, r, LENS, **kw)
        assert torch.equal(same, chan) and m.tolist() == LENS, kw
    half, m = MRig.rotations_to_rig(j, r, LENS, fps_out=10)
    assert m.tolist() == [12, 1, 1] and half.shape[1] == 12
    for b, n in enumerate(m.tolist()):
        assert torch.equal(half[b, :n], chan[b, ::2][:n]) and not half[b, n:].any()
    for fps_out, num, den in ((30, 3, 2), (60, 3, 1)):
        fr = {(k * den % num, num) for k in range((24 - 1) * num // den + 1)}
        assert {(1, 3), (2, 3)} <= fr                                                      # fractions 1/3 and 2/3 occur
        truth, yj, yg = truth_of("t2m_clean", "ZXY", num, den)
        out, m = MRig.rotations_to_rig(j, r, LENS, fps_out=fps_out)
        assert m.tolist() == [(n - 1) * num // den + 1 for n in LENS] and out.shape[1] == max(m.tolist())
        ej, eg = worst(read_channels(rig, off, out, m.tolist()), truth)
        print("20 ->", fps_out, f"joints {ej:.3g} (yardstick {yj:.3g})  globals {eg:.3g} (yardstick {yg:.3g})")
        assert ej <= GATE * yj and eg <= GATE * yg, (fps_out, ej, yj, eg, yg)


def test_constant_angular_velocity_clip():
    """One axis and one rate per node, the right shoulder passing 180 degrees: at 20 -> 60 the local rotations rebuilt from the
    channels are the analytic ones.  Yardstick: the fp32 restatement on the same fp32 inputs against the analytic rotations."""
    MRig = pkg("motion_rig")
    off = np.load(os.path.join(GOLDEN, "motion_fk.npz"))["t2m_offsets"]
    rig = MRig.rig_of("t2m")
    T = 8
    j, R, local_at = RR.spin_clip(rig, off, T, 3, turning=rig.names.index("right_shoulder"))
    j32, R32 = j.astype(np.float32), R.astype(np.float32)
    K = (T - 1) * 3 + 1
    want = np.stack([local_at(k / 3)[0] for k in range(K)])
    root = np.stack([local_at(k / 3)[1] for k in range(K)])

    def rebuilt(chan):
        chan = np.asarray(chan, np.float64)
        return RR.euler_to_matrix(np.deg2rad(chan[:, 3:].reshape(K, rig.n_nodes, 3)), "ZXY"), chan[:, :3]

    ref = rebuilt(RR.rig_channels(rig, j32, R32, num=3, den=1, dtype=np.float32)[0])
    yl, yp = float(np.abs(ref[0] - want).max()), float(np.abs(ref[1] - root).max())
    out, m = MRig.rotations_to_rig(torch.from_numpy(j32).cuda()[None], torch.from_numpy(R32).cuda()[None], None, fps_out=60)
    assert m.tolist() == [K]
    got = rebuilt(out[0].cpu().numpy())
    el, ep = float(np.abs(got[0] - want).max()), float(np.abs(got[1] - root).max())
    print(f"analytic clip: local rotations {el:.3g} (yardstick {yl:.3g})  root {ep:.3g} (yardstick {yp:.3g})")
    assert el <= GATE * yl and ep <= GATE * yp, (el, yl, ep, yp)


def test_after_the_foot_skate_clean_up():
    """The reader's joints from the exported text are the pinned joints.  Yardstick: the fp32 restatement's text on the pinned
    joints and turned rotations, against those joints."""
    MRig, P = pkg("motion_rig"), pkg("postprocess")
    z = np.load(os.path.join(GOLDEN, "motion_fk.npz"))
    skel, off, j, r = fk("t2m_noisy")
    rig = MRig.rig_of(skel)
    rows = torch.from_numpy(z["t2m_noisy_rows"]).cuda()
    j2, r2 = P.remove_foot_skate(j, LENS, (rows, z["t2m_mean"], z["t2m_std"]), rotations=r)
    assert not torch.equal(j2, j)
    pinned, turned = j2.cpu().numpy(), r2.cpu().numpy()
    yj = 0.0
    for b, n in enumerate(LENS):
        c32 = RR.rig_channels(rig, pinned[b, :n], turned[b, :n], dtype=np.float32)[0]
        yj = max(yj, float(np.abs(RR.read_back(MRig.bvh_text(rig, off, c32, n, 0.05), rig)[0] - pinned[b, :n]).max()))
    chan, m = MRig.rotations_to_rig(j2, r2, LENS)
    got = read_channels(rig, off, chan, LENS)
    ej = max(float(np.abs(got[b][0] - pinned[b, :n]).max()) for b, n in enumerate(LENS))
    print(f"pinned joints {ej:.3g} (yardstick {yj:.3g})")
    assert ej <= GATE * yj, (ej, yj)


def test_through_the_trainer(tmp_path):
    import test_motion_features_gpu as TF
    import test_motion_fk_gpu as TK
    MRig = pkg("motion_rig")
    tr = TF._tiny_trainer()
    rig = MRig.rig_of("t2m")
    mean, std = TK._mean_std(263, 22, 12)
    caps, lens = ["a", "b", "c", "d"], [16, 16, 12, 9]   # batches of two: the denoiser takes even T
    opts = dict(seed=0, sampler="ddim", sample_steps=5, batch_size=2, fix_feet=True)
    paths = [str(tmp_path / "a.bvh"), None, str(tmp_path / "c.bvh"), None]
    texts = tr.generate_bvh(caps, torch.tensor(lens), 263, mean, std, fps_out=30, paths=paths, **opts)
    res = tr.generate_rotations(caps, torch.tensor(lens), 263, mean, std, **opts)
    assert len(texts) == 4 and sorted(os.listdir(tmp_path)) == ["a.bvh", "c.bvh"] and open(paths[0]).read() == texts[0] and open(paths[2]).read() == texts[2]
    for i, n in enumerate(lens):
        jo, ro, of = (t.cpu().numpy() for t in res[i])
        bvh = RR.parse_bvh(texts[i], np.float32)
        m = (n - 1) * 3 // 2 + 1
        assert bvh.frames == m and abs(bvh.frame_time - 1 / 30) < 1e-9 and bvh.names == rig.names
        shared = [k for k in range(m) if k * 2 % 3 == 0]
        assert np.array_equal(bvh.values[shared, :3], jo[[k * 2 // 3 for k in shared], 0])   # the root path, to the bit
        truth, yj, yg = RR.yardstick(MRig.bvh_text, rig, of, [jo], [ro], [n], num=3, den=2)
        got = RR.read_back(texts[i], rig)
        ej, eg = worst([got], truth)
        print("generate_bvh", i, f"joints {ej:.3g} (yardstick {yj:.3g})  globals {eg:.3g} (yardstick {yg:.3g})")
        assert ej <= GATE * yj and eg <= GATE * yg, (i, ej, yj, eg, yg)
    # without retiming and in centimetres: the frame count is the length, positions and offsets carry the scale
    cm = tr.generate_bvh(caps, torch.tensor(lens), 263, mean, std, scale=100.0, euler="XYZ", **opts)
    b0, b1 = RR.parse_bvh(cm[0], np.float32), RR.parse_bvh(texts[0], np.float32)
    assert b0.frames == 16 and b0.frame_time == 0.05 and b0.channels[1] == ["Xrotation", "Yrotation", "Zrotation"]
    assert np.array_equal(b0.values[:, :3], np.float32(100.0) * res[0][0][:, 0].cpu().numpy())
    assert np.abs(b0.offsets - 100.0 * b1.offsets).max() <= 1e-4
    # a long motion
    scripts = [[("a", 16), ("b", 16)]]
    lopts = dict(overlap=4, seed=4, sampler="ddim", sample_steps=5)
    path = str(tmp_path / "long.bvh")
    (text,) = tr.generate_long_bvh(scripts, 263, mean, std, fps_out=30, paths=[path], **lopts)
    bvh = RR.parse_bvh(text, np.float32)
    assert bvh.frames == (28 - 1) * 3 // 2 + 1 and open(path).read() == text
    (jl,) = tr.generate_long_joints(scripts, 263, mean, std, sigma=0.0, from_rotations=True, **lopts)
    shared = [k for k in range(bvh.frames) if k * 2 % 3 == 0]
    assert np.array_equal(bvh.values[shared, :3], jl[[k * 2 // 3 for k in shared], 0].cpu().numpy())
    with pytest.raises(ValueError):
        tr.generate_bvh(caps, torch.tensor(lens), 263, mean, std, paths=paths[:2], **opts)


def test_bad_arguments_on_the_device_path():
    MRig, L = pkg("motion_rig"), pkg("_lib")
    j, r = torch.zeros(2, 8, 22, 3, device="cuda"), torch.zeros(2, 8, 22, 3, 3, device="cuda")
    with pytest.raises(ValueError):
        MRig.rotations_to_rig(j, r, skeleton="kit")
    with pytest.raises(ValueError):
        MRig.rotations_to_rig(j, r, [8, 9])
    for a, b in ((j, r.cpu()), (j.cpu(), r), (j.cpu(), r.cpu())):
        with pytest.raises(L.MdmError):
            MRig.rotations_to_rig(a, b)                                        # no eager fallback

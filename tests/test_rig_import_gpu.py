"""GPU: rig import (mdm_rig_joints): BVH files -> joints at the picked nodes -> feature rows -> the trainer.

The files are written by tests/rig_import_ref.py from tests/golden/motion_fk.npz (B = 3, lengths 24 / 2 / 1): (a) our own
export, (b) the CMU-like file, (c) a single chain of 128 nodes; and a file on the CMU files' own hierarchy (zero offsets at Neck
and the Shoulder nodes), where the preset puts the head at an End Site.

Tolerances.  GATE = 4 x a yardstick, as tests/test_motion_rig_gpu.py has it: the yardstick of a case is how far the all-fp32
restatement (tests/rig_import_ref.py) lies from what the case compares with, on the same files and over the whole batch.  What
a case compares with is the fp64 restatement, but for the analytic clip (its analytic rotations through fp64 forward
kinematics) and the round trip with the exporter (the joints that went in).  Nothing is gated against the kernel's output.
tests/test_rig_import_host.py shows that each of eight mistakes lies >= 100 gates away.
"""
import functools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, pkg

import rig_import_ref as IR
import rig_ref as RR

pytestmark = pytest.mark.gpu

GATE = 4.0
LENS = [24, 2, 1]
AT = np.cumsum([0] + LENS)
CHAIN_PICK = ["n000", "n001", "n064", "n127"]


@functools.lru_cache(maxsize=None)
def golden(name="t2m_noisy"):
    z = np.load(os.path.join(GOLDEN, "motion_fk.npz"))
    j, R = z[f"{name}_joints64"], z[f"{name}_rotations64"]
    return z["t2m_offsets"], [j[AT[b]:AT[b] + n] for b, n in enumerate(LENS)], [R[AT[b]:AT[b] + n] for b, n in enumerate(LENS)]


@functools.lru_cache(maxsize=None)
def texts(kind, frame_time=0.05, name="t2m_noisy"):
    """The three samples of a golden case as files of one kind ("own" or "cmu"); read-only."""
    MRig = pkg("motion_rig")
    off, joints, rots = golden(name)
    rig = MRig.rig_of("t2m")
    if kind == "own":
        return tuple(IR.own_export(MRig.bvh_text, rig, off, j, R, frame_time=frame_time) for j, R in zip(joints, rots))
    return tuple(IR.cmu_like(rig, off, j, R, frame_time=frame_time) for j, R in zip(joints, rots))


def own_names():
    rig = pkg("motion_rig").rig_of("t2m")
    return [rig.names[rig.joint_of.index(j)] for j in range(22)]


@functools.lru_cache(maxsize=None)
def truth_of(kind, frame_time=0.05, num=1, den=1, scale=1.0, basis=None, name="t2m_noisy"):
    """-> (the parsed files, their picks, per file the fp64 restatement's joints, the yardstick); read-only."""
    one = {"chain": IR.chain, "cmu_real": IR.cmu_real}.get(kind)
    files = [RR.parse_bvh(t) for t in ((one(),) if one else texts(kind, frame_time, name))]
    names = {"own": own_names(), "cmu": IR.CMU_JOINTS, "cmu_real": IR.CMU_JOINTS, "chain": CHAIN_PICK}[kind]
    picks = [IR.pick_of(f, names) for f in files]
    truth, y = IR.yardstick(files, picks, num=num, den=den, scale=scale, basis=IR.EYE if basis is None else np.array(basis))
    return files, picks, truth, y


def worst(got, want):
    assert [tuple(g.shape) for g in got] == [w.shape for w in want]
    return max(float(np.abs(g.cpu().numpy() - w).max()) for g, w in zip(got, want))


def quaternion_check(q, want, gate, what):
    """Device quaternions (frames, N, 4) against the restatement's fp64 ones, up to sign: unit to 4 ulp, w >= 0, within gate."""
    q = q.cpu().numpy().astype(np.float64)
    want = want[:, :q.shape[1]]                                                   # without the End Sites' nodes
    assert q.shape == want.shape and (q[..., 0] >= 0).all()
    assert np.abs(np.linalg.norm(q, axis=-1) - 1).max() <= 4 * np.finfo(np.float32).eps
    e = float(np.minimum(np.abs(q - want).max(-1), np.abs(q + want).max(-1)).max())
    print(what, f"quaternions {e:.3g} (gate {gate:.3g})")
    assert e <= gate, (what, e, gate)


def quaternion_gate(f, num, den):
    """4 x how far the fp32 restatement's local quaternions lie from the fp64 ones, up to sign; and the fp64 ones."""
    q64 = IR.import_joints(f, [0], num, den, np.float64, force_quaternions=True)[1]
    q32 = IR.import_joints(f, [0], num, den, np.float32, force_quaternions=True)[1].astype(np.float64)
    return GATE * float(np.minimum(np.abs(q32 - q64).max(-1), np.abs(q32 + q64).max(-1)).max()), q64


@pytest.mark.parametrize("kind", ["own", "cmu", "chain", "cmu_real"])
def test_unretimed_import(kind):
    MRig = pkg("motion_rig")
    files, picks, truth, y = truth_of(kind)
    src = {"chain": [IR.chain()], "cmu_real": [IR.cmu_real()]}.get(kind) or list(texts(kind))
    if kind == "cmu_real":                                                        # 120 fps: also read at 20, every sixth frame
        assert torch.equal(MRig.bvh_to_joints(src)[0], MRig.bvh_to_joints(src, fps_out=None)[0][::6])
    got, quat = MRig.bvh_to_joints(src, fps_out=None, joint_map=CHAIN_PICK if kind == "chain" else None, return_quaternions=True)
    e = worst(got, truth)
    print(kind, f"joints {e:.3g} (yardstick {y:.3g})")
    assert e <= GATE * y, (e, y)
    eq = 0.0
    for f, p, q, t in zip(files, picks, quat, truth):
        q = q.cpu().numpy()
        assert q.shape == (f.frames, len(f.names), 4) and (q[..., 0] >= 0).all()
        assert np.abs(np.linalg.norm(q.astype(np.float64), axis=-1) - 1).max() <= 4 * np.finfo(np.float32).eps
        # down the tree in fp64 the quaternions give the same joints (a node that stands for an End Site does not turn)
        _, pos_col = IR.node_channels(f)
        root = np.stack([f.values[:, c] for c in pos_col], -1)
        fe = IR.with_end_sites(f)
        L = np.broadcast_to(np.eye(3), (f.frames, len(fe.names), 3, 3)).copy()
        L[:, :len(f.names)] = RR.quaternion_to_matrix(q.astype(np.float64))
        pos = IR.walk_down(fe.parent, fe.offsets, L, root)
        eq = max(eq, float(np.abs(pos[:, p] - t).max()))
    print(kind, f"joints from the quaternions {eq:.3g}")
    assert eq <= GATE * y, (eq, y)


def test_lengths_and_batching():
    MRig = pkg("motion_rig")
    cmu, own = texts("cmu"), texts("own")
    bvh = MRig.parse_bvh(cmu[0])
    pick = MRig.resolve_joint_map(bvh)
    N = len(bvh.names)
    parsed = [MRig.parse_bvh(t) for t in cmu]
    for num, den in ((1, 1), (3, 2)):
        values = torch.zeros(3, 24, bvh.values.shape[1])
        for b, f in enumerate(parsed):
            values[b, :f.frames] = torch.from_numpy(f.values)
        out, n_out, quat = MRig.rig_joints(values.cuda(), LENS, bvh, pick, num, den, return_quaternions=True)
        assert n_out.tolist() == [(n - 1) * num // den + 1 for n in LENS] and out.shape == (3, int(n_out.max()), 22, 3)
        assert quat.shape == (3, int(n_out.max()), N, 4) and bool(torch.isfinite(out).all())
        planted = values.clone()
        for b, n in enumerate(LENS):
            planted[b, n:] = float("nan")
        out2, _, quat2 = MRig.rig_joints(planted.cuda(), LENS, bvh, pick, num, den, return_quaternions=True)
        assert torch.equal(out2, out) and torch.equal(quat2, quat)                          # nothing past a length is read
        for b, (n, m) in enumerate(zip(LENS, n_out.tolist())):
            assert not out[b, m:].any() and not quat[b, m:].any()                            # zeros past length_out
            one, m1, q1 = MRig.rig_joints(values[b:b + 1, :n].cuda(), None, bvh, pick, num, den, return_quaternions=True)
            assert m1.tolist() == [m] and one.shape == (1, m, 22, 3)                         # T = 1 among them
            assert torch.equal(one[0], out[b, :m]) and torch.equal(q1[0], quat[b, :m]), (num, den, b)
    # the batched call is the files' own runs, and files with different hierarchies come back in order
    mixed = [cmu[0], own[1], cmu[2], own[0], cmu[1]]
    got = MRig.bvh_to_joints(mixed, fps_out=30)
    alone = [MRig.bvh_to_joints([t], fps_out=30)[0] for t in mixed]
    assert [tuple(g.shape) for g in got] == [(35, 22, 3), (2, 22, 3), (1, 22, 3), (35, 22, 3), (2, 22, 3)]
    assert all(torch.equal(g, a) for g, a in zip(got, alone))
    single = MRig.bvh_to_joints([cmu[2]])                                                    # a single-frame file
    assert single[0].shape == (1, 22, 3) and worst(single, truth_of("cmu")[2][2:]) <= GATE * truth_of("cmu")[3]


def test_retiming(tmp_path):
    MRig = pkg("motion_rig")
    plain = MRig.bvh_to_joints(list(texts("cmu")), fps_out=None)
    same = MRig.bvh_to_joints(list(texts("cmu")), fps_out=20)                                # a 20 fps file at 20: num == den
    assert all(torch.equal(a, b) for a, b in zip(same, plain))
    paths = []
    for i, t in enumerate(texts("cmu", 1 / 120)):
        paths.append(str(tmp_path / f"{i}.bvh"))
        with open(paths[-1], "w") as f:
            f.write(t)
    sixth = MRig.bvh_to_joints(paths)                                                        # 120 -> 20, from paths
    assert [g.shape[0] for g in sixth] == [4, 1, 1] and all(torch.equal(g, p[::6]) for g, p in zip(sixth, plain))
    # num == den > 1: source time k num / num, no remainder, nothing interpolated
    bvh = MRig.parse_bvh(texts("cmu")[0])
    pick, values = MRig.resolve_joint_map(bvh), torch.from_numpy(bvh.values).cuda()[None]
    a, b = MRig.rig_joints(values, None, bvh, pick, 1, 1, return_quaternions=True), MRig.rig_joints(values, None, bvh, pick, 7, 7, return_quaternions=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and torch.equal(a[0][0], plain[0]) and a[1].tolist() == b[1].tolist() == [24]
    for fps, num, den in ((30, 2, 3), (20, 3, 2)):                                           # 30 -> 20 and 20 -> 30
        fps_out = fps * num / den
        assert {k * den % num for k in range((24 - 1) * num // den + 1)} == set(range(num))  # every fraction occurs
        files, picks, truth, y = truth_of("cmu", 1 / fps, num, den)
        got, quat = MRig.bvh_to_joints(list(texts("cmu", 1 / fps)), fps_out=fps_out, return_quaternions=True)
        assert [g.shape[0] for g in got] == [(n - 1) * num // den + 1 for n in LENS]
        for f, q in zip(files, quat):                                                        # the slerped quaternions
            gate, q64 = quaternion_gate(f, num, den)
            quaternion_check(q, q64, gate, f"{fps} -> {fps_out}")
        e = worst(got, truth)
        print(fps, "->", fps_out, f"joints {e:.3g} (yardstick {y:.3g})")
        assert e <= GATE * y, (fps, e, y)


def test_constant_angular_velocity_clip():
    """rig_ref.spin_clip, one axis and one rate per node and the right shoulder passing 180 degrees, exported at 20 fps and
    imported at 60: the joints are those of the analytic rotations.  Yardstick: the fp32 restatement on the same file."""
    MRig = pkg("motion_rig")
    off = golden()[0]
    rig = MRig.rig_of("t2m")
    T = 8
    j, R, local_at = RR.spin_clip(rig, off, T, 3, turning=rig.names.index("right_shoulder"))
    text = IR.own_export(MRig.bvh_text, rig, off, j, R)
    K = (T - 1) * 3 + 1
    want = IR.analytic_joints(rig, off, local_at, [k / 3 for k in range(K)])
    bvh = RR.parse_bvh(text)
    y = float(np.abs(IR.import_joints(bvh, IR.pick_of(bvh, own_names()), 3, 1, np.float32)[0] - want).max())
    (got,) = MRig.bvh_to_joints([text], fps_out=60)
    e = worst([got], [want])
    print(f"analytic clip: joints {e:.3g} (yardstick {y:.3g})")
    assert e <= GATE * y, (e, y)


@functools.lru_cache(maxsize=None)
def fk(name):
    """A golden case through motion_to_joints_fk, as tests/test_motion_rig_gpu.py has it: (offsets, joints, rotations)."""
    z = np.load(os.path.join(GOLDEN, "motion_fk.npz"))
    off = z["t2m_offsets"]
    j, r = pkg("postprocess").motion_to_joints_fk(torch.from_numpy(z[f"{name}_rows"]).cuda(), z["t2m_mean"], z["t2m_std"], LENS,
                                                  torch.from_numpy(off), skeleton="t2m", sigma=0.0, return_rotations=True)
    return off, j, r


@pytest.mark.parametrize("order,fps_out", [("ZXY", None), ("YZX", None), ("ZXY", 60)])
def test_round_trip_with_the_exporter(order, fps_out):
    """rotations_to_rig -> bvh_text -> bvh_to_joints gives the joints back.  Yardstick: the composed fp32 restatement (rig_ref's
    channels -> the text -> rig_import_ref's joints) against the same joints."""
    MRig = pkg("motion_rig")
    off, j, r = fk("t2m_clean")
    rig = MRig.rig_of("t2m")
    num = 3 if fps_out else 1
    chan, lens_out = MRig.rotations_to_rig(j, r, LENS, euler=order, fps_out=fps_out)
    chan, jn, rn = chan.cpu(), j.cpu().numpy(), r.cpu().numpy()
    out = [MRig.bvh_text(rig, off, chan[b], int(m), 1 / (20 * num), euler=order) for b, m in enumerate(lens_out)]
    got = MRig.bvh_to_joints(out, fps_out=20)
    y = 0.0
    for b, n in enumerate(LENS):
        c32 = RR.rig_channels(rig, jn[b, :n], rn[b, :n], order, num=num, den=1, dtype=np.float32)[0]
        bvh = RR.parse_bvh(MRig.bvh_text(rig, off, c32, len(c32), 1 / (20 * num), euler=order))
        back = IR.import_joints(bvh, IR.pick_of(bvh, own_names()), 1, num, np.float32)[0]
        y = max(y, float(np.abs(back - jn[b, :n]).max()))
    e = worst(got, [jn[b, :n] for b, n in enumerate(LENS)])
    print(order, fps_out, f"joints {e:.3g} (yardstick {y:.3g})")
    assert e <= GATE * y, (e, y)


def test_scale_up_and_basis():
    MRig = pkg("motion_rig")
    src = list(texts("cmu"))
    plain = MRig.bvh_to_joints(src)
    rs = np.random.RandomState(5)
    skew = tuple(map(tuple, rs.uniform(-1, 1, (3, 3))))
    for kw, basis in ((dict(scale=0.056, up="Z"), tuple(map(tuple, IR.Z_UP))), (dict(scale=100.0, basis=np.array(skew)), skew),
                      (dict(up="Z", basis=torch.eye(3)), None)):                              # basis overrides up
        files, picks, truth, y = truth_of("cmu", scale=kw.get("scale", 1.0), basis=basis)
        got = MRig.bvh_to_joints(src, **kw)
        e = worst(got, truth)
        print(sorted(kw), f"joints {e:.3g} (yardstick {y:.3g})")
        assert e <= GATE * y, (kw, e, y)
    z = MRig.bvh_to_joints(src, up="Z")
    assert all(torch.equal(a[..., 0], p[..., 0]) and torch.equal(a[..., 1], p[..., 2]) and torch.equal(a[..., 2], -p[..., 1])
               for a, p in zip(z, plain))                                                     # (x, y, z) -> (x, z, -y)
    for s in (0.056, 4.0, 100.0):                                                             # the scale is the last product
        assert all(torch.equal(a, p * float(np.float32(s))) for a, p in zip(MRig.bvh_to_joints(src, scale=s), plain)), s
    for bad in (dict(up="X"), dict(basis=np.eye(4)), dict(basis=np.full((3, 3), np.nan)), dict(scale=float("inf")), dict(fps_out=0),
                dict(joint_map="mixamo")):
        with pytest.raises(ValueError):
            MRig.bvh_to_joints(src, **bad)
    with pytest.raises(ValueError):
        MRig.bvh_to_joints(src[0])                                                            # a list is wanted
    with pytest.raises(pkg("_lib").MdmError):
        MRig.bvh_to_joints(src, device="cpu")                                                 # no eager fallback


def test_bvh_to_motion():
    """(b) of the clean golden clip (human proportions, heading Z+) -> rows on target offsets: the same bits as the two calls
    it stands for, and the rows show the canonical joints within the round-trip gate of tests/test_motion_features_gpu.py
    (4 x the round trip of the restated reference functions), here on the fp64 restatement's joints."""
    import motion_features_ref as MR
    import test_motion_features_gpu as TF
    MRig, MF, P = pkg("motion_rig"), pkg("motion_features"), pkg("postprocess")
    src = list(texts("cmu", name="t2m_clean"))[:2]
    sk = TF.ref_skel("t2m")
    tgt = MF.skeleton_offsets(MR.synth_clip(sk, 2, 77)[0])
    zero, one = np.zeros(263, np.float32), np.ones(263, np.float32)
    rows, n = MRig.bvh_to_motion(src, zero, one, target_offsets=tgt)
    assert rows.shape == (2, 23, 263) and n.tolist() == [23, 1]
    clips = MRig.bvh_to_joints(src)
    rows2, pos = MF.joints_to_motion(clips, None, zero, one, target_offsets=tgt, return_positions=True)
    assert torch.equal(rows, rows2)
    back = P.motion_to_joints(rows, zero, one, n, sigma=0.0)
    truth = truth_of("cmu", name="t2m_clean")[2][:2]
    gate = 0.0
    for c in truth:
        data, glob = MR.process_file(sk, c, 0.002, tgt.numpy())
        gate = max(gate, GATE * float(np.abs(TF.PR.recover_from_ric(torch.from_numpy(data).float(), sk.J).numpy() - glob[:-1]).max()))
    errs = [float((back[i, :k] - pos[i, :k]).abs().max()) for i, k in enumerate(n.tolist())]
    print("bvh_to_motion round trip", max(errs), "gate", gate)
    assert max(errs) <= gate, (errs, gate)
    assert not rows[1, 1:].any()
    # the CMU files' own hierarchy, zero offsets and all, under the default preset: rows without a NaN
    real, nr = MRig.bvh_to_motion([IR.cmu_real()], zero, one, fps_out=None)
    assert real.shape == (1, 8, 263) and nr.tolist() == [8] and bool(torch.isfinite(real).all())
    with pytest.raises(ValueError, match="no length"):
        MRig.bvh_to_motion([IR.cmu_real()], zero, one, joint_map=IR.CMU_NAIVE)


def test_through_the_trainer():
    import test_motion_features_gpu as TF
    MRig, E = pkg("motion_rig"), pkg("motion_edit")
    tr = TF._tiny_trainer()
    off, joints, rots = golden("t2m_clean")
    rig = MRig.rig_of("t2m")                                          # 13 and 9 frames: 12 and 8 rows in the tiny model's window of 16
    src = [IR.cmu_like(rig, off, joints[0][:13], rots[0][:13]), IR.own_export(MRig.bvh_text, rig, off, joints[0][:9], rots[0][:9])]
    gen = torch.Generator().manual_seed(2)
    mean, std = (torch.randn(263, generator=gen) * 0.1).numpy(), (0.5 + torch.rand(263, generator=gen)).numpy()
    caps, lens = ["a", "b"], torch.tensor([16, 16])
    mask = torch.stack([E.prefix_mask(16, 12), E.prefix_mask(16, 8)])
    opts = dict(seed=4, sampler="ddim", sample_steps=5, eta=0.5, edit_mask=mask, batch_size=2, mean=mean, std=std)
    bo = dict(scale=0.5, up="Y")
    a = tr.generate(caps, lens, 263, edit_bvh=src, bvh_options=bo, **opts)
    clips = MRig.bvh_to_joints(src, **bo)
    b = tr.generate(caps, lens, 263, edit_joints=clips, **opts)
    assert len(a) == 2 and all(torch.equal(x, y) for x, y in zip(a, b))
    plain = tr.generate(caps, lens, 263, edit_bvh=src, **opts)
    assert not torch.equal(plain[0], a[0])
    scripts = [[("a", 16), ("b", 16)]]
    lopts = dict(overlap=4, seed=4, sampler="ddim", sample_steps=5, edit_mask=[E.prefix_mask(28, 12)], mean=mean, std=std)
    la = tr.generate_long(scripts, 263, edit_bvh=src[:1], bvh_options=bo, **lopts)
    lb = tr.generate_long(scripts, 263, edit_joints=clips[:1], **lopts)
    assert la[0].shape == (28, 263) and torch.equal(la[0], lb[0])
    # file in -> continued -> file out, in one call: the kept frames come back from the text
    out = tr.generate_bvh(caps, lens, 263, mean, std, edit_bvh=src, bvh_options=bo, **{k: v for k, v in opts.items() if k not in ("mean", "std")})
    assert [RR.parse_bvh(t).frames for t in out] == [16, 16]
    rot = tr.generate_rotations(caps, lens, 263, mean, std, edit_bvh=src, bvh_options=bo, **{k: v for k, v in opts.items() if k not in ("mean", "std")})
    assert [tuple(r[0].shape) for r in rot] == [(16, 22, 3), (16, 22, 3)]
    for kw in (dict(edit_bvh=src, edit_joints=clips), dict(edit_bvh=src, edit_motion=torch.zeros(2, 16, 263)), dict(bvh_options=bo),
               dict(edit_bvh=src, bvh_options=dict(euler="ZXY"))):
        with pytest.raises(ValueError):
            tr.generate(caps, lens, 263, **dict(opts, **kw))
    with pytest.raises(ValueError, match="exclusive"):
        tr.generate_long(scripts, 263, edit_bvh=src[:1], edit_joints=clips[:1], **lopts)

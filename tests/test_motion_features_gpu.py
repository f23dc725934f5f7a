"""GPU: joints -> feature rows on the device (mdm_motion_features).

* parity with the reference on tests/golden/motion_features.npz (its process_file output), per column group, foot contacts
  exactly, rows past each length exactly zero;
* round trips with motion_to_joints, refeaturize, a full-size ragged batch against the restatement;
* through the trainer: edit_joints == edit_motion of the converted rows bit for bit, generate_for_evaluation unchanged
  without the new arguments and consistent with them;
* bad arguments on the device path.

Tolerances.  e32 is the error of the all-fp32 CPU restatement (tests/motion_features_ref.py, all32=True) against the
golden, per case and column group, as tools/make_motion_features_golden.py printed and recorded it in the golden's meta.
The device differs from that restatement only in the operation order inside sums, in asinf / sqrtf and in where the
facing-direction filter is rounded, so every case is gated at 4 x its own e32 per group (a wrong term is >= 1e-2 on these
inputs).  e32, and in brackets what the device measured on an MI355X:
    case          root                ric                 rot6d               vel                 canonical positions
    t2m_uniform   5.36e-07 (3.5e-07)  6.08e-06 (6.2e-06)  9.78e-06 (9.9e-06)  1.01e-05 (8.9e-06)  6.05e-06 (6.1e-06)
    t2m_plain     2.29e-07 (1.8e-07)  2.98e-07 (2.5e-07)  3.61e-06 (2.8e-06)  3.13e-07 (2.6e-07)  5.36e-07 (4.2e-07)
    t2m_two       7.45e-08 (8.2e-08)  1.49e-07 (1.5e-07)  1.01e-06 (1.1e-06)  1.49e-07 (1.2e-07)  1.49e-07 (1.5e-07)
    kit_uniform   6.46e-07 (6.7e-07)  5.78e-06 (6.1e-06)  3.53e-04 (3.5e-04)  8.90e-06 (6.9e-06)  4.77e-06 (5.5e-06)
KIT's rot6d e32 is 36 x the largest t2m one because of the reference's KIT tables, not of the clip: the bone axes of the
two hip joints (11: +x, 16: -x) point opposite to where process_file's canonical pose puts those joints (the golden's hip
bones have cosines of -0.73 .. -1.00 to their axes), so qbetween(axis, bone) works next to its antiparallel singularity for
them, and every rotation further down the legs is taken relative to theirs.
Where a test has other inputs than the golden's, the same yardstick is computed on those inputs: 4 x the error of the
all-fp32 restatement against the restatement in the reference's fp64 mix.  Round trips are held to 4 x the same round
trip through the restated reference functions (oracle/motion_ref.py recover_from_ric on the fp64-mix rows).
"""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, build_module, load_golden, pkg

import motion_features_ref as MR

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import motion_ref as PR  # noqa: E402

pytestmark = pytest.mark.gpu

GATE = 4.0          # x e32 / x the reference's round trip
BAND = 1e-4         # a contact may be left out when the reference's squared foot speed is this close to feet_thre ...
MAX_LEFT_OUT = 0.01  # ... for at most this share of a case's contact entries


def golden():
    z = np.load(os.path.join(GOLDEN, "motion_features.npz"))
    return z, json.loads(str(z["meta"]))


def ref_skel(name):
    sk = pkg("motion_features").SKELETONS[name]  # equal to the reference's tables: tests/test_motion_features_host.py
    return MR.skeleton_from_tables(sk.chains, sk.raw_offsets, sk.face, sk.feet, sk.legs)


def group_err(got, want, J):
    return {k: float(np.abs(got[..., s] - want[..., s]).max()) if want.size else 0.0 for k, s in MR.column_groups(J).items()}


def check_contacts(got, want, speed2, thre, what):
    """Exact, but for entries whose reference squared foot speed lies within BAND (relative) of the threshold."""
    near = np.abs(speed2.astype(np.float64) - thre) < BAND * thre
    assert near.mean() <= MAX_LEFT_OUT, (what, float(near.mean()))
    assert np.array_equal(got[~near], want[~near]), (what, int((got[~near] != want[~near]).sum()))
    assert set(np.unique(got)) <= {0.0, 1.0}


def test_parity_with_the_reference():
    MF = pkg("motion_features")
    z, meta = golden()
    for case in meta["cases"]:
        e32 = case["e32"]  # this case's own
        n, sk = case["name"], MF.SKELETONS[case["skel"]]
        tgt = z[f"{n}_target_offsets"] if f"{n}_target_offsets" in z.files else None
        want, wpos = z[f"{n}_data"], z[f"{n}_global_positions"]
        clip = torch.from_numpy(z[f"{n}_joints"]).float().cuda()
        T = case["n"] + 3  # padded: rows past length - 1 must come out zero
        x = torch.full((2, T, sk.joints, 3), 7.0, device="cuda")
        x[0, :case["n"]] = clip
        x[1, :case["n"]] = clip
        rows, pos = MF.joints_to_motion(x, [case["n"], case["n"]], skeleton=case["skel"], target_offsets=tgt,
                                        return_positions=True)
        assert rows.shape == (2, T - 1, sk.feats) and pos.shape == x.shape
        assert torch.equal(rows[0], rows[1]) and torch.equal(pos[0], pos[1])
        rows, pos = rows[0].cpu().numpy(), pos[0].cpu().numpy()
        assert not rows[case["n"] - 1:].any() and not pos[case["n"]:].any()
        err = group_err(rows[:case["n"] - 1], want, sk.joints)
        err["pos"] = float(np.abs(pos[:case["n"]] - wpos).max())
        print(n, {k: f"{v:.3g}" for k, v in err.items()}, "gates", {k: f"{GATE * v:.3g}" for k, v in e32.items()})
        for k, v in err.items():
            assert v <= GATE * e32[k], (n, k, v, GATE * e32[k])
        speed2 = MR.extract_features(ref_skel(case["skel"]), wpos, case["feet_thre"])[1]
        check_contacts(rows[:case["n"] - 1, -4:], want[:, -4:], speed2, case["feet_thre"], n)
        # the one-clip forms under the reference's names
        d1, g1 = MF.process_file(clip, case["feet_thre"], skeleton=case["skel"], target_offsets=tgt)
        assert torch.equal(d1.cpu(), torch.from_numpy(rows[:case["n"] - 1])) and torch.equal(g1.cpu(), torch.from_numpy(pos[:case["n"]]))
        d2 = MF.extract_features(g1, case["feet_thre"], skeleton=case["skel"])
        assert torch.equal(d2, d1)  # extract_features is the tail of process_file


def _ragged(B, T, seed, short=(2,), turn=1.0):
    sk = ref_skel("t2m")
    rng = np.random.RandomState(seed)
    lens = [T] + list(short) + [int(v) for v in rng.randint(3, T + 1, B - 1 - len(short))]
    return sk, [MR.synth_clip(sk, n, seed * 1000 + i, turn) for i, n in enumerate(lens)], lens


def _round_trip_gate(sk, clips):
    """4 x the largest round-trip error of the restated reference functions on these clips (fp64-mix rows -> fp32 joints)."""
    worst = 0.0
    for c in clips:
        data, glob = MR.process_file(sk, c, 0.002)
        if len(data):
            rec = PR.recover_from_ric(torch.from_numpy(data).float(), sk.J).numpy()
            worst = max(worst, float(np.abs(rec - glob[:-1]).max()))
    return GATE * worst


@pytest.mark.parametrize("B,T,turn", [(4, 196, 1.0), (1, None, 0.0)])
def test_round_trip_with_motion_to_joints(B, T, turn):
    MF, P, Tr = pkg("motion_features"), pkg("postprocess"), pkg("trainer")
    T = T or Tr.MAX_JOINTS_FRAMES
    sk, clips, lens = _ragged(B, T, 5, short=(2,) if B > 1 else (), turn=turn)
    gate = _round_trip_gate(sk, clips)
    cl = [torch.from_numpy(c).float().cuda() for c in clips]
    zero, one = np.zeros(263, np.float32), np.ones(263, np.float32)
    rows, pos = MF.joints_to_motion(cl, return_positions=True)
    assert rows.shape == (B, T - 1, 263)
    back = P.motion_to_joints(rows, zero, one, torch.tensor(lens) - 1, sigma=0.0)
    errs = [float((back[i, :n - 1] - pos[i, :n - 1]).abs().max()) for i, n in enumerate(lens)]
    print("canonical round trip", max(errs), "gate", gate)
    assert max(errs) <= gate, (errs, gate)
    # taken as they are: the rows describe the input but for frame 0's root XZ, which recover_from_ric puts at the origin.
    # Inputs: the canonical clips turned by 0.5 rad and moved off the origin, so that frame 0's forced identity quaternion and
    # the first rotation velocity are not trivial (a clip that faces away from Z+ at some frame is ill-conditioned in the
    # reference itself: qbetween towards Z+); gate: 4 x the same round trip through the restated reference functions
    shift = torch.tensor([1.5, 0.0, -2.0], device="cuda")
    c5, s5 = float(np.cos(0.5)), float(np.sin(0.5))
    turn5 = torch.tensor([[c5, 0.0, s5], [0.0, 1.0, 0.0], [-s5, 0.0, c5]], device="cuda")  # frame 0 heads 0.5 rad off Z+
    moved = [pos[i, :n] @ turn5.T + shift for i, n in enumerate(lens)]
    gate2 = GATE * max(_refeat_round_trip(sk, c.cpu().numpy()) for c in moved)
    rows2 = MF.joints_to_motion(moved, canonicalize=False)
    back2 = P.motion_to_joints(rows2, zero, one, torch.tensor(lens) - 1, sigma=0.0)
    errs = []
    for i, n in enumerate(lens):
        want = moved[i][:n - 1] - moved[i][0, 0] * torch.tensor([1.0, 0.0, 1.0], device="cuda")
        errs.append(float((back2[i, :n - 1] - want).abs().max()))
    print("as-is round trip", max(errs), "gate", gate2)
    assert max(errs) <= gate2, (errs, gate2)


def test_refeaturize_keeps_the_joints_and_is_a_fixed_point():
    MF, P = pkg("motion_features"), pkg("postprocess")
    gen = torch.Generator().manual_seed(8)
    B, T = 6, 60
    mean, std = (torch.randn(263, generator=gen) * 0.1).numpy(), (0.5 + torch.rand(263, generator=gen)).numpy()
    lens = torch.tensor([60, 3, 33, 47, 60, 5])
    # rows of moving skeletons whose steerable columns (root, positions) were pushed about, as joint control does, and whose
    # other columns are random numbers: none of those enters recover_from_ric
    sk = ref_skel("t2m")
    base = MF.joints_to_motion([torch.from_numpy(MR.synth_clip(sk, n + 1, 500 + i)).float().cuda() for i, n in enumerate(lens.tolist())],
                               None, mean, std)
    m = torch.randn(B, T, 263, generator=gen).cuda()
    m[:, :, :67] = base[:, :, :67] + 0.02 * m[:, :, :67]
    want = P.motion_to_joints(m, mean, std, lens, sigma=0.0)
    r1 = MF.refeaturize(m, mean, std, lens)
    assert r1.shape == (B, T - 1, 263)
    got = P.motion_to_joints(r1, mean, std, lens - 1, sigma=0.0)
    gate = GATE * max(_refeat_round_trip(sk, want[i, :n].cpu().numpy()) for i, n in enumerate(lens.tolist()))
    errs = [float((got[i, :n - 1] - want[i, :n - 1]).abs().max()) for i, n in enumerate(lens.tolist())]
    print("refeaturize round trip", max(errs), "gate", gate)
    assert max(errs) <= gate, (errs, gate)
    for i, n in enumerate(lens.tolist()):
        assert not r1[i, n - 1:].any()
    # A second pass over its own output.  Its rows cannot equal the first pass's: it has one frame fewer, so the sigma-20
    # "nearest"-edge filter of the facing direction, with it the root quaternion and every column rotated by it, changes.
    # What is well defined is compared: the joints the rows show (gate as above), and what a rotation about Y leaves alone
    # in rows of joints that agree to `gate`: root height, the height and the horizontal length of every root-relative
    # position and joint velocity (each a difference of two positions: 2 x gate), and the foot contacts (exact, but where
    # the squared foot speed s lies so close to the threshold that moving both frames by `gate` can cross it:
    # |s - thre| <= 4 sqrt(thre) gate + 4 gate^2, doubled for fp32 rounding of s).
    r2 = MF.refeaturize(torch.cat([r1, r1[:, -1:]], 1), mean, std, lens - 1)
    got2 = P.motion_to_joints(r2, mean, std, (lens - 2).clamp(min=0), sigma=0.0)
    mean_t, std_t = torch.from_numpy(mean).cuda(), torch.from_numpy(std).cuda()
    worst = {"joints": 0.0, "height": 0.0, "ric": 0.0, "vel": 0.0}
    for i, n in enumerate(lens.tolist()):
        if n < 3:
            continue
        k = n - 2
        worst["joints"] = max(worst["joints"], float((got2[i, :k] - got[i, :k]).abs().max()))
        a, b = r2[i, :k] * std_t + mean_t, r1[i, :k] * std_t + mean_t
        worst["height"] = max(worst["height"], float((a[:, 3] - b[:, 3]).abs().max()))
        for name, sl in (("ric", slice(4, 67)), ("vel", slice(193, 259))):
            va, vb = a[:, sl].reshape(k, -1, 3), b[:, sl].reshape(k, -1, 3)
            dy = (va[..., 1] - vb[..., 1]).abs().max()
            dh = (torch.linalg.vector_norm(va[..., [0, 2]], dim=-1) - torch.linalg.vector_norm(vb[..., [0, 2]], dim=-1)).abs().max()
            worst[name] = max(worst[name], float(dy), float(dh))
        feet = got[i, :k + 1][:, list(MF.SKELETONS["t2m"].feet)].double()
        s2 = ((feet[1:] - feet[:-1]) ** 2).sum(-1)
        clear = (s2 - 0.002).abs() > 2 * (4 * 0.002 ** 0.5 * gate + 4 * gate * gate)
        ca, cb = torch.round(a[:, -4:]), torch.round(b[:, -4:])
        assert float((a[:, -4:] - ca).abs().max()) < 1e-5 and torch.equal(ca[clear], cb[clear]), i
    # de-normalising x * std + mean rounds every value once more
    slack = 4 * np.finfo(np.float32).eps * float((r1 * std_t + mean_t)[..., :259].abs().max())
    print("second pass", {k: f"{v:.3g}" for k, v in worst.items()}, "gate", gate, "slack", slack)
    assert worst["joints"] <= gate and worst["height"] <= gate + slack, worst
    assert worst["ric"] <= 2 * gate + slack and worst["vel"] <= 2 * gate + slack, worst


def _refeat_round_trip(sk, joints):
    if len(joints) < 2:
        return 0.0
    data = MR.extract_features(sk, joints.astype(np.float64), 0.002)[0]
    rec = PR.recover_from_ric(torch.from_numpy(data).float(), sk.J).numpy()
    want = joints[:-1] - joints[0, 0] * np.array([1.0, 0.0, 1.0])
    return float(np.abs(rec - want).max())


def test_full_size_batch_against_the_restatement():
    MF = pkg("motion_features")
    B, T = 32, 196
    sk, clips, lens = _ragged(B, T, 9, short=(2, 3))
    gen = torch.Generator().manual_seed(1)
    mean, std = (torch.randn(263, generator=gen) * 0.1).numpy(), (0.5 + torch.rand(263, generator=gen)).numpy()
    tgt = MF.skeleton_offsets(MR.synth_clip(sk, 2, 77)[0])
    assert np.array_equal(tgt.numpy(), MR.get_offsets(sk, MR.synth_clip(sk, 2, 77)[0]).numpy())
    cl = [torch.from_numpy(c).float().cuda() for c in clips]
    for target in (None, tgt):
        rows, pos = MF.joints_to_motion(cl, None, mean, std, target_offsets=target, return_positions=True)
        rows, pos = rows.cpu().numpy(), pos.cpu().numpy()
        worst = {}
        for i, (c, n) in enumerate(zip(clips, lens)):
            t64 = None if target is None else target.numpy()
            lo, plo = MR.process_file(sk, c, 0.002, t64, all32=False)
            hi, phi = MR.process_file(sk, c, 0.002, t64, all32=True)
            e32 = group_err(hi, lo, 22)
            e32["pos"] = float(np.abs(phi - plo).max())
            got = rows[i, :n - 1] * std + mean
            err = group_err(got, lo, 22)
            err["pos"] = float(np.abs(pos[i, :n] - plo).max())
            for k in err:
                # de-normalising the device's rows adds one fp32 rounding of each value
                slack = 2 * np.finfo(np.float32).eps * float(np.abs(lo[:, MR.column_groups(22)[k]]).max()) if k != "pos" and lo.size else 0.0
                assert err[k] <= GATE * e32[k] + slack, (i, n, k, err[k], e32[k])
                worst[k] = max(worst.get(k, 0.0), err[k] / max(e32[k], 1e-12))
            speed2 = MR.extract_features(sk, plo, 0.002)[1]
            contacts = np.rint(rows[i, :n - 1, -4:] * std[-4:] + mean[-4:])
            assert np.abs(contacts - (rows[i, :n - 1, -4:] * std[-4:] + mean[-4:])).max() < 1e-5
            near = np.abs(speed2.astype(np.float64) - 0.002) < BAND * 0.002
            assert np.array_equal(contacts[~near], lo[:, -4:][~near]), (i, n)
            assert not rows[i, n - 1:].any() and not pos[i, n:].any()
        print("full size, target offsets" if target is not None else "full size", "worst err / e32", {k: f"{v:.2f}" for k, v in worst.items()})


def _tiny_trainer(steps=25):
    g, meta = load_golden("loops_tiny")
    m, _ = build_module(meta, precision=3)
    m.set_uncond_embedding(g["xf_proj_uncond"][:1].cuda(), g["xf_out_uncond"][:1].cuda())
    synth = pkg("synth")
    Dt = meta["text_latent_dim"]

    def enc(text, device):
        xo = torch.stack([synth.uniform_pm1((6, Dt), "cap." + t, 1) * (3.0 ** 0.5) for t in text])
        return xo.mean(1).to(device), xo.to(device)

    m.text_encoder_fn = enc
    args = types.SimpleNamespace(device=torch.device("cuda"), diffusion_steps=steps, is_train=False, cfg_scale=2.5)
    return pkg("trainer").DDPMTrainer(args, m)


def test_edit_joints_through_the_trainer():
    MF, P, E = pkg("motion_features"), pkg("postprocess"), pkg("motion_edit")
    tr = _tiny_trainer()
    sk = ref_skel("t2m")
    ns = [9, 13, 5, 16]
    clips = [torch.from_numpy(MR.synth_clip(sk, n, 300 + n)).float() for n in ns]  # CPU clips: the trainer moves them
    gen = torch.Generator().manual_seed(2)
    mean, std = (torch.randn(263, generator=gen) * 0.1).numpy(), (0.5 + torch.rand(263, generator=gen)).numpy()
    T = 16
    caps, lens = ["a", "b", "c", "d"], torch.tensor([16, 16, 12, 16])
    mask = torch.stack([E.prefix_mask(T, n - 1) for n in ns])
    opts = dict(seed=4, sampler="ddim", sample_steps=5, eta=0.5, edit_mask=mask, batch_size=2)
    a = tr.generate(caps, lens, 263, edit_joints=clips, mean=mean, std=std, **opts)
    rows, pos = MF.joints_to_motion([c.cuda() for c in clips], None, mean, std, return_positions=True)
    known = torch.zeros(4, T, 263, device="cuda")
    known[:, :rows.shape[1]] = rows
    b = tr.generate(caps, lens, 263, edit_motion=known, **opts)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    gate = _round_trip_gate(sk, [c.numpy().astype(np.float64) for c in clips])
    for i, n in enumerate(ns):
        k = min(n - 1, a[i].shape[0])
        assert torch.equal(a[i][:k], rows[i, :k])  # the editing tolerance of tests/test_motion_edit_gpu.py: kept entries exact
        j = P.motion_to_joints(a[i][None, :k], mean, std, sigma=0.0)[0]
        # de-normalising x * std + mean rounds each feature once more than the reference's round trip does
        slack = 4 * np.finfo(np.float32).eps * float(pos[i].abs().max())
        assert float((j - pos[i, :k]).abs().max()) <= gate + slack
    bk = tr.generate_bucketed(caps, lens, 263, 2, unit_length=4, edit_joints=clips, mean=mean, std=std,
                              **{k: v for k, v in opts.items() if k != "batch_size"})
    for i, n in enumerate(lens.tolist()):
        k = min(ns[i] - 1, n)
        assert torch.equal(bk[i][:k], rows[i, :k])
    jj = tr.generate_joints(caps, lens, 263, mean, std, sigma=0.0, edit_joints=clips, **opts)
    assert [tuple(j.shape) for j in jj] == [(n, 22, 3) for n in lens.tolist()]
    with pytest.raises(ValueError, match="one frame short"):
        tr.generate(caps, lens, 263, edit_joints=clips, mean=mean, std=std, **dict(opts, edit_mask=E.prefix_mask(T, 5)))
    with pytest.raises(ValueError, match="exclusive"):
        tr.generate(caps, lens, 263, edit_joints=clips, edit_motion=known, mean=mean, std=std, **opts)
    # a long motion continued from joints
    scripts = [[("a", 16), ("b", 16)]]
    canvas = 16 + 16 - 4
    lm = tr.generate_long(scripts, 263, overlap=4, seed=4, sampler="ddim", sample_steps=5, edit_joints=[clips[1]],
                          edit_mask=[E.prefix_mask(canvas, 12)], mean=mean, std=std)
    assert lm[0].shape == (canvas, 263) and torch.equal(lm[0][:12], rows[1, :12])
    # joints in, joints out: generate_long_joints converts the clip under its own mean / std
    lj = tr.generate_long_joints(scripts, 263, mean, std, sigma=0.0, overlap=4, seed=4, sampler="ddim", sample_steps=5,
                                 edit_joints=[clips[1]], edit_mask=[E.prefix_mask(canvas, 12)])
    assert lj[0].shape == (canvas, 22, 3)
    assert torch.equal(lj[0], P.motion_to_joints(lm[0][None], mean, std, sigma=0.0)[0])
    slack = 4 * np.finfo(np.float32).eps * float(pos[1].abs().max())
    assert float((lj[0][:12] - pos[1, :12]).abs().max()) <= gate + slack


def test_generate_for_evaluation_unchanged_and_consistent():
    P = pkg("postprocess")
    tr = _tiny_trainer()
    N, T = 6, 16
    caps = [f"caption {i}" for i in range(N)]
    raw = torch.tensor([16, 9, 13, 5, 16, 12])
    kw = dict(mm_num_samples=2, mm_num_repeats=2, unit_length=1, max_motion_length=T, seed=5, batch_size=4, sampler="dpmpp2m",
              sample_steps=5)
    out = tr.generate_for_evaluation(caps, raw, 263, **kw)
    lens = out["m_lens"]
    mm = set(out["mm_idxs"].tolist())
    all_cap = [c for i, c in enumerate(caps) for _ in range(2 if i in mm else 1)]
    all_len = [int(lens[i]) for i in range(N) for _ in range(2 if i in mm else 1)]
    first = np.cumsum([0] + [2 if i in mm else 1 for i in range(N)])[:-1]
    ref = tr.generate_bucketed(all_cap, torch.tensor(all_len), 263, 4, unit_length=1, seed=5, sampler="dpmpp2m", sample_steps=5)
    for i in range(N):
        n = int(lens[i])
        assert torch.equal(out["motions"][i, :n], ref[first[i]][:n]) and not out["motions"][i, n:].any()
    gen = torch.Generator().manual_seed(3)
    mean, std = (torch.randn(263, generator=gen) * 0.1).numpy(), (0.5 + torch.rand(263, generator=gen)).numpy()
    con = tr.generate_for_evaluation(caps, raw, 263, consistent_features=True, mean=mean, std=std, **kw)
    assert torch.equal(con["m_lens"], lens - 1) and torch.equal(con["mm_lens"], out["mm_lens"] - 1)
    assert con["motions"].shape == out["motions"].shape and con["mm_motions"].shape == out["mm_motions"].shape
    sk = ref_skel("t2m")
    for i in range(N):
        n = int(lens[i])
        want = P.motion_to_joints(out["motions"][i:i + 1, :n], mean, std, sigma=0.0)[0]
        got = P.motion_to_joints(con["motions"][i:i + 1, :n - 1], mean, std, sigma=0.0)[0]
        gate = GATE * _refeat_round_trip(sk, want.cpu().numpy())
        assert float((got - want[:n - 1]).abs().max()) <= gate, (i, float((got - want[:n - 1]).abs().max()), gate)
        assert not con["motions"][i, n - 1:].any()
        assert not torch.equal(con["motions"][i, :n - 1, 67:193], out["motions"][i, :n - 1, 67:193])  # rot6d rewritten
    with pytest.raises(ValueError, match="mean and std"):
        tr.generate_for_evaluation(caps, raw, 263, consistent_features=True, **kw)
    rf = tr.refeaturize([out["motions"][i] for i in range(N)], lens, mean, std)
    assert [tuple(r.shape) for r in rf] == [(int(n) - 1, 263) for n in lens]
    assert torch.equal(rf[0], con["motions"][0, :int(lens[0]) - 1])


def test_bad_arguments_on_the_device_path():
    MF, L = pkg("motion_features"), pkg("_lib")
    sk = ref_skel("t2m")
    clip = torch.from_numpy(MR.synth_clip(sk, 8, 1)).float()
    with pytest.raises(L.MdmError):
        MF.joints_to_motion(clip[None])  # a CPU tensor
    with pytest.raises(ValueError):
        MF.joints_to_motion(clip[None, :, :20].cuda())
    with pytest.raises(L.MdmError):
        MF.joints_to_motion(torch.zeros(1, MF.max_frames() + 1, 22, 3, device="cuda"))
    assert MF.joints_to_motion(clip[None].cuda()).shape == (1, 7, 263)
    kit = MF.joints_to_motion(torch.from_numpy(MR.synth_clip(ref_skel("kit"), 8, 1)).float().cuda()[None], skeleton="kit")
    assert kit.shape == (1, 7, 251) and bool(torch.isfinite(kit).all())

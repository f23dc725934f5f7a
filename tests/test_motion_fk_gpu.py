"""GPU: rows -> joints by forward kinematics of the rot6d columns (mdm_motion_fk).

* parity with the reference's recover_from_rot on tests/golden/motion_fk.npz: joints, global rotations, filtered joints;
* round trip joints -> rows (joints_to_motion) -> joints on each clip's own frame-0 offsets;
* rigid bones, where the same rows through motion_to_joints have none; a sample's own mean-bone-length offsets;
* lengths (nothing past a length is read, every sample equals its run alone), more frames than threads, T = 1 and 2;
* through the trainer: generate_joints(from_rotations=True), the unchanged default, generate_long_joints, generate_rotations;
* bad arguments on the device path.

Tolerances.  GATE = 4 x a yardstick measured on the same inputs: the error of the reference's own fp32 result (or, where the
reference was not recorded, of the fp32 restatement tests/motion_fk_ref.py, which reproduces the reference bit for bit on the
golden) against the fp64 restatement; tests/test_motion_features_gpu.py uses the same convention.  The golden's cases read
their yardsticks from its meta (joints 3.0e-7 .. 3.7e-7, rotations 3.4e-7 .. 5.8e-7, offsets 2.3e-8 .. 7.3e-8); the other
cases compute theirs at test time, for the quantity they compare (positions, bone lengths, R^T R - I).  Nothing is gated
against the kernel's own output.  tests/test_motion_fk_host.py shows that each of the mistakes an implementation most easily
makes lies >= 1e5 gates away on the golden's inputs.
"""
import json
import os

import numpy as np
import pytest
import torch
from scipy.ndimage import gaussian_filter1d

from conftest import GOLDEN, pkg

import motion_features_ref as MR
import motion_fk_ref as FR
import test_motion_features_gpu as TF

pytestmark = pytest.mark.gpu

GATE = 4.0
CASES = ("t2m_clean", "t2m_noisy", "kit_clean", "kit_noisy")


def golden(name):
    z = np.load(os.path.join(GOLDEN, "motion_fk.npz"))
    meta = json.loads(str(z["meta"]))
    case = {c["name"]: c for c in meta["cases"]}[name]
    s = case["skel"]
    g = dict(skel=s, sk=TF.ref_skel(s), rows=z[f"{name}_rows"], mean=z[f"{s}_mean"], std=z[f"{s}_std"], lens=meta["lengths"],
             off=z[f"{s}_offsets"], y=case["yardstick"], at=np.cumsum([0] + meta["lengths"]))
    for k in ("ref_joints", "joints64", "rotations64", "offsets64"):
        g[k] = z[f"{name}_{k}"]
    return g


def bone_lengths(j, sk):
    j = np.asarray(j, np.float64)
    return np.linalg.norm(j[..., 1:, :] - j[..., np.asarray(sk.parents[1:]), :], axis=-1)


def noisy_rows(sk, n, seed, feet_thre=0.002, noise=0.1):
    """(n, F) fp32 rows of a synthetic clip with gaussian noise on all columns, the conditioning bound of the golden kept."""
    data = MR.process_file(sk, MR.synth_clip(sk, n + 1, seed), feet_thre)[0].astype(np.float32)
    data = data + (noise * np.random.RandomState(seed).randn(*data.shape)).astype(np.float32)
    assert min(FR.gram_schmidt_margins(sk, data)) >= 0.2
    return data


@pytest.mark.parametrize("name", CASES)
def test_parity_with_the_reference(name):
    P = pkg("postprocess")
    g = golden(name)
    rows, off = torch.from_numpy(g["rows"]).cuda(), torch.from_numpy(g["off"])
    j, r = P.motion_to_joints_fk(rows, g["mean"], g["std"], g["lens"], off, skeleton=g["skel"], sigma=0.0, return_rotations=True)
    j1 = P.motion_to_joints_fk(rows, g["mean"], g["std"], g["lens"], off, skeleton=g["skel"], sigma=1.0)
    J = g["sk"].J
    assert j.shape == (3, 24, J, 3) and r.shape == (3, 24, J, 3, 3) and j1.shape == j.shape
    j, r, j1 = j.cpu().numpy(), r.cpu().numpy(), j1.cpu().numpy()
    worst = dict(joints=0.0, rotations=0.0, filtered=0.0)
    for b, n in enumerate(g["lens"]):
        sl = slice(g["at"][b], g["at"][b] + n)
        assert not j[b, n:].any() and not r[b, n:].any() and not j1[b, n:].any()
        worst["joints"] = max(worst["joints"], float(np.abs(j[b, :n] - g["ref_joints"][sl]).max()))
        worst["rotations"] = max(worst["rotations"], float(np.abs(r[b, :n] - g["rotations64"][sl]).max()))
        want = gaussian_filter1d(g["ref_joints"][sl], 1.0, axis=0, mode="nearest")
        worst["filtered"] = max(worst["filtered"], float(np.abs(j1[b, :n] - want).max()))
    print(name, {k: f"{v:.3g}" for k, v in worst.items()}, "yardsticks", {k: f"{v:.3g}" for k, v in g["y"].items()})
    assert worst["joints"] <= GATE * g["y"]["joints"], worst
    assert worst["rotations"] <= GATE * g["y"]["rotations"], worst
    assert worst["filtered"] <= GATE * g["y"]["joints"], worst
    # the one-clip form under the reference's name, on de-normalised rows
    data = torch.from_numpy(g["rows"][0] * g["std"] + g["mean"]).cuda()
    one = P.recover_from_rot(data, J, off)
    assert one.shape == (24, J, 3)
    assert float(np.abs(one.cpu().numpy() - g["ref_joints"][:24]).max()) <= GATE * g["y"]["joints"]


def test_round_trip_with_joints_to_motion():
    MF, P = pkg("motion_features"), pkg("postprocess")
    sk, clips, lens = TF._ragged(4, 196, 5)
    kit = TF.ref_skel("kit")
    sets = [("t2m", sk, clips, 0.002), ("kit", kit, [MR.synth_clip(kit, 60, 61)], 0.05)]
    for name, s, cl, thre in sets:
        # the gate: 4 x the same round trip through the restated reference functions (fp64-mix rows -> fp32 joints)
        worst = 0.0
        for c in cl:
            data, glob = MR.process_file(s, c, thre)
            if len(data):
                rec = FR.recover_from_rot(s, data.astype(np.float32), MR.get_offsets(s, glob[0]).numpy())
                worst = max(worst, float(np.abs(rec - glob[:-1]).max()))
        gate = GATE * worst
        ns = [len(c) for c in cl]
        F = 12 * s.J - 1
        rows, pos = MF.joints_to_motion([torch.from_numpy(c).float().cuda() for c in cl], skeleton=name, return_positions=True)
        offs = torch.stack([MF.skeleton_offsets(pos[b, 0].cpu(), name) for b in range(len(cl))])
        back = P.motion_to_joints_fk(rows, np.zeros(F, np.float32), np.ones(F, np.float32), torch.tensor(ns) - 1, offs,
                                     skeleton=name, sigma=0.0)
        errs = [float((back[i, :n - 1] - pos[i, :n - 1]).abs().max()) for i, n in enumerate(ns)]
        print(name, "round trip", max(errs), "gate", gate)
        assert max(errs) <= gate, (name, errs, gate)
        for i, n in enumerate(ns):
            assert not back[i, n - 1:].any()


def _mean_std(F, J, seed):
    """Statistics like a dataset's: the rot6d columns around the identity rotation, so that generated rows are well conditioned."""
    gen = torch.Generator().manual_seed(seed)
    mean, std = (torch.randn(F, generator=gen) * 0.1).numpy(), (0.5 + torch.rand(F, generator=gen)).numpy()
    a, b = 4 + 3 * (J - 1), 4 + 9 * (J - 1)
    mean[a:b] = np.tile(np.array([1, 0, 0, 0, 1, 0], np.float32), J - 1)
    std[a:b] = 0.1
    return mean, std


def _bone_gate(sk, data, off):
    """4 x how far the fp32 restatement's bones are from the offsets' lengths on these de-normalised rows."""
    want = np.linalg.norm(np.asarray(off, np.float64)[1:], axis=-1)
    return GATE * float(np.abs(bone_lengths(FR.recover_from_rot(sk, data, off), sk) - want).max())


def test_rigid_bones_where_motion_to_joints_has_none():
    P = pkg("postprocess")
    for name in ("t2m_noisy", "kit_noisy"):
        g = golden(name)
        rows = torch.from_numpy(g["rows"]).cuda()
        want = np.linalg.norm(g["off"].astype(np.float64)[1:], axis=-1)
        ref_err = max(float(np.abs(bone_lengths(g["ref_joints"][g["at"][b]:g["at"][b] + n], g["sk"]) - want).max())
                      for b, n in enumerate(g["lens"]))
        gate = GATE * ref_err  # the reference's own fp32 joints on these rows
        fk = P.motion_to_joints_fk(rows, g["mean"], g["std"], g["lens"], torch.from_numpy(g["off"]), skeleton=g["skel"], sigma=0.0)
        ric = P.motion_to_joints(rows, g["mean"], g["std"], torch.tensor(g["lens"]), g["sk"].J, sigma=0.0)
        e_fk = max(float(np.abs(bone_lengths(fk[b, :n].cpu().numpy(), g["sk"]) - want).max()) for b, n in enumerate(g["lens"]))
        e_ric = max(float(np.abs(bone_lengths(ric[b, :n].cpu().numpy(), g["sk"]) - want).max()) for b, n in enumerate(g["lens"]))
        print(name, "bones: fk", e_fk, "ric", e_ric, "gate", gate)
        assert e_fk <= gate and e_ric > 1000 * gate, (name, e_fk, e_ric, gate)
    # generated rows
    tr = TF._tiny_trainer()
    sk = TF.ref_skel("t2m")
    mean, std = _mean_std(263, 22, 11)
    lens = [16, 9, 12]
    motions = tr.generate(["a", "b", "c"], torch.tensor(lens), 263, seed=3, sampler="ddim", sample_steps=5)
    x = torch.zeros(3, 16, 263, device="cuda")
    for i, (m, n) in enumerate(zip(motions, lens)):
        x[i, :n] = m[:n]
    fk, off = P.motion_to_joints_fk(x, mean, std, lens, None, sigma=0.0, return_offsets=True)
    ric = P.motion_to_joints(x, mean, std, torch.tensor(lens), sigma=0.0)
    for b, n in enumerate(lens):
        data = x[b, :n].cpu().numpy() * std + mean
        assert min(FR.gram_schmidt_margins(sk, data)) >= 0.2
        o = off[b].cpu().numpy()
        gate = _bone_gate(sk, data, o)
        want = np.linalg.norm(o.astype(np.float64)[1:], axis=-1)
        e_fk = float(np.abs(bone_lengths(fk[b, :n].cpu().numpy(), sk) - want).max())
        spread = float(np.ptp(bone_lengths(ric[b, :n].cpu().numpy(), sk), axis=0).max())  # a bone's length range over the frames
        print("generated", b, "bones: fk", e_fk, "ric spread", spread, "gate", gate)
        assert e_fk <= gate and spread > 1000 * gate, (b, e_fk, spread, gate)


def test_own_offsets():
    MF, P = pkg("motion_features"), pkg("postprocess")
    for name in ("t2m_noisy", "kit_noisy"):
        g = golden(name)
        rows = torch.from_numpy(g["rows"]).cuda()
        j, r, off = P.motion_to_joints_fk(rows, g["mean"], g["std"], g["lens"], None, skeleton=g["skel"], sigma=0.0,
                                          return_rotations=True, return_offsets=True)
        assert off.shape == (3, g["sk"].J, 3)
        err = float(np.abs(off.cpu().numpy() - g["offsets64"]).max())
        print(name, "own offsets", err, "yardstick", g["y"]["offsets"])
        assert err <= GATE * g["y"]["offsets"]
        j2, r2, off2 = P.motion_to_joints_fk(rows, g["mean"], g["std"], g["lens"], off, skeleton=g["skel"], sigma=0.0,
                                             return_rotations=True, return_offsets=True)
        assert torch.equal(j2, j) and torch.equal(r2, r) and torch.equal(off2, off)
        # a shared (J, 3) table comes back once per sample
        off3 = P.motion_to_joints_fk(rows, g["mean"], g["std"], g["lens"], off[0], skeleton=g["skel"], return_offsets=True)[1]
        assert torch.equal(off3, off[:1].expand(3, -1, -1))
    # a clip with rigid bones: its own offsets are those of its frame 0
    sk = TF.ref_skel("t2m")
    clip = MR.synth_clip(sk, 41, 2)
    data, glob = MR.process_file(sk, clip, 0.002)
    truth = MR.get_offsets(sk, glob[0]).numpy()
    gate = GATE * float(np.abs(FR.mean_bone_offsets(sk, data.astype(np.float32)) - truth).max())
    rows, pos = MF.joints_to_motion(torch.from_numpy(clip).float().cuda()[None], return_positions=True)
    off = P.motion_to_joints_fk(rows, np.zeros(263, np.float32), np.ones(263, np.float32), return_offsets=True)[1]
    err = float((off[0].cpu() - MF.skeleton_offsets(pos[0, 0].cpu())).abs().max())
    print("rigid clip: own offsets against frame 0's", err, "gate", gate)
    assert err <= gate


def test_lengths():
    P = pkg("postprocess")
    g = golden("t2m_noisy")
    rows = torch.from_numpy(g["rows"]).cuda()
    lens = [24, 2, 1]
    assert g["lens"] == lens
    rows[1, 2:] = float("nan")
    rows[2, 1:] = torch.linspace(-1e30, 1e30, 23 * 263, device="cuda").reshape(23, 263)
    for offsets in (None, torch.from_numpy(g["off"])):
        for sigma in (0.0, 1.0):
            j, r, o = P.motion_to_joints_fk(rows, g["mean"], g["std"], lens, offsets, sigma=sigma, return_rotations=True,
                                            return_offsets=True)
            for b, n in enumerate(lens):
                assert not j[b, n:].any() and not r[b, n:].any()
                assert bool(torch.isfinite(j[b, :n]).all()) and bool(torch.isfinite(r[b, :n]).all()) and bool(torch.isfinite(o).all())
                j1, r1, o1 = P.motion_to_joints_fk(rows[b:b + 1, :n], g["mean"], g["std"], None, offsets, sigma=sigma,
                                                   return_rotations=True, return_offsets=True)
                assert torch.equal(j1[0], j[b, :n]) and torch.equal(r1[0], r[b, :n]) and torch.equal(o1[0], o[b]), (b, sigma)


@pytest.mark.parametrize("T", [300, 1, 2])
def test_more_frames_than_threads_and_the_shortest(T):
    P = pkg("postprocess")
    sk = TF.ref_skel("t2m")
    data = noisy_rows(sk, T, 17)
    mean, std = _mean_std(263, 22, 5)
    rows = ((data - mean) / std).astype(np.float32)[None]
    want = [FR.motion_to_joints_fk(sk, rows, mean, std, None, None, dtype=dt) for dt in (torch.float64, torch.float32)]
    j, r, o = P.motion_to_joints_fk(torch.from_numpy(rows).cuda(), mean, std, None, None, sigma=0.0, return_rotations=True,
                                    return_offsets=True)
    for got, k, what in ((j, 0, "joints"), (r, 1, "rotations"), (o, 2, "offsets")):
        yard = float(np.abs(want[1][k] - want[0][k]).max())
        err = float(np.abs(got.cpu().numpy() - want[0][k]).max())
        print(T, what, err, "yardstick", yard)
        assert err <= GATE * yard, (T, what, err, yard)


def test_frame_limit():
    P, L = pkg("postprocess"), pkg("_lib")
    most = P.fk_max_frames()
    with pytest.raises(ValueError, match="at most"):
        P.motion_to_joints_fk(torch.zeros(1, most + 1, 263, device="cuda"), np.zeros(263), np.ones(263))
    x = torch.zeros(1, most, 263, device="cuda")
    x[..., 67:193] = torch.tensor([1.0, 0, 0, 0, 1, 0], device="cuda").repeat(21)
    j = P.motion_to_joints_fk(x, np.zeros(263), np.ones(263), None, torch.ones(22, 3), sigma=0.0)
    assert j.shape == (1, most, 22, 3) and bool(torch.isfinite(j).all()) and float(j[0, -1, 21].abs().max()) > 0


def test_through_the_trainer():
    P = pkg("postprocess")
    tr = TF._tiny_trainer()
    sk = TF.ref_skel("t2m")
    mean, std = _mean_std(263, 22, 12)
    caps, lens = ["a", "b", "c", "d"], torch.tensor([16, 16, 12, 9])
    opts = dict(seed=0, sampler="ddim", sample_steps=5, batch_size=2)
    o = torch.from_numpy(golden("t2m_clean")["off"])
    motions = tr.generate(caps, lens, 263, **opts)
    x = torch.zeros(4, 16, 263, device="cuda")
    for i, (m, n) in enumerate(zip(motions, lens.tolist())):
        x[i, :n] = m[:n]
    fk = tr.generate_joints(caps, lens, 263, mean, std, from_rotations=True, offsets=o, **opts)
    want = P.motion_to_joints_fk(x, mean, std, lens, o)
    assert [tuple(j.shape) for j in fk] == [(n, 22, 3) for n in lens.tolist()]
    for i, n in enumerate(lens.tolist()):
        assert torch.equal(fk[i], want[i, :n])
    own = tr.generate_joints(caps, lens, 263, mean, std, from_rotations=True, **opts)
    want = P.motion_to_joints_fk(x, mean, std, lens, None)
    assert all(torch.equal(own[i], want[i, :n]) for i, n in enumerate(lens.tolist()))
    # the default is the old path, bit for bit
    old = P.motion_to_joints(x, mean, std, lens, 22, 1.0)
    new = tr.generate_joints(caps, lens, 263, mean, std, **opts)
    assert all(torch.equal(new[i], old[i, :n]) for i, n in enumerate(lens.tolist()))
    assert not torch.equal(new[0], fk[0])
    with pytest.raises(ValueError, match="from_rotations"):
        tr.generate_joints(caps, lens, 263, mean, std, offsets=o, **opts)
    # a long motion: rigid bones across the overlap
    scripts = [[("a", 16), ("b", 16)]]
    lopts = dict(overlap=4, seed=4, sampler="ddim", sample_steps=5)
    canvas = tr.generate_long(scripts, 263, **lopts)[0]
    lj = tr.generate_long_joints(scripts, 263, mean, std, sigma=0.0, from_rotations=True, offsets=o, **lopts)[0]
    assert lj.shape == (28, 22, 3) and torch.equal(lj, P.motion_to_joints_fk(canvas[None], mean, std, None, o, sigma=0.0)[0])
    data = canvas.cpu().numpy() * std + mean
    assert min(FR.gram_schmidt_margins(sk, data)) >= 0.2
    gate = _bone_gate(sk, data, o.numpy())
    err = float(np.abs(bone_lengths(lj.cpu().numpy(), sk) - np.linalg.norm(o.numpy().astype(np.float64)[1:], axis=-1)).max())
    print("long motion bones", err, "gate", gate)
    assert err <= gate
    # rotations
    res = tr.generate_rotations(caps, lens, 263, mean, std, **opts)
    for i, n in enumerate(lens.tolist()):
        jo, ro, of = res[i]
        assert jo.shape == (n, 22, 3) and ro.shape == (n, 22, 3, 3) and of.shape == (22, 3)
        assert torch.equal(jo, P.motion_to_joints_fk(x[i:i + 1, :n], mean, std, None, None, sigma=0.0)[0])
        data = x[i, :n].cpu().numpy() * std + mean
        assert min(FR.gram_schmidt_margins(sk, data)) >= 0.2
        r32 = FR.recover_from_rot(sk, data, of.cpu().numpy(), return_rotations=True)[1].astype(np.float64)
        gate = GATE * float(np.abs(np.einsum("tjab,tjac->tjbc", r32, r32) - np.eye(3)).max())
        r = ro.cpu().numpy().astype(np.float64)
        err = float(np.abs(np.einsum("tjab,tjac->tjbc", r, r) - np.eye(3)).max())
        print("generated rotations", i, "R^T R - I", err, "gate", gate)
        assert err <= gate and (np.linalg.det(r) > 0).all()


def test_bad_arguments_on_the_device_path():
    P, L = pkg("postprocess"), pkg("_lib")
    x = torch.zeros(2, 8, 263, device="cuda")
    mean, std = np.zeros(263), np.ones(263)
    with pytest.raises(ValueError):
        P.motion_to_joints_fk(x[..., :251], mean, std)                      # F of the other skeleton
    with pytest.raises(ValueError):
        P.motion_to_joints_fk(x, mean, std, None, torch.zeros(3, 22, 3, device="cuda"))
    with pytest.raises(ValueError):
        P.motion_to_joints_fk(x, mean, std, None, torch.zeros(22, 4))
    with pytest.raises(L.MdmError):
        P.motion_to_joints_fk(x.cpu(), mean, std)                           # a CPU tensor

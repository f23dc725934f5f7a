"""CPU: joints -> feature rows without a device.

* the package's skeleton tables equal the ones the reference ran with (recorded in tests/golden/motion_features.npz);
* the restatement tests/motion_features_ref.py, in the reference's precision mix, reproduces the golden's data and
  global_positions (the GPU tests lean on it), and its batch form pads and normalises as the device function does;
* Conditioning turns edit_joints into the edit_motion it gets from rows (conversion injected: no HIP library), and refuses
  edit_joints with edit_motion, without mean / std, and with a mask that reaches past a clip's rows;
* argument checks of joints_to_motion and of the C entry point that need no device; the frame limit covers every canvas
  generate_long_joints can return.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, pkg

import motion_features_ref as MR


def golden():
    z = np.load(os.path.join(GOLDEN, "motion_features.npz"))
    return z, json.loads(str(z["meta"]))


def ref_skeleton(z, meta, name):
    tb = meta[f"{name}_tables"]
    return MR.skeleton_from_tables(tb["chains"], z[f"{name}_raw_offsets"], tb["face"], tb["fid_l"] + tb["fid_r"], tb["legs"])


def ref_to_motion(clips, lengths, mean, std, *, skeleton="t2m", **kw):
    """joints_to_motion's signature on the CPU restatement (what Conditioning is handed in place of the HIP kernel)."""
    assert lengths is None
    z, meta = golden()
    rows, _ = MR.joints_to_motion(ref_skeleton(z, meta, skeleton), [c.cpu().numpy() for c in clips], mean, std)
    return torch.from_numpy(rows)


def test_skeleton_tables_equal_the_references():
    MF = pkg("motion_features")
    z, meta = golden()
    for name, J in (("t2m", 22), ("kit", 21)):
        sk, tb = MF.SKELETONS[name], meta[f"{name}_tables"]
        assert sk.joints == J and sk.feats == 12 * J - 1
        assert [list(c) for c in sk.chains] == tb["chains"]
        assert np.array_equal(sk.raw_offsets, z[f"{name}_raw_offsets"].astype(np.float32))
        assert list(sk.face) == tb["face"] and list(sk.feet) == tb["fid_l"] + tb["fid_r"] and list(sk.legs) == tb["legs"]
        assert list(sk.parents) == ref_skeleton(z, meta, name).parents
    assert {c["skel"]: c["feet_thre"] for c in meta["cases"]} == {n: MF.SKELETONS[n].feet_thre for n in ("t2m", "kit")}


def test_restatement_reproduces_the_reference():
    z, meta = golden()
    assert [c["n"] for c in meta["cases"]] == [120, 41, 2, 60]
    for case in meta["cases"]:
        n = case["name"]
        sk = ref_skeleton(z, meta, case["skel"])
        tgt = z[f"{n}_target_offsets"] if f"{n}_target_offsets" in z.files else None
        data, glob = MR.process_file(sk, z[f"{n}_joints"], case["feet_thre"], tgt, all32=False)
        want = z[f"{n}_data"]
        assert data.shape == want.shape == (case["n"] - 1, 12 * sk.J - 1)
        assert np.abs(glob - z[f"{n}_global_positions"]).max() <= 1e-6
        assert np.abs(data[:, :-4] - want[:, :-4]).max() <= 1e-6
        assert np.array_equal(data[:, -4:], want[:, -4:])
        assert case["margin"] >= meta["min_margin"]
        again = MR.extract_features(sk, z[f"{n}_global_positions"], case["feet_thre"])[0]
        assert np.abs(again - want).max() <= 1e-6
        if tgt is not None:  # skeleton_offsets is get_offsets_joints
            MF = pkg("motion_features")
            pose = MR.synth_clip(sk, 2, case["tgt_seed"])[0]
            assert np.abs(MF.skeleton_offsets(pose, case["skel"]).numpy() - tgt).max() <= 1e-7


def test_restatement_batch_form_pads_and_normalises():
    z, meta = golden()
    sk = ref_skeleton(z, meta, "t2m")
    clips = [MR.synth_clip(sk, n, 40 + n) for n in (9, 2, 5)]
    mean, std = np.linspace(-1, 1, 263).astype(np.float32), np.linspace(0.5, 2, 263).astype(np.float32)
    rows, pos = MR.joints_to_motion(sk, clips, mean, std)
    assert rows.shape == (3, 8, 263) and pos.shape == (3, 9, 22, 3)
    assert not rows[1, 1:].any() and not rows[2, 4:].any() and not pos[1, 2:].any()
    one = MR.process_file(sk, clips[2], 0.002, all32=True)[0].astype(np.float32)
    assert np.array_equal(rows[2, :4], (one - mean) / std)


def _clips(ns, seed=70):
    z, meta = golden()
    sk = ref_skeleton(z, meta, "t2m")
    return [torch.from_numpy(MR.synth_clip(sk, n, seed + i)).float() for i, n in enumerate(ns)]


def test_conditioning_converts_edit_joints_once():
    Cn, E = pkg("conditioning"), pkg("motion_edit")
    clips = _clips([9, 13, 7])
    mean, std = torch.linspace(-1, 1, 263), torch.linspace(0.5, 2, 263)
    T = 16
    mask = torch.stack([E.prefix_mask(T, n - 1) for n in (9, 13, 7)])
    calls = []

    def to_motion(*a, **k):
        calls.append(1)
        return ref_to_motion(*a, **k)

    caps = ["a", "b", "c"]
    c = Cn.Conditioning(caps, 263, edit_mask=mask, mean=mean, std=std, edit_joints=clips, to_motion=to_motion)
    rows = ref_to_motion(clips, None, mean, std)
    want = Cn.Conditioning(caps, 263, edit_motion=Cn.pad_frames(rows, T), edit_mask=mask)
    assert len(calls) == 1
    for sl, t in ((slice(0, 2), 12), (slice(2, 3), 16), (torch.tensor([2, 0]), 8)):
        a, b = c.edit_kwargs(sl, t), want.edit_kwargs(sl, t)
        assert torch.equal(a["inpaint_motion"], b["inpaint_motion"]) and torch.equal(a["inpaint_mask"], b["inpaint_mask"])
        assert a["inpaint_motion"].shape[1] == t
    assert len(calls) == 1
    k = c.edit[0]
    assert k.shape == (3, T, 263) and not k[2, 6:].any() and k[2, :6].abs().sum() > 0
    # a padded tensor of equally long clips is taken as well
    same = torch.stack(_clips([9, 9]))
    c2 = Cn.Conditioning(caps[:2], 263, edit_mask=E.prefix_mask(T, 8), mean=mean, std=std, edit_joints=same, to_motion=ref_to_motion)
    assert torch.equal(c2.edit[0][:, :8], ref_to_motion(list(same), None, mean, std))


def test_conditioning_refuses_bad_edit_joints():
    Cn, E = pkg("conditioning"), pkg("motion_edit")
    clips = _clips([9, 13])
    mean, std = torch.zeros(263), torch.ones(263)
    T = 16
    ok = torch.stack([E.prefix_mask(T, 8), E.prefix_mask(T, 12)])
    kw = dict(mean=mean, std=std, edit_joints=clips, to_motion=ref_to_motion)
    Cn.Conditioning(["a", "b"], 263, edit_mask=ok, **kw)
    with pytest.raises(ValueError, match="exclusive"):
        Cn.Conditioning(["a", "b"], 263, edit_motion=torch.zeros(2, T, 263), edit_mask=ok, **kw)
    with pytest.raises(ValueError, match="mean and std"):
        Cn.Conditioning(["a", "b"], 263, edit_mask=ok, edit_joints=clips, to_motion=ref_to_motion)
    with pytest.raises(ValueError, match="mean and std"):
        Cn.Conditioning(["a", "b"], 263, edit_mask=ok, edit_joints=clips, mean=mean, to_motion=ref_to_motion)
    with pytest.raises(ValueError, match="go together"):
        Cn.Conditioning(["a", "b"], 263, **kw)
    for bad in (torch.stack([E.prefix_mask(T, 9), E.prefix_mask(T, 12)]),       # frame n - 1 of clip 0
                torch.stack([E.prefix_mask(T, 8), E.inbetween_mask(T, 3, 1)])):  # the canvas's last frame of clip 1
        with pytest.raises(ValueError, match="one frame short"):
            Cn.Conditioning(["a", "b"], 263, edit_mask=bad, **kw)
    with pytest.raises(ValueError, match="263"):
        Cn.Conditioning(["a", "b"], 100, edit_mask=ok, **kw)
    with pytest.raises(ValueError, match="covers 10 frames"):  # clip 1 gives 12 rows
        Cn.Conditioning(["a", "b"], 263, edit_mask=E.prefix_mask(10, 4), **kw)
    with pytest.raises(ValueError, match="more dims"):
        Cn.Conditioning(["a", "b"], 263, edit_mask=ok[None], **kw)
    c = Cn.Conditioning(["a", "b"], 263, edit_mask=E.joint_feature_mask(E.UPPER_BODY) * 0, **kw)  # a mask without frames
    assert c.edit[0].shape == (2, 12, 263)


def test_joints_to_motion_argument_checks_need_no_device():
    MF, L = pkg("motion_features"), pkg("_lib")
    good = _clips([6])[0][None]
    bad_args = [
        (dict(joints=good[:, :, :20]), "must be"),                          # J = 20
        (dict(joints=good[:, :1]), "at least 2 frames"),
        (dict(joints=good, mean=np.zeros(263)), "go together"),
        (dict(joints=good, mean=np.zeros(262), std=np.ones(262)), "263 entries"),
        (dict(joints=good, mean=np.zeros(263), std=np.zeros(263)), "zero"),
        (dict(joints=torch.full_like(good, float("nan"))), "non-finite"),
        (dict(joints=good, lengths=[7]), "lengths|length"),
        (dict(joints=good, lengths=[1]), "lengths|length"),
        (dict(joints=[good[0], good[0, :, :21]]), "clip 1"),
        (dict(joints=good, skeleton="smplx"), "skeleton"),
        (dict(joints=good, canonicalize=False, target_offsets=torch.zeros(22, 3)), "canonicalize"),
        (dict(joints=good, target_offsets=torch.zeros(21, 3)), "target_offsets"),
        (dict(joints=good, skeleton="kit"), "must be"),
    ]
    for kw, msg in bad_args:
        kw = dict(kw)
        with pytest.raises(ValueError, match=msg):
            MF.joints_to_motion(kw.pop("joints"), kw.pop("lengths", None), kw.pop("mean", None), kw.pop("std", None), **kw)
    nan_tail = torch.cat([good, torch.full_like(good, float("nan"))], dim=1)
    with pytest.raises(L.MdmError):  # frames past the length are not read; a CPU tensor has no kernel to go to
        MF.joints_to_motion(nan_tail, [6])
    with pytest.raises(L.MdmError):  # the frame limit is the entry point's to refuse (below); no device here
        MF.joints_to_motion(torch.zeros(1, MF.max_frames() + 1, 22, 3))
    with pytest.raises(ValueError):
        MF.skeleton_offsets(torch.zeros(21, 3))


def test_entry_point_checks_and_frame_limit():
    MF, L, Tr = pkg("motion_features"), pkg("_lib"), pkg("trainer")
    lib = L.lib()
    assert lib.mdm_motion_features_max_frames() == MF.max_frames() >= Tr.MAX_JOINTS_FRAMES
    sk = MF._skeleton_struct(MF.SKELETONS["t2m"])
    p = C.c_void_p(64)  # never dereferenced: every call below is refused before a launch

    def call(skel, T, joints=p, out=p, pos=p, canon=1, tgt=None, mean=None, std=None):
        return lib.mdm_motion_features(joints, None, mean, std, C.byref(skel) if skel else None, tgt, C.c_int32(1), C.c_int32(T),
                                       C.c_double(0.002), C.c_int32(canon), C.c_int32(0), None, pos, out, None)

    assert call(sk, MF.max_frames() + 1) == 3   # MDM_ERR_UNSUPPORTED
    assert call(sk, 1) == 1 and call(None, 8) == 1 and call(sk, 8, joints=None) == 1 and call(sk, 8, out=None) == 1
    assert call(sk, 8, pos=None) == 1 and call(sk, 8, canon=0, tgt=p) == 1 and call(sk, 8, mean=p) == 1
    for field, idx, val in (("chain_joints", 3, 22), ("chain_joints", 7, -1), ("face", 0, 22), ("feet", 3, 40), ("legs", 0, 0),
                            ("chain_joints", 6, 5), ("chain_offsets", 1, 1), ("chain_joints", 15, 20)):
        bad = MF._skeleton_struct(MF.SKELETONS["t2m"])
        getattr(bad, field)[idx] = val
        assert call(bad, 8) == 1, (field, idx, val)
    bad = MF._skeleton_struct(MF.SKELETONS["t2m"])
    bad.joints = 33
    assert call(bad, 8) == 1

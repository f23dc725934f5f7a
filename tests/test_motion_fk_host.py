"""CPU: rows -> joints by forward kinematics without a device.

* the fp32 form of the restatement tests/motion_fk_ref.py reproduces the reference's recover_from_rot output recorded in
  tests/golden/motion_fk.npz within the recorded yardstick (the reference's own fp32 error against the fp64 restatement), and
  the golden's fp64 arrays are the restatement's;
* the golden keeps the conditioning bound of its generator, and every wrong variant of the restatement lies at least
  4 gates (a gate: GATE x yardstick, as tests/test_motion_fk_gpu.py uses it) from the truth on the golden's inputs: the
  golden can see each of these mistakes;
* argument checks of motion_to_joints_fk / recover_from_rot / the trainer switch and of the C entry point that need no device.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, pkg

import motion_features_ref as MR
import motion_fk_ref as FR

GATE = 4.0


def golden():
    z = np.load(os.path.join(GOLDEN, "motion_fk.npz"))
    return z, json.loads(str(z["meta"]))


def ref_skel(name):
    sk = pkg("motion_features").SKELETONS[name]  # equal to the reference's tables: tests/test_motion_features_host.py
    return MR.skeleton_from_tables(sk.chains, sk.raw_offsets, sk.face, sk.feet, sk.legs)


def case_inputs(z, meta, case):
    """-> skeleton, normalised rows (B, T, F), mean, std, lengths, shared offsets, first valid-frame index per sample."""
    s = case["skel"]
    lens = meta["lengths"]
    return ref_skel(s), z[f"{case['name']}_rows"], z[f"{s}_mean"], z[f"{s}_std"], lens, z[f"{s}_offsets"], np.cumsum([0] + lens)


def test_golden_shape_and_conditioning():
    z, meta = golden()
    assert [c["name"] for c in meta["cases"]] == ["t2m_clean", "t2m_noisy", "kit_clean", "kit_noisy"]
    assert meta["T"] == 24 and sorted(meta["lengths"]) == [1, 2, 24]
    for case in meta["cases"]:
        sk, rows, mean, std, lens, off, at = case_inputs(z, meta, case)
        assert rows.shape == (3, 24, 12 * sk.J - 1) and rows.dtype == np.float32 and off.shape == (sk.J, 3)
        assert z[f"{case['name']}_ref_joints"].shape == (sum(lens), sk.J, 3)
        for b, n in enumerate(lens):
            nx, nc = FR.gram_schmidt_margins(sk, rows[b, :n] * std + mean)
            assert nx >= meta["min_norm"] and nc >= meta["min_norm"], (case["name"], b, nx, nc)
            assert not rows[b, n:].any()
        if case["kind"] == "noisy":  # not orthonormal, as a network's output is not
            assert case["min_x"] < 0.9 and case["min_cross"] < 0.9


def test_restatement_reproduces_the_reference():
    z, meta = golden()
    for case in meta["cases"]:
        sk, rows, mean, std, lens, off, at = case_inputs(z, meta, case)
        y = case["yardstick"]
        j32, r32, _ = FR.motion_to_joints_fk(sk, rows, mean, std, lens, off)
        j64, r64, _ = FR.motion_to_joints_fk(sk, rows, mean, std, lens, off, dtype=torch.float64)
        _, _, o64 = FR.motion_to_joints_fk(sk, rows, mean, std, lens, None, dtype=torch.float64)
        _, _, o32 = FR.motion_to_joints_fk(sk, rows, mean, std, lens, None)
        for b, n in enumerate(lens):
            sl = slice(at[b], at[b] + n)
            want = z[f"{case['name']}_ref_joints"][sl]
            assert np.abs(j32[b, :n] - want).max() <= y["joints"], (case["name"], b)
            assert np.array_equal(j64[b, :n], z[f"{case['name']}_joints64"][sl])
            assert np.array_equal(r64[b, :n], z[f"{case['name']}_rotations64"][sl])
            assert np.abs(want - j64[b, :n]).max() <= y["joints"]
            assert np.abs(r32[b, :n] - r64[b, :n]).max() <= y["rotations"]
            assert not j32[b, n:].any() and not r32[b, n:].any()
            # the truth's rotations are rotations, and its bones have the offsets' lengths
            eye = np.einsum("tjab,tjac->tjbc", r64[b, :n], r64[b, :n]) - np.eye(3)
            assert np.abs(eye).max() < 1e-12 and (np.linalg.det(r64[b, :n]) > 0).all()
            par = np.asarray(sk.parents[1:])
            bones = np.linalg.norm(j64[b, :n, 1:] - j64[b, :n][:, par], axis=-1)
            assert np.abs(bones - np.linalg.norm(off[1:], axis=-1)).max() < 1e-12
        assert np.array_equal(o64, z[f"{case['name']}_offsets64"])
        assert np.abs(o32 - o64).max() <= y["offsets"]
        assert 0 < y["joints"] < 1e-6 and 0 < y["rotations"] < 1e-6 and 0 < y["offsets"] < 1e-6


def test_the_golden_sees_every_wrong_variant():
    z, meta = golden()
    assert len(FR.WRONG) == 6
    for case in meta["cases"]:
        sk, rows, mean, std, lens, off, at = case_inputs(z, meta, case)
        gate = GATE * case["yardstick"]["joints"]
        for wrong in FR.WRONG:
            j, _, _ = FR.motion_to_joints_fk(sk, rows, mean, std, lens, off, wrong=wrong)
            err = max(float(np.abs(j[b, :n] - z[f"{case['name']}_ref_joints"][at[b]:at[b] + n]).max()) for b, n in enumerate(lens))
            print(case["name"], wrong, f"{err:.3g}", "gate", f"{gate:.3g}")
            assert err >= 4 * gate, (case["name"], wrong, err, gate)


def test_argument_checks_need_no_device():
    P, L = pkg("postprocess"), pkg("_lib")
    good = torch.zeros(2, 6, 263)
    mean, std = np.zeros(263), np.ones(263)
    bad_args = [
        (dict(motion=good[..., :262]), "263"),
        (dict(motion=good, skeleton="kit"), "251"),
        (dict(motion=good, skeleton="smplx"), "skeleton"),
        (dict(motion=good, mean=np.zeros(262)), "263 entries"),
        (dict(motion=good, std=np.zeros(263)), "zero"),
        (dict(motion=good, std=np.full(263, np.nan)), "non-finite"),
        (dict(motion=good, lengths=[6]), "2 entries"),
        (dict(motion=good, lengths=[0, 6]), "length"),
        (dict(motion=good, lengths=[6, 7]), "length"),
        (dict(motion=good, offsets=torch.zeros(21, 3)), "offsets"),
        (dict(motion=good, offsets=torch.zeros(3, 22, 3)), "offsets"),
        (dict(motion=good, offsets=torch.full((22, 3), float("inf"))), "offsets"),
        (dict(motion=torch.zeros(1, P.fk_max_frames() + 1, 263)), "at most"),
        (dict(motion=good[:, :0]), "at least 1 frame"),
    ]
    for kw in bad_args:
        kw, msg = dict(kw[0]), kw[1]
        with pytest.raises(ValueError, match=msg):
            P.motion_to_joints_fk(kw.pop("motion"), kw.pop("mean", mean), kw.pop("std", std), kw.pop("lengths", None),
                                  kw.pop("offsets", None), **kw)
    with pytest.raises(L.MdmError):  # well-formed arguments on the CPU: there is no eager fallback
        P.motion_to_joints_fk(good, mean, std, [6, 1], torch.zeros(2, 22, 3))
    with pytest.raises(ValueError, match="joints_num"):
        P.recover_from_rot(good, 24, torch.zeros(24, 3))
    with pytest.raises(ValueError, match="not 22"):
        P.recover_from_rot(good, 22, torch.zeros(22, 3), skeleton="kit")
    with pytest.raises(L.MdmError):
        P.recover_from_rot(good, 22, torch.zeros(22, 3))
    MO = pkg("motion_outputs")
    with pytest.raises(ValueError, match="from_rotations"):
        MO.to_joints([good[0]], [6], 263, mean, std, 22, 1.0, offsets=torch.zeros(22, 3))
    with pytest.raises(ValueError, match="dim_pose"):
        MO.to_joints([torch.zeros(6, 100)], [6], 100, mean, std, 22, 1.0, from_rotations=True)


def test_entry_point_checks_and_frame_limit():
    MF, P, L = pkg("motion_features"), pkg("postprocess"), pkg("_lib")
    lib = L.lib()
    assert lib.mdm_motion_fk_max_frames() == P.fk_max_frames() >= 3000
    sk = MF._skeleton_struct(MF.SKELETONS["t2m"])
    p = C.c_void_p(64)  # never dereferenced: every call below is refused before a launch

    def call(skel, T, F=263, motion=p, mean=p, std=p, off=p, scratch=p, out=p, radius=0, w=None):
        return lib.mdm_motion_fk(motion, None, mean, std, C.byref(skel) if skel else None, off, C.c_int32(0), C.c_int32(1),
                                 C.c_int32(T), C.c_int32(F), C.c_int32(radius), w, scratch, out, None, None, None)

    assert call(sk, P.fk_max_frames() + 1) == 3   # MDM_ERR_UNSUPPORTED
    assert call(sk, 0) == 1 and call(None, 8) == 1 and call(sk, 8, motion=None) == 1 and call(sk, 8, out=None) == 1
    assert call(sk, 8, mean=None) == 1 and call(sk, 8, std=None) == 1 and call(sk, 8, F=251) == 1 and call(sk, 8, F=264) == 1
    assert call(sk, 8, off=None, scratch=None) == 1 and call(sk, 8, radius=2, scratch=None, w=p) == 1
    assert call(sk, 8, radius=2) == 1 and call(sk, 8, radius=-1) == 1
    assert call(MF._skeleton_struct(MF.SKELETONS["kit"]), P.fk_max_frames() + 1, F=251) == 3
    for field, idx, val in (("chain_joints", 3, 22), ("chain_joints", 7, -1), ("chain_joints", 6, 5), ("chain_offsets", 1, 1),
                            ("chain_joints", 15, 20)):
        bad = MF._skeleton_struct(MF.SKELETONS["t2m"])
        getattr(bad, field)[idx] = val
        assert call(bad, 8) == 1, (field, idx, val)

"""CPU: the rig export's host side and its restatement, on tests/golden/motion_fk.npz.

* the inputs satisfy joint[c] = joint[p] + R[c] offset[c], which is all the export relies on;
* rig_of: node counts, every joint at one node, helpers exactly at the branching joints, parents first;
* fp64 round trip restatement channels -> bvh_text -> BVH reader -> the input joints, all six Euler orders; the text parsed to
  fp32 is the fp32 channel tensor bit for bit;
* each of six wrong variants lies >= 1e4 gates from the truth, from the restatement alone;
* the gimbal; argument checks without a device, in Python and at the C entry.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, pkg

import rig_ref as RR

LENS = [24, 2, 1]
AT = np.cumsum([0] + LENS)
CASES = ("t2m_clean", "t2m_noisy", "kit_clean", "kit_noisy")
GATE = 4.0


def golden(name):
    """-> (skeleton name, offsets fp32 (J, 3), joints fp64 per sample, rotations fp64 per sample)."""
    z = np.load(os.path.join(GOLDEN, "motion_fk.npz"))
    skel = name.split("_")[0]
    j, R = z[f"{name}_joints64"], z[f"{name}_rotations64"]
    return (skel, z[f"{skel}_offsets"], [j[AT[b]:AT[b] + n] for b, n in enumerate(LENS)],
            [R[AT[b]:AT[b] + n] for b, n in enumerate(LENS)])


def branching(sk):
    return sorted(p for p in range(sk.joints) if sum(1 for q in sk.parents[1:] if q == p) > 1)


@pytest.mark.parametrize("name", CASES)
def test_inputs_satisfy_the_precondition(name):
    skel, off, joints, rots = golden(name)
    sk = pkg("motion_features").SKELETONS[skel]
    for j, R in zip(joints, rots):
        for c in range(1, sk.joints):
            p = sk.parents[c]
            assert np.abs(j[:, c] - j[:, p] - R[:, c] @ off[c].astype(np.float64)).max() <= 1e-12, (name, c)


def test_rig_of():
    MRig, MF = pkg("motion_rig"), pkg("motion_features")
    for skel, nodes in (("t2m", 28), ("kit", 27)):
        sk, rig = MF.SKELETONS[skel], MRig.rig_of(skel)
        N = rig.n_nodes
        assert N == nodes and all(len(getattr(rig, k)) == N for k in ("names", "parent", "carried", "joint_of", "has_offset"))
        assert sorted(j for j in rig.joint_of if j >= 0) == list(range(sk.joints))      # every joint at exactly one node
        assert rig.parent[0] == -1 and rig.joint_of[0] == 0 and not rig.has_offset[0]
        assert all(0 <= rig.parent[n] < n for n in range(1, N))                          # parents first
        assert len(set(rig.names)) == N
        helpers = [n for n in range(N) if rig.joint_of[n] < 0]
        assert sorted({rig.joint_of[rig.parent[n]] for n in helpers}) == branching(sk)   # helpers exactly at the branching joints
        for n in range(N):
            j, kids = rig.joint_of[n], [m for m in range(N) if rig.parent[m] == n]
            if j < 0:  # a helper: no offset, carries its one child's R, the child sits below with its own offset
                (m,) = kids
                assert not rig.has_offset[n] and rig.carried[n] == rig.joint_of[m] and rig.has_offset[m]
                assert sk.parents[rig.joint_of[m]] == rig.joint_of[rig.parent[n]]
                assert rig.names[n] == f"{rig.names[rig.parent[n]]}_to_{rig.names[m]}"
                continue
            below = [c for c in range(sk.joints) if sk.parents[c] == j and c > 0]
            if len(below) == 1:
                assert rig.carried[n] == below[0] and [rig.joint_of[m] for m in kids] == below
            elif below:
                assert rig.carried[n] == j and all(rig.joint_of[m] < 0 for m in kids) and len(kids) == len(below)
            else:
                assert rig.carried[n] == -1 and not kids
    assert MRig.rig_of("t2m").names[0] == "pelvis" and "spine3_to_left_collar" in MRig.rig_of("t2m").names
    assert MRig.rig_of("kit").names[:2] == ["joint_00", "joint_00_to_joint_11"]
    assert MRig.rig_of(MF.SKELETONS["kit"]).parent == MRig.rig_of("kit").parent


@pytest.mark.parametrize("name", CASES)
def test_round_trip_in_fp64(name):
    MRig = pkg("motion_rig")
    skel, off, joints, rots = golden(name)
    rig = MRig.rig_of(skel)
    worst = 0.0
    for order in RR.ORDERS:
        for j, R, n in zip(joints, rots, LENS):
            chan, _ = RR.rig_channels(rig, j, R, order)
            assert chan.shape == (n, 3 + 3 * rig.n_nodes)
            text = MRig.bvh_text(rig, off, chan, n, 0.05, euler=order)
            bvh = RR.parse_bvh(text)
            assert bvh.frames == n and bvh.frame_time == 0.05 and bvh.names == rig.names and bvh.parent == rig.parent
            assert all(c[-3:] == [a + "rotation" for a in order] for c in bvh.channels)
            assert bvh.channels[0][:3] == ["Xposition", "Yposition", "Zposition"] and all(len(c) == 3 for c in bvh.channels[1:])
            leaves = [m for m in range(rig.n_nodes) if m not in rig.parent]
            assert sorted(bvh.end_sites) == leaves and all(np.linalg.norm(v) > 0 for v in bvh.end_sites.values())
            got, G = RR.read_back(text, rig)
            worst = max(worst, float(np.abs(got - j).max()))
            assert np.abs(G - RR.global_rotations(rig, R)).max() <= 1e-12
            # channels of the leaves: zeros
            assert not chan[:, [3 + 3 * m + e for m in leaves for e in range(3)]].any()
            # the fp32 tensor comes back bit for bit from its text
            c32 = RR.rig_channels(rig, j, R, order, dtype=np.float32)[0]
            assert np.array_equal(RR.parse_bvh(MRig.bvh_text(rig, off, c32, n, 0.05, euler=order), np.float32).values, c32)
    print(name, "fp64 round trip", worst)
    assert worst <= 1e-12


def test_bvh_text_details(tmp_path):
    MRig = pkg("motion_rig")
    skel, off, joints, rots = golden("t2m_noisy")
    rig = MRig.rig_of(skel)
    chan = RR.rig_channels(rig, joints[0], rots[0], "ZXY", scale=100.0, dtype=np.float32)[0]
    text = MRig.bvh_text(rig, off, torch.from_numpy(chan), 7, 1 / 30, scale=100.0, end_site=0.1)
    bvh = RR.parse_bvh(text, np.float32)
    assert bvh.frames == 7 and np.array_equal(bvh.values, chan[:7]) and abs(bvh.frame_time - 1 / 30) < 1e-9
    at = {j: n for n, j in enumerate(rig.joint_of) if j >= 0}
    for j in range(1, 22):
        assert np.abs(bvh.offsets[at[j]] - 100.0 * off[j].astype(np.float64)).max() <= 1e-5
    assert not bvh.offsets[[n for n in range(rig.n_nodes) if not rig.has_offset[n]]].any()
    for n, v in bvh.end_sites.items():  # the leaf's own bone, continued for end_site * scale
        o = off[rig.joint_of[n]].astype(np.float64)
        assert np.abs(v - 10.0 * o / np.linalg.norm(o)).max() < 1e-5
    zero = MRig.bvh_text(rig, np.zeros((22, 3)), chan, 1, 0.05, scale=100.0)
    assert all(np.array_equal(v, [0, 5, 0]) for v in RR.parse_bvh(zero).end_sites.values())
    path = tmp_path / "a.bvh"
    assert MRig.write_bvh(str(path), rig, off, chan, 7, 1 / 30, scale=100.0, end_site=0.1) == text == path.read_text()
    for bad in (dict(channels=chan[:, :-1]), dict(n_frames=25), dict(frame_time=0.0), dict(offsets=off[:21]), dict(euler="XYX")):
        kw = dict(rig=rig, offsets=off, channels=chan, n_frames=7, frame_time=0.05)
        kw.update(bad)
        with pytest.raises(ValueError):
            MRig.bvh_text(**kw)


def _variant_distance(MRig, rig, off, joints, rots, lens, variant, **kw):
    """How many gates the variant's read-back lies from the truth's: the larger of joints and global rotations."""
    truth, yj, yg = RR.yardstick(MRig.bvh_text, rig, off, joints, rots, lens, **kw)
    ej = eg = 0.0
    for b, n in enumerate(lens):
        r2 = RR.without_helpers(rig) if variant == "without_helpers" else rig
        chan = RR.rig_channels(r2, joints[b][:n], rots[b][:n], variant=None if r2 is not rig else variant, **kw)[0]
        j, G = RR.read_back(MRig.bvh_text(r2, off, chan, len(chan), 0.05), r2)
        ej = max(ej, float(np.abs(j - truth[b][0]).max()))
        if r2 is rig:
            eg = max(eg, float(np.abs(G - truth[b][1]).max()))
    return max(ej / (GATE * yj), eg / (GATE * yg)), yj, yg


@pytest.mark.parametrize("variant", ["without_helpers", "right_division", "reversed", "radians", "arms_from_root"])
def test_wrong_variants_lie_far_from_the_truth(variant):
    MRig = pkg("motion_rig")
    for name in CASES:
        skel, off, joints, rots = golden(name)
        gates, yj, yg = _variant_distance(MRig, MRig.rig_of(skel), off, joints, rots, LENS, variant)
        print(variant, name, f"{gates:.3g} gates (yardsticks {yj:.3g}, {yg:.3g})")
        assert gates >= 1e4, (variant, name, gates)


def flip_clip(MRig):
    """t2m, 6 frames: the right shoulder's local angle runs from 170 to 190 degrees about a fixed axis."""
    off = np.load(os.path.join(GOLDEN, "motion_fk.npz"))["t2m_offsets"]
    rig = MRig.rig_of("t2m")
    node = rig.names.index("right_shoulder")
    return (rig, off, node) + RR.spin_clip(rig, off, 6, 3, turning=node)


def test_slerp_without_the_hemisphere_flip_lies_far_from_the_truth():
    MRig = pkg("motion_rig")
    rig, off, node, j, R, local_at = flip_clip(MRig)
    q = RR.matrix_to_quaternion(RR.local_rotations(rig, R))[:, node]
    assert (np.sum(q[:-1] * q[1:], -1) < 0).sum() == 1                  # the canonical quaternion changes sign once
    gates, yj, yg = _variant_distance(MRig, rig, off, [j], [R], [6], "no_flip", num=3, den=1)
    print("no_flip", f"{gates:.3g} gates (yardsticks {yj:.3g}, {yg:.3g})")
    assert gates >= 1e4
    # and the restated slerp is the motion itself on this clip
    chan, qk = RR.rig_channels(rig, j, R, num=3, den=1)
    assert len(chan) == 16
    want = np.stack([local_at(k / 3)[0] for k in range(16)])
    assert np.abs(RR.quaternion_to_matrix(qk) - want).max() <= 1e-12
    assert np.abs(chan[:, :3] - np.stack([local_at(k / 3)[1] for k in range(16)])).max() <= 1e-12


def test_gimbal():
    for order in RR.ORDERS:
        for b in (90.0, -90.0):
            for a, c in ((0.0, 0.0), (25.0, -70.0), (-160.0, 130.0)):
                M = RR.euler_to_matrix(np.deg2rad(np.array([a, b, c])), order)
                ang = RR.matrix_to_euler(M, order)
                assert ang[2] == 0.0 and abs(abs(np.rad2deg(ang[1])) - 90.0) < 1e-6
                assert np.abs(RR.euler_to_matrix(ang, order) - M).max() <= 1e-12, (order, a, b, c)
    rs = np.random.RandomState(0)  # and away from it, the angles themselves
    for order in RR.ORDERS:
        ang = np.deg2rad(rs.uniform([-180, -89, -180], [180, 89, 180], (200, 3)))
        assert np.abs(RR.matrix_to_euler(RR.euler_to_matrix(ang, order), order) - ang).max() <= 1e-12


def test_retime_ratio_and_lengths():
    MRig = pkg("motion_rig")
    assert MRig.retime_ratio("t2m", None, None)[:2] == (1, 1)
    assert MRig.retime_ratio("t2m", None, 30)[:2] == (3, 2) and MRig.retime_ratio("t2m", None, 60)[:2] == (3, 1)
    assert MRig.retime_ratio("t2m", None, 10)[:2] == (1, 2) and MRig.retime_ratio("t2m", None, 20.0)[:2] == (1, 1)
    assert MRig.retime_ratio("kit", None, 30)[:2] == (12, 5) and MRig.retime_ratio("kit", 25, 29.97)[:2] == (2997, 2500)
    j, r = torch.zeros(3, 24, 22, 3), torch.zeros(3, 24, 22, 3, 3)
    for fps_out, num, den in ((None, 1, 1), (30, 3, 2), (60, 3, 1), (10, 1, 2)):
        out = MRig.check_rig(j, r, LENS, "t2m", fps_out=fps_out)
        assert out[5:7] == (num, den) and out[7].tolist() == [(n - 1) * num // den + 1 for n in LENS]
    assert MRig.check_rig(j, r, None, "t2m", fps_out=30)[7].tolist() == [35, 35, 35]


def test_argument_checks_without_a_device():
    MRig, MF, L = pkg("motion_rig"), pkg("motion_features"), pkg("_lib")
    j, r = torch.zeros(2, 8, 22, 3), torch.zeros(2, 8, 22, 3, 3)
    bad = [dict(joints=j[:, :, :21]), dict(rotations=r[:, :7]), dict(rotations=r[..., :2]), dict(skeleton="kit"),
           dict(euler="XYX"), dict(euler="zx"), dict(euler=None), dict(fps_out=0), dict(fps_out=-30), dict(fps_out=float("nan")),
           dict(fps=0, fps_out=30), dict(lengths=[8, 9]), dict(lengths=[0, 8]), dict(lengths=[8]), dict(scale=float("inf")),
           dict(joints=j[:, :0], rotations=r[:, :0])]
    for kw in bad:
        args = dict(joints=j, rotations=r, lengths=None, skeleton="t2m")
        args.update(kw)
        with pytest.raises(ValueError):
            MRig.check_rig(**args)
        with pytest.raises(ValueError):  # the public function refuses the same before it asks for a device
            MRig.rotations_to_rig(args.pop("joints"), args.pop("rotations"), args.pop("lengths"), **args)
    with pytest.raises(L.MdmError):
        MRig.rotations_to_rig(j, r)  # CPU tensors: no eager fallback
    # a skeleton of its own: names joint_00 .., fps required with fps_out, and more than 64 nodes refused
    star = MF._skeleton([[0, c] for c in range(1, 8)], np.zeros((8, 3)), (1, 2, 3, 4), (1, 2, 3, 4), (1, 2), 0.002)
    rig = MRig.rig_of(star)
    assert rig.n_nodes == 15 and rig.names[:3] == ["joint_00", "joint_00_to_joint_01", "joint_01"]
    with pytest.raises(ValueError, match="fps"):
        MRig.check_rig(torch.zeros(1, 4, 8, 3), torch.zeros(1, 4, 8, 3, 3), None, star, fps_out=30)
    assert MRig.check_rig(torch.zeros(1, 4, 8, 3), torch.zeros(1, 4, 8, 3, 3), None, star, fps=24, fps_out=30)[5:7] == (5, 4)
    big = MF._skeleton([[0, c] for c in range(1, 34)], np.zeros((34, 3)), (1, 2, 3, 4), (1, 2, 3, 4), (1, 2), 0.002)
    with pytest.raises(ValueError, match="64"):
        MRig.rig_of(big)  # 34 joints + 33 helpers


def test_entry_refuses_bad_arguments_before_the_device():
    """mdm_rig_channels returns MDM_ERR_ARG for null pointers, malformed tables and bad ratios without touching a device."""
    L = pkg("_lib")
    if not os.path.exists(L.LIB_PATH):
        pkg("build").build(verbose=False)
    lib = L.lib()
    buf = (C.c_float * 16)()
    p = C.addressof(buf)

    def call(parent=(-1, 0, 1), carried=(0, 1, -1), axes=(2, 0, 1), num=1, den=1, T=4, T_out=4, J=2, B=0, joints=p, rot=p, out=p,
             tables=True):
        n = len(parent)
        par, car = (C.c_int32 * n)(*parent), (C.c_int32 * n)(*carried)
        return lib.mdm_rig_channels(joints, rot, None, B, T, J, n, par if tables else None, car, axes[0], axes[1], axes[2], 1.0,
                                    num, den, T_out, None, out, None, None)

    assert call() == 0                                   # well formed, nothing to do
    for kw in (dict(joints=None), dict(rot=None), dict(out=None), dict(tables=False), dict(num=0), dict(den=0), dict(num=-3),
               dict(parent=(-1, 1, 1)), dict(parent=(-1, 0, 2)), dict(parent=(0, 0, 1)), dict(parent=(-1, -1, 0)),
               dict(carried=(0, 2, -1)), dict(carried=(0, -2, 1)), dict(axes=(0, 0, 1)), dict(axes=(0, 1, 3)), dict(axes=(-1, 1, 2)),
               dict(T=0), dict(T_out=0), dict(J=0), dict(B=-1), dict(T_out=5), dict(num=3, den=2, T_out=6),
               dict(parent=(-1,) + tuple(range(64)), carried=(0,) * 65)):
        assert call(**kw) == 1, kw
    assert call(num=3, den=2, T_out=5) == 0            # (4 - 1) 3 // 2 + 1 frames
    assert call(parent=(-1,) + tuple(range(63)), carried=(0,) * 64) == 0

"""CPU: the rig retargeting's host side and its restatement, on tests/golden/motion_fk.npz.

* ``target_rig`` on the synthetic targets of tests/retarget_ref.py: the verbatim tables, which node follows which rule, the rule
  for opposite rest directions, the legs; ``target_bvh_text`` gives the target's HIERARCHY back token for token;
* the restatement has the properties the feature is for, from the text-only reader alone: bone directions, the root, the same
  rest pose, the ankles under leg IK (and how many frames are out of the target's reach), the knee's side;
* each of seven mistakes lies >= 100 gates from the truth (GATE = 4 x the yardstick: how far the all-fp32 restatement's file
  reads back from the fp64 one's, joints and global matrices separately);
* ValueError of ``target_rig`` / ``check_retarget`` / ``to_bvh``, MDM_ERR_ARG of ``mdm_retarget_channels`` without a device.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, pkg

import retarget_ref as TR

GATE = 4.0
LENS = [24, 2, 1]
AT = np.cumsum([0] + LENS)


@functools.lru_cache(maxsize=None)
def case(name):
    """A golden case in fp64: (skeleton, raw rest axes, joints per sample, rotations per sample, offsets (3, J, 3)): the golden
    rotations and root path posed on the golden file's shared offsets with left and right evened (``TR.even_offsets``)."""
    z = np.load(os.path.join(GOLDEN, "motion_fk.npz"))
    skel = name.split("_")[0]
    sk = pkg("motion_features").get_skeleton(skel)
    j, R = z[f"{name}_joints64"], z[f"{name}_rotations64"]
    off = TR.even_offsets(skel, z[f"{skel}_offsets"])
    rots = [R[AT[b]:AT[b] + n] for b, n in enumerate(LENS)]
    joints = [TR.pose(sk.parents, j[AT[b]:AT[b] + n, 0], rots[b], off) for b, n in enumerate(LENS)]
    return skel, sk.raw_offsets, joints, rots, np.repeat(off[None], 3, 0)


@functools.lru_cache(maxsize=None)
def target(key, skel="t2m"):
    MRig = pkg("motion_rig")
    off = np.load(os.path.join(GOLDEN, "motion_fk.npz"))[f"{skel}_offsets"]
    text, jmap, up = {"a": lambda: (TR.own_rig_text(MRig, skel, off), "smpl" if skel == "t2m" else "kit", "Y"),
                      "a2": lambda: (TR.own_rig_text(MRig, skel, off, True), "smpl" if skel == "t2m" else "kit", "Y"),
                      "b": lambda: (TR.mixamo_text(), "mixamo", "Y"), "c": lambda: (TR.mixamo_text("A"), "mixamo", "Y"),
                      "d": lambda: (TR.cmu_text(), TR.CMU_MAP, "Y"), "e": lambda: (TR.mixamo_text(up="Z"), "mixamo", "Z"),
                      "f": lambda: (TR.mixamo_text("up"), "mixamo", "Y")}[key]()
    return MRig.target_rig(text, jmap, up), text


def test_target_tables():
    MRig = pkg("motion_rig")
    tg, text = target("b")
    bvh = MRig.parse_bvh(text)
    assert tg.n_nodes == 65 and tg.joints == 22 and tg.names == bvh.names and tg.parent == list(bvh.parent)
    assert np.array_equal(tg.offsets, bvh.offsets) and set(tg.end_sites) == set(bvh.end_sites)
    assert tg.pick == MRig.resolve_joint_map(bvh, "mixamo") and tg.leg_ok
    at = {n.split(":")[1]: i for i, n in enumerate(tg.names)}
    assert tg.kind[at["Hips"]] == MRig.RT_FIT and tg.kind[at["Spine2"]] == MRig.RT_FIT
    assert tg.kind[at["LeftHandIndex2"]] == MRig.RT_NONE and tg.kind[at["LeftHand"]] == MRig.RT_NONE
    assert tg.res[at["LeftHandIndex2"]] == at["LeftForeArm"]          # the wrist is a mapped leaf: the hand turns with the forearm
    assert tg.kind[at["Head"]] == MRig.RT_NONE and tg.res[at["HeadTop_End"]] == at["Neck"]
    assert tg.kind[at["LeftArm"]] == MRig.RT_COPY and tg.src[at["LeftArm"]] == 18
    # the T pose: the upper arm along +X onto the source's -Y
    A = tg.M[at["LeftArm"]]
    assert np.abs(A @ np.array([1.0, 0, 0]) - np.array([0, -1.0, 0])).max() < 1e-12 and abs(np.linalg.det(A) - 1) < 1e-12
    assert tg.table.dtype == np.int32 and tg.table.size == MRig.RT_WORDS and tg.table[0] == 65 and tg.table[1] == 22
    # (f): opposite directions turn half a turn about unit(u x e_m), m the axis of u's smallest component (X here)
    tf, _ = target("f")
    A = tf.M[at["LeftArm"]]
    assert np.abs(A - np.diag([-1.0, -1.0, 1.0])).max() < 1e-12     # u = +Y: across(u) = unit(Y x X) = -Z
    assert np.array_equal(MRig.across(np.array([0.0, 1.0, 0.0])), np.array([0.0, 0.0, -1.0]))
    # (d): zero-offset nodes; Hips fitted from its two legs, Spine1 follows the neck, the collars sit at no distance
    td, _ = target("d")
    at = {n: i for i, n in enumerate(td.names)}
    assert td.fit[at["Hips"]] == (1, 2, [1, 2]) and td.kind[at["LHipJoint"]] == MRig.RT_NONE
    assert td.kind[at["Spine1"]] == MRig.RT_COPY and td.src[at["Spine1"]] == 12 and td.pick[15] == td.n_nodes + at["Head"]
    assert td.kind[at["LowerBack"]] == MRig.RT_COPY and td.src[at["LowerBack"]] == 6
    # (e): the same character written Z-up has the same rules, and its rest positions are the Y-up ones turned
    te, _ = target("e")
    assert te.kind == tg.kind and te.src == tg.src and te.fit == tg.fit
    assert np.abs(te.rest @ TR.Z_UP.T - tg.rest).max() < 1e-6


@pytest.mark.parametrize("key", ["a", "b", "d", "e"])
def test_text_gives_the_hierarchy_back(key):
    MRig = pkg("motion_rig")
    tg, text = target(key)
    chan = np.zeros((2, 3 + 3 * tg.n_nodes), np.float32)
    out = MRig.target_bvh_text(tg, chan, 2, 0.05)
    head = lambda s: s[:s.index("MOTION")].split()
    assert head(out) == head(text)
    assert out[out.index("MOTION"):].split()[:6] == ["MOTION", "Frames:", "2", "Frame", "Time:", "0.05"]
    xyz = MRig.target_bvh_text(tg, chan, 1, 0.05, euler="XYZ")
    assert "CHANNELS 3 Xrotation Yrotation Zrotation" in xyz and MRig.parse_bvh(xyz).frames == 1
    with pytest.raises(ValueError):
        MRig.target_bvh_text(tg, chan[:, :-1], 2, 0.05)
    with pytest.raises(ValueError):
        MRig.target_bvh_text(tg, chan, 3, 0.05)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def properties(tg, skel, joints, offs, truth, gate_j, leg_ik, frames=None):
    """The direction, root and ankle properties of a read-back ``truth`` (per sample (joints, positions, globals)) against the
    source joints; ``frames``: per sample the source frame of each read-back frame.  -> (worst direction error, worst root
    error, worst ankle error on reachable frames, unreachable frames, frames, the smallest knee-side dot product)."""
    parents = pkg("motion_features").get_skeleton(skel).parents
    Bt = tg.basis.T
    e_dir = e_root = e_ank = 0.0
    out, total, side = 0, 0, np.inf
    for b, (jo, _, _) in enumerate(truth):
        x = joints[b][:len(jo)] if frames is None else joints[b][frames[b]]
        s = TR.scale_of(tg, offs[b])
        e_root = max(e_root, float(np.abs(jo[:, 0] - s * x[:, 0] @ Bt.T).max()))
        for jc in range(1, tg.joints):
            j = parents[jc]
            n = tg.pick[j]
            if n >= tg.n_nodes or tg.kind[n] != 1 or tg.src[n] != jc or (leg_ik and any(jc in leg[1:] for leg in tg.legs)):
                continue  # a fitted node, a bone without length in the target, or a bone the leg IK turns
            e_dir = max(e_dir, float(np.abs(_unit(jo[:, jc] - jo[:, j]) - _unit((x[:, jc] - x[:, j]) @ Bt.T)).max()))
        for (h, k, a), (l1, l2, _, _) in zip(tg.legs, tg.leg_rest):
            want = s * x[:, a] @ Bt.T
            dist = np.linalg.norm(want - jo[:, h], axis=-1)
            ok = (dist < l1 + l2 - 1e-4 * (l1 + l2)) & (dist > abs(l1 - l2) + 1e-4 * (l1 + l2))
            out, total = out + int((~ok).sum()), total + len(ok)
            if ok.any():
                e_ank = max(e_ank, float(np.abs(jo[ok, a] - want[ok]).max()))
            line = _unit(jo[:, a] - jo[:, h])
            pole = lambda hip, knee: (knee - hip) - ((knee - hip) * line).sum(-1, keepdims=True) * line
            ours, theirs = pole(jo[:, h], jo[:, k]), pole(x[:, h] @ Bt.T, x[:, k] @ Bt.T)
            bent = np.linalg.norm(theirs, axis=-1) > 1e-3 * np.linalg.norm(x[:, k] - x[:, h], axis=-1)
            if leg_ik and bent.any():
                side = min(side, float((_unit(ours[bent]) * _unit(theirs[bent])).sum(-1).min()))
    return e_dir, e_root, e_ank, out, total, side


@pytest.mark.parametrize("key,name", [("a", "t2m_noisy"), ("b", "t2m_noisy"), ("c", "t2m_clean"), ("d", "t2m_noisy"),
                                      ("e", "t2m_noisy"), ("f", "t2m_clean"), ("a", "kit_noisy"), ("a", "kit_clean")])
def test_the_restatement_has_the_properties(key, name):
    MRig = pkg("motion_rig")
    skel, raw, joints, rots, offs = case(name)
    tg, _ = target(key, skel)
    for leg_ik in (False, True):
        truth, yj, yg = TR.yardstick(MRig, tg, raw, joints, rots, offs, LENS, leg_ik=leg_ik)
        size = float(np.abs(truth[0][0]).max())
        e_dir, e_root, e_ank, out, total, side = properties(tg, skel, joints, offs, truth, GATE * yj, leg_ik)
        print(key, name, "leg_ik", leg_ik, f"yardstick joints {yj:.3g} globals {yg:.3g}; direction {e_dir:.3g} root {e_root:.3g} "
              f"ankle {e_ank:.3g} unreachable {out}/{total} knee side {side:.3g}")
        # a direction is a difference of two positions over a bone's length: the gate of positions over the shortest bone
        shortest = min(float(np.linalg.norm(tg.joint_rest[jc] - tg.rest[n])) for n, jc in
                       ((n, tg.src[n]) for n in range(tg.n_nodes) if tg.kind[n] == 1))
        assert e_dir <= 2 * GATE * yj / shortest and e_root <= GATE * yj, (e_dir, e_root, yj, size)
        if key in "bcef" and name == "t2m_noisy":                      # the clip chosen for it; the others are recorded
            assert out <= 0.1 * total                                   # at most 10 % of the frames are out of the legs' reach
        if leg_ik:
            assert e_ank <= GATE * yj and side > 0, (e_ank, yj, side)
        elif key != "a":
            assert e_ank > 100 * GATE * yj, (e_ank, yj)                # without the IK the ankles are somewhere else


def test_the_same_rest_pose_copies_the_rotations():
    """On the project's own tree, every bone subdivided by an unmapped node: A = I, and a node with one bone has the global
    rotation R[jc]; the nodes in between turn with it."""
    MRig = pkg("motion_rig")
    skel, raw, joints, rots, offs = case("t2m_noisy")
    tg, _ = target("a2")
    assert tg.n_nodes > 28 and max(float(np.abs(tg.M[n] - np.eye(3)).max()) for n in range(tg.n_nodes) if tg.kind[n] == 1) < 1e-12
    truth, yj, yg = TR.yardstick(MRig, tg, raw, joints, rots, offs, LENS)
    worst = 0.0
    for b in range(3):
        for n in range(tg.n_nodes):
            r = tg.res[n]
            if r >= 0 and tg.kind[r] == 1:
                worst = max(worst, float(np.abs(truth[b][2][:, n] - rots[b][:, tg.src[r]]).max()))
    print(f"globals against R[jc] {worst:.3g} (yardstick {yg:.3g})")
    assert worst <= GATE * yg


@pytest.mark.parametrize("variant", TR.VARIANTS)
def test_each_mistake_lies_far_from_the_truth(variant):
    MRig = pkg("motion_rig")
    skel, raw, joints, rots, offs = case("t2m_noisy")
    key = "e" if variant == "basis" else "c"  # basis and its transpose differ only where the file is not Y-up
    leg_ik = variant == "knee_mirrored"
    tg, _ = target(key)
    truth, yj, yg = TR.yardstick(MRig, tg, raw, joints, rots, offs, LENS, leg_ik=leg_ik)
    gates = 0.0
    for b, n in enumerate(LENS):
        chan = TR.channels_of(tg, raw, joints[b], rots[b], offs[b], leg_ik=leg_ik, variant=variant)[0]
        jo, _, G = TR.read_back(MRig.target_bvh_text(tg, chan, n, 0.05), tg)
        gates = max(gates, float(np.abs(jo - truth[b][0]).max()) / (GATE * yj), float(np.abs(G - truth[b][2]).max()) / (GATE * yg))
    print(variant, f"{gates:.3g} gates (yardstick joints {yj:.3g}, globals {yg:.3g})")
    assert gates >= 100, (variant, gates)


def _mixamo_names():
    return list(pkg("motion_rig").JOINT_MAPS["mixamo"])


def test_value_errors():
    MRig, MO = pkg("motion_rig"), pkg("motion_outputs")
    text = TR.mixamo_text()
    names = _mixamo_names()
    twice = list(names)
    twice[20] = twice[18]                                              # the wrist on the elbow's node
    with pytest.raises(ValueError, match="two joints on one node"):
        MRig.target_rig(text, twice)
    swapped = list(names)
    swapped[1], swapped[4] = swapped[4], swapped[1]                    # hip and knee exchanged: the knee's node is above the hip's
    with pytest.raises(ValueError, match="not below"):
        MRig.target_rig(text, swapped)
    with pytest.raises(ValueError, match="not below"):
        MRig.target_rig(TR.cmu_text(), "cmu")                          # spine3 on Neck1, the shoulders hang off Spine1
    moved = list(names)
    moved[0] = "Spine"
    with pytest.raises(ValueError):
        MRig.target_rig(text, moved)
    with pytest.raises(ValueError, match="rotation"):
        MRig.target_rig(text, "mixamo", basis=np.diag([1.0, 1.0, -1.0]))
    with pytest.raises(ValueError, match="up must be"):
        MRig.target_rig(text, "mixamo", up="X")
    with pytest.raises(ValueError):
        MRig.target_rig(text, "smpl")
    with pytest.raises(ValueError):
        MRig.target_rig(text, "mixamo", skeleton="kit")
    tg = MRig.target_rig(text, "mixamo")
    j, r, off = torch.zeros(2, 8, 22, 3), torch.zeros(2, 8, 22, 3, 3), torch.ones(22, 3)
    out = MRig.check_retarget(j, r, [8, 3], tg, off, fps_out=30)
    assert out[6:8] == (3, 2) and out[8].tolist() == [11, 4] and out[9] is True and out[3].shape == (2, 22, 3)
    for bad in (dict(joints=j[:, :, :21]), dict(rotations=r[:1]), dict(lengths=[8, 9]), dict(offsets=None),
                dict(offsets=torch.ones(3, 22, 3)), dict(euler="XYX"), dict(skeleton="kit"), dict(fps_out=0)):
        kw = dict(joints=j, rotations=r, lengths=[8, 3], target=tg, offsets=off)
        kw.update(bad)
        with pytest.raises(ValueError):
            MRig.check_retarget(**kw)
    # a target whose legs cannot take IK: off by default, refused where asked for
    from types import SimpleNamespace
    stiff = SimpleNamespace(**{**vars(tg), "leg_ok": False})
    assert MRig.check_retarget(j, r, [8, 3], stiff, off)[9] is False
    with pytest.raises(ValueError, match="leg_ik"):
        MRig.check_retarget(j, r, [8, 3], stiff, off, leg_ik=True)
    # the trainer's output stage refuses a scale with a target, before anything runs
    with pytest.raises(ValueError, match="scale"):
        MO.to_bvh([torch.zeros(6, 263)], [6], 263, None, None, None, False, 5, None, None, None, "ZXY", 100.0, text)


def test_the_entry_refuses_bad_arguments_without_a_device():
    """mdm_retarget_channels returns MDM_ERR_ARG for null pointers, malformed tables, bad axes and ratios before any launch."""
    MRig, L = pkg("motion_rig"), pkg("_lib")
    lib = L.lib()
    tg, _ = target("b")
    assert lib.mdm_retarget_table_words() == MRig.RT_WORDS
    B, T, J = 2, 4, 22
    bufs = [np.zeros(n, np.float32) for n in (B * T * J * 3, B * T * J * 9, B * J * 3, B * T * 65 * 9, B * T * (3 + 3 * 65))]
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(table=None, **kw):
        t = np.ascontiguousarray(tg.table if table is None else table, np.int32)
        a = dict(joints=ptr(bufs[0]), rot=ptr(bufs[1]), off=ptr(bufs[2]), length=None, B=B, T=T, J=J, host=ptr(t), dev=ptr(t),
                 leg_ik=1, a0=2, a1=0, a2=1, num=1, den=1, T_out=T, length_out=None, glob=ptr(bufs[3]), chan=ptr(bufs[4]))
        a.update(kw)
        return lib.mdm_retarget_channels(*a.values(), None)

    assert call(B=0) == 0                                              # the good arguments pass the checks (no sample: no launch)
    for k in ("joints", "rot", "off", "host", "dev", "glob", "chan"):
        assert call(B=0, **{k: None}) == 1, k
    for kw in (dict(T=0), dict(T_out=0), dict(num=0), dict(den=0), dict(a0=0), dict(a1=3), dict(a2=-1), dict(leg_ik=2),
               dict(T_out=T + 1), dict(num=3, den=2, T_out=6), dict(J=21), dict(B=-1)):
        assert call(B=kw.pop("B", 0), **kw) == 1, kw
    assert call(B=0, num=3, den=2, T_out=5) == 0
    base, node = 16, 16

    def broken(at, value, as_float=False):
        t = tg.table.copy()
        if as_float:
            t.view(np.float32)[at] = value
        else:
            t[at] = value
        return t

    fbase = 16 + 16 * 128
    cases = {"129 nodes": broken(0, 129), "no node": broken(0, 0), "33 joints": broken(1, 33),
             "a parent after its node": broken(base + node * 3, 5), "a root with a parent": broken(base, 0),
             "a kind": broken(base + 2, 3), "a copied joint": broken(base + node * 1 + 3, 22),
             "a fit joint": broken(base + 4, -1), "nb": broken(base + 6, 9), "a b joint": broken(base + 7, 40),
             "res": broken(base + node * 2 + 1, 1), "an inherited res": broken(base + node * 6 + 1, 6),
             "a leg joint": broken(4, 22), "a shin node": broken(4 + 4, 65), "a thigh that copies nothing": broken(4 + 3, 6),
             "nan in the basis": broken(fbase, np.nan, True), "no leg length": broken(fbase + 9, 0.0, True),
             "l1": broken(fbase + 10, -1.0, True), "an offset": broken(fbase + 32 + 12 * 3, np.inf, True)}
    for what, t in cases.items():
        assert call(B=0, table=t) == 1, what
    no_legs = broken(2, 0)
    assert call(B=0, table=no_legs, leg_ik=0) == 0 and call(B=0, table=no_legs, leg_ik=1) == 1
    more = TR.hierarchy_text(("r", (0, 0, 0), [(f"n{i}", (0, 1, 0), [], None) for i in range(128)], None))
    with pytest.raises(ValueError, match="128"):
        MRig.target_rig(more, ["r"] * 22)

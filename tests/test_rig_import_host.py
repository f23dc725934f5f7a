"""CPU: the rig import's host side and its restatement, on files written by tests/rig_import_ref.py from
tests/golden/motion_fk.npz.

* parse_bvh gives the tables and values of the independent reader rig_ref.parse_bvh on our own export and on the CMU-like file,
  also with CRLF line ends, tabs and keywords in another letter case; every malformed file raises with its line number;
* every preset of JOINT_MAPS resolves on its own naming, detection picks the right one, a missing name is reported; on the
  CMU files' own hierarchy (zero offsets at Neck and the Shoulder nodes) the preset leaves every bone its length and a joint
  map that does not is refused;
* the restatement gives the clip's joints back in fp64, and each of eight wrong variants lies >= 100 gates from the truth,
  from the restatement alone;
* mdm_rig_joints refuses every malformed table with MDM_ERR_ARG, without a device.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, pkg

import rig_import_ref as IR
import rig_ref as RR

LENS = [24, 2, 1]
AT = np.cumsum([0] + LENS)
GATE = 4.0


def golden(name="t2m_noisy"):
    z = np.load(os.path.join(GOLDEN, "motion_fk.npz"))
    j, R = z[f"{name}_joints64"], z[f"{name}_rotations64"]
    return z["t2m_offsets"], [j[AT[b]:AT[b] + n] for b, n in enumerate(LENS)], [R[AT[b]:AT[b] + n] for b, n in enumerate(LENS)]


def files():
    """(a) our own export and (b) the CMU-like file of the golden's first sample."""
    MRig = pkg("motion_rig")
    off, joints, rots = golden()
    rig = MRig.rig_of("t2m")
    return (IR.own_export(MRig.bvh_text, rig, off, joints[0], rots[0]), IR.cmu_like(rig, off, joints[0], rots[0])), joints[0]


def same_tables(got, want):
    assert got.names == want.names and list(got.parent) == list(want.parent) and got.channels == want.channels
    assert np.array_equal(got.offsets, want.offsets) and got.offsets.shape == (len(want.names), 3)
    assert sorted(got.end_sites) == sorted(want.end_sites) and all(np.array_equal(got.end_sites[k], v) for k, v in want.end_sites.items())
    assert got.frames == want.frames and got.frame_time == want.frame_time
    assert got.values.dtype == np.float32 and np.array_equal(got.values, want.values.astype(np.float32))
    rot, pos = IR.node_channels(want)  # the columns, counted by the restatement
    for n, r in enumerate(rot):
        k = len(r)
        assert got.rot_col[n, :k].tolist() == [c for c, _ in r] and got.rot_axis[n, :k].tolist() == [a for _, a in r]
        assert (got.rot_col[n, k:] == -1).all()
    assert got.pos_col.tolist() == pos and got.rot_col.shape == got.rot_axis.shape == (len(want.names), 3)


def test_parser_against_the_independent_reader(tmp_path):
    MRig = pkg("motion_rig")
    (own, cmu), _ = files()
    for text in (own, cmu):
        want = RR.parse_bvh(text)
        same_tables(MRig.parse_bvh(text), want)
        same_tables(MRig.parse_bvh(text.replace("\n", "\r\n")), want)
        same_tables(MRig.parse_bvh(text.rstrip("\n")), want)                       # no final newline
        same_tables(MRig.parse_bvh(text.replace("rotation ", "rotation\n")), want)  # a CHANNELS list that wraps
        same_tables(MRig.parse_bvh(re.sub(r"^ +", lambda m: "\t" * len(m.group()), text, flags=re.M).replace(" ", " \t ")), want)
        mixed = text
        for a, b in (("HIERARCHY", "Hierarchy"), ("ROOT", "root"), ("JOINT", "Joint"), ("OFFSET", "offset"), ("CHANNELS", "Channels"),
                     ("End Site", "END SITE"), ("MOTION", "motion"), ("Frames:", "FRAMES:"), ("Frame Time:", "frame time:"),
                     ("rotation", "ROTATION"), ("Xposition", "xPosition")):
            mixed = mixed.replace(a, b)
        assert mixed != text
        same_tables(MRig.parse_bvh(mixed), want)
    cm = RR.parse_bvh(cmu)
    assert len(cm.names) == 33 and cm.channels[cm.names.index(IR.CMU_SIX)][:3] == ["Xposition", "Yposition", "Zposition"]
    assert [len(c) for c in cm.channels].count(0) == 2 and [len(c) for c in cm.channels].count(2) == 1
    got = MRig.parse_bvh(cmu)
    six = got.names.index(IR.CMU_SIX)
    assert got.rot_col[six].tolist() == [got.rot_col[six - 1, 2] + 4 + k for k in range(3)]     # its positions count as columns
    pre = IR.cmu_like(pkg("motion_rig").rig_of("t2m"), *[v[0] if isinstance(v, list) else v for v in golden()], prefix="mixamorig:")
    assert MRig.parse_bvh(pre).names == ["mixamorig:" + n for n in got.names]                      # names with ':'
    path = tmp_path / "a.bvh"
    path.write_bytes(cmu.replace("\n", "\r\n").encode())
    same_tables(MRig.read_bvh(str(path)), cm)


def line_of(text, needle, nth=0):
    return [i + 1 for i, ln in enumerate(text.splitlines()) if needle in ln][nth]


def test_parser_errors_carry_the_line_number():
    MRig = pkg("motion_rig")
    (own, _), _ = files()
    first_row = line_of(own, "Frame Time:") + 1
    rows = own.splitlines()
    cases = [
        ("a second ROOT", own.replace("JOINT left_hip", "ROOT left_hip"), line_of(own, "JOINT left_hip")),
        ("a second ROOT after the first", own.replace("MOTION", "ROOT again\n{\nOFFSET 0 0 0\n}\nMOTION"), line_of(own, "MOTION")),
        ("count and list", own.replace("CHANNELS 3", "CHANNELS 4", 1), line_of(own, "CHANNELS 3")),
        ("count and list", own.replace("CHANNELS 6 Xposition", "CHANNELS 6", 1), line_of(own, "CHANNELS 6")),
        ("unknown channel", own.replace("Zrotation", "Wrotation", 1), line_of(own, "Zrotation")),
        ("four rotations", own.replace("CHANNELS 3 Zrotation", "CHANNELS 4 Yrotation Zrotation", 1), line_of(own, "CHANNELS 3")),
        ("row width", "\n".join(rows[:first_row] + [rows[first_row] + " 1.0"] + rows[first_row + 1:]) + "\n", first_row + 1),
        ("fewer rows", "\n".join(rows[:-1]) + "\n", len(rows) - 1),
        ("nan", own.replace(rows[first_row].split()[5], "nan", 1), line_of(own, rows[first_row].split()[5])),
        ("inf offset", own.replace("OFFSET 0 0 0", "OFFSET 0 inf 0", 1), line_of(own, "OFFSET 0 0 0")),
        ("not a number", own.replace(rows[first_row].split()[5], "abc", 1), line_of(own, rows[first_row].split()[5])),
        ("a bare CHANNELS", own.replace("CHANNELS 3 Zrotation Xrotation Yrotation", "CHANNELS", 1), line_of(own, "CHANNELS 3") + 1),
        ("CHANNELS twice", own.replace("CHANNELS 3 Zrotation Xrotation Yrotation\n", "CHANNELS 0\nCHANNELS 3 Zrotation Xrotation Yrotation\n", 1),
         line_of(own, "CHANNELS 3") + 1),
        ("frame time", own.replace("Frame Time: 0.05", "Frame Time: 0"), line_of(own, "Frame Time:")),
        ("frame time", own.replace("Frame Time: 0.05", "Frame Time: -0.05"), line_of(own, "Frame Time:")),
    ]
    for what, text, line in cases:
        assert text != own, what
        with pytest.raises(ValueError, match=rf"line {line}:") as e:
            MRig.parse_bvh(text)
        print(what, "->", e.value)
    many = IR.chain(MRig.MAX_IMPORT_NODES + 1)
    with pytest.raises(ValueError, match=rf"line {line_of(many, 'JOINT', MRig.MAX_IMPORT_NODES - 1)}: more than 128 nodes"):
        MRig.parse_bvh(many)
    assert len(MRig.parse_bvh(IR.chain(MRig.MAX_IMPORT_NODES)).names) == 128


def picked(bvh, pick):
    """The names of what the product's indices pick: N + n is the End Site of node n."""
    N = len(bvh.names)
    return [bvh.names[p] if p < N else bvh.names[p - N] + "/End" for p in pick]


def test_joint_maps():
    MRig = pkg("motion_rig")
    (own, cmu), _ = files()
    off, joints, rots = golden()
    a, b = MRig.parse_bvh(own), MRig.parse_bvh(cmu)
    rig = MRig.rig_of("t2m")
    assert all(len(MRig.JOINT_MAPS[k]) == 22 for k in ("smpl", "cmu", "mixamo")) and len(MRig.JOINT_MAPS["kit"]) == 21
    assert list(MRig.JOINT_MAPS["cmu"]) == list(IR.CMU_JOINTS)
    want = [rig.joint_of.index(j) for j in range(22)]
    assert MRig.resolve_joint_map(a) == want == MRig.resolve_joint_map(a, "smpl")
    pick = MRig.resolve_joint_map(b)
    assert picked(b, pick) == list(IR.CMU_JOINTS) and pick == MRig.resolve_joint_map(b, "cmu")
    assert pick[15] == len(b.names) + b.names.index("Head") and max(pick[:15] + pick[16:]) < len(b.names)   # the head: Head's End Site
    tables = MRig.import_tables(b, pick)                                                       # ... a node of its own for the kernel
    assert len(tables[0]) == 34 and tables[0][33] == b.names.index("Head") and tables[4][15] == 33
    assert np.array_equal(tables[1][33], b.end_sites[b.names.index("Head")]) and (tables[2][33] == -1).all()
    pre = MRig.parse_bvh(IR.cmu_like(rig, off, joints[0], rots[0], prefix="mixamorig:"))
    assert MRig.resolve_joint_map(pre) == pick and MRig.resolve_joint_map(pre, [n.upper() for n in IR.CMU_JOINTS]) == pick
    # the KIT export and a Mixamo hierarchy
    kit = MRig.rig_of("kit")
    k = SimpleNames(kit.names)
    assert MRig.resolve_joint_map(k) == [kit.joint_of.index(j) for j in range(21)]
    mix = SimpleNames(["mixamorig:" + n for n in ("Hips", "Spine", "Spine1", "Spine2", "Neck", "Head", "HeadTop_End")] +
                      ["mixamorig:" + s + n for s in ("Left", "Right") for n in ("Shoulder", "Arm", "ForeArm", "Hand", "HandIndex1",
                                                                                 "UpLeg", "Leg", "Foot", "ToeBase", "Toe_End")])
    got = MRig.resolve_joint_map(mix)
    assert [mix.names[n].split(":")[1] for n in got] == list(MRig.JOINT_MAPS["mixamo"]) == [mix.names[n].split(":")[1] for n in MRig.resolve_joint_map(mix, "mixamo")]
    assert [mix.names[n] for n in got[:4]] == ["mixamorig:Hips", "mixamorig:LeftUpLeg", "mixamorig:RightUpLeg", "mixamorig:Spine"]
    # a dict by joint name or index, and what is missing is named
    assert picked(b, MRig.resolve_joint_map(b, {"pelvis": "hips", 1: "LeftUpLeg", "right_hip": "RHipJoint", 3: "lthumb/end"})) == \
        ["Hips", "LeftUpLeg", "RHipJoint", "LThumb/End"]
    with pytest.raises(ValueError, match="Spine/End"):
        MRig.resolve_joint_map(b, ["Hips", "Spine/End"])                                       # Spine has no End Site
    with pytest.raises(ValueError, match="Spine2"):
        MRig.resolve_joint_map(b, "mixamo")
    with pytest.raises(ValueError, match="Tail.*Wing|Wing.*Tail"):
        MRig.resolve_joint_map(b, ["Hips", "Tail", "Wing"])
    with pytest.raises(ValueError, match="lacks"):
        MRig.resolve_joint_map(SimpleNames(["Hips", "Tail"]))
    for bad in ("vicon", {0: "Hips", 2: "Spine"}, {"tail": "Hips"}, []):
        with pytest.raises(ValueError):
            MRig.resolve_joint_map(b, bad)


class SimpleNames:
    def __init__(self, names):
        self.names = list(names)


def spin_file(fps=30.0):
    """The clip of the wrong-variant test as a CMU-like file: every node turns by 2 .. 12 degrees a frame from a phase of up
    to a radian, the right upper arm passes 180 degrees between source frames 4 and 5."""
    MRig = pkg("motion_rig")
    off = np.load(os.path.join(GOLDEN, "motion_fk.npz"))["t2m_offsets"]
    rig = MRig.rig_of("t2m")
    j, R, _ = RR.spin_clip(rig, off, 9, 3, turning=rig.names.index("right_shoulder"), span=(169.0, 189.0))
    return RR.parse_bvh(IR.cmu_like(rig, off, j, R, frame_time=1 / fps)), j


def test_restatement_gives_the_joints_back():
    (own, cmu), joints = files()
    for text in (own, cmu):
        bvh = RR.parse_bvh(text)
        names = IR.CMU_JOINTS if text is cmu else [pkg("motion_rig").rig_of("t2m").names[n] for n in
                                                    [pkg("motion_rig").rig_of("t2m").joint_of.index(j) for j in range(22)]]
        pick = IR.pick_of(bvh, names)
        direct, _ = IR.import_joints(bvh, pick)
        through_q, q = IR.import_joints(bvh, pick, force_quaternions=True)
        # the file holds fp32 channels: the joints come back to that rounding (angles of ~100 degrees to 4e-6 degrees)
        assert np.abs(direct - joints).max() <= 2e-6 and np.abs(through_q - direct).max() <= 1e-12
        assert np.abs(np.linalg.norm(q, axis=-1) - 1).max() <= 1e-15 and (q[..., 0] >= 0).all()
    bvh, j = spin_file()
    assert np.abs(IR.import_joints(bvh, IR.pick_of(bvh, IR.CMU_JOINTS))[0] - j).max() <= 2e-6
    w = RR.matrix_to_quaternion(IR.local_matrices(bvh, np.float64))[:, bvh.names.index("RightArm"), 0]
    assert w[4] > 0 and w[5] > 0 and np.rad2deg(2 * np.arccos(w[4])) > 178 and np.rad2deg(2 * np.arccos(w[5])) > 178


def test_the_cmu_files_own_hierarchy():
    """On the hierarchy of the CMU files, zero offsets included, the preset leaves no bone of the skeleton without length; a
    placement that does (spine3 at Neck, which sits on Spine1) is refused before anything runs, with the bones named."""
    MRig = pkg("motion_rig")
    text = IR.cmu_real()
    bvh = MRig.parse_bvh(text)
    assert len(bvh.names) == 31 and sorted(bvh.names[n] for n in range(31) if not bvh.offsets[n].any() and n) == \
        ["LHipJoint", "LeftShoulder", "LowerBack", "Neck", "RHipJoint", "RightShoulder"]
    pick = MRig.resolve_joint_map(bvh)
    assert picked(bvh, pick) == list(IR.CMU_JOINTS) and MRig.zero_length_bones(bvh, pick, "t2m") == []
    files, picks, ratios, lengths_out, _ = MRig.check_import([text])
    assert picks == [pick] and ratios == [(1, 6)] and lengths_out == [2]
    # every bone of the skeleton has length in the restated joints
    ref = RR.parse_bvh(text)
    j = IR.import_joints(ref, IR.pick_of(ref, IR.CMU_JOINTS))[0]
    par = pkg("motion_features").SKELETONS["t2m"].parents
    assert min(float(np.linalg.norm(j[:, c] - j[:, par[c]], axis=-1).min()) for c in range(1, 22)) > 0.05
    naive = MRig.resolve_joint_map(bvh, IR.CMU_NAIVE)
    assert MRig.zero_length_bones(bvh, naive, "t2m") == [(6, 9), (9, 13), (9, 14)]
    jn = IR.import_joints(ref, IR.pick_of(ref, IR.CMU_NAIVE))[0]
    assert all(np.array_equal(jn[:, a], jn[:, b]) for a, b in ((6, 9), (9, 13), (9, 14)))         # they do coincide
    with pytest.raises(ValueError, match=r"\(6, 9\), \(9, 13\), \(9, 14\).*no length.*Spine1.*Neck"):
        MRig.check_import([text], joint_map=IR.CMU_NAIVE)
    assert MRig.zero_length_bones(bvh, [pick[0]] * 22, "t2m") == [(par[c], c) for c in range(1, 22)]   # all at one node
    assert MRig.check_import([text], joint_map=["Hips", "Neck", "Spine1"])[1] == [[0, 14, 13]]        # no skeleton: nothing to refuse


def test_wrong_variants_lie_far_from_the_truth():
    """30 -> 20 fps (output frame k at source frame 1.5 k) of a Z-up file: each mistake's joints against the truth's, in gates
    of 4 x the fp32 restatement's distance from the fp64 one."""
    bvh, _ = spin_file()
    pick = IR.pick_of(bvh, IR.CMU_JOINTS)
    kw = dict(num=2, den=3, basis=IR.Z_UP)
    (truth,), y = IR.yardstick([bvh], [pick], **kw)
    assert truth.shape == (6, 22, 3) and 0 < y < 1e-5
    for variant in IR.VARIANTS:
        d = float(np.abs(IR.import_joints(bvh, pick, variant=variant, **kw)[0] - truth).max()) / (GATE * y)
        print(f"{variant}: {d:.3g} gates (yardstick {y:.3g})")
        assert d >= 100, (variant, d)


def test_argument_checks_at_the_c_entry():
    """Everything that could make the kernel read out of bounds is MDM_ERR_ARG before any launch: no device is touched (the
    data pointers are made-up addresses that are never dereferenced)."""
    L = pkg("_lib")
    lib = L.lib()
    N, width, T = 4, 15, 8
    good = dict(values=0x1000, length=None, B=1, T=T, C=width, n_nodes=N, parent=[-1, 0, 1, 1],
                offsets=[0.0] * (3 * N), rot_col=[3, 4, 5, 6, 7, 8, 9, 10, -1, -1, -1, -1], rot_axis=[2, 0, 1] * N,
                pos_col=[0, 1, 2], pick=[0, 3], n_pick=2, basis=[1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0], scale=1.0, num=1, den=1,
                T_out=T, length_out=None, joints_out=0x2000, quaternions_out=None, stream=None)

    def call(**change):
        a = dict(good, **change)
        for k in ("parent", "rot_col", "rot_axis", "pos_col", "pick"):
            if a[k] is not None:
                a[k] = (C.c_int32 * len(a[k]))(*a[k])
        for k in ("offsets", "basis"):
            if a[k] is not None:
                a[k] = (C.c_float * len(a[k]))(*a[k])
        return lib.mdm_rig_joints(*[a[k] for k in good])

    assert call(B=0) == 0                                                        # the tables pass, and nothing is launched
    bad = [dict(parent=[-1, 0, 2, 1]), dict(parent=[-1, 0, 3, 1]), dict(parent=[0, 0, 1, 1]), dict(parent=[-1, -1, 1, 1]),
           dict(rot_col=[3, 4, width] + good["rot_col"][3:]), dict(rot_col=[-2] + good["rot_col"][1:]),
           dict(rot_axis=[3] + good["rot_axis"][1:]), dict(rot_axis=good["rot_axis"][:-1] + [-1]),
           dict(pos_col=[0, 1, width]), dict(pos_col=[-2, 1, 2]), dict(pick=[0, N]), dict(pick=[-1, 0]),
           dict(n_nodes=0), dict(n_nodes=129), dict(n_pick=0), dict(n_pick=129), dict(num=0), dict(den=0), dict(num=-1),
           dict(T=0), dict(T_out=0), dict(C=0), dict(B=-1), dict(T_out=T + 1), dict(num=1, den=2, T_out=5), dict(num=3, den=2, T_out=12),
           dict(values=None), dict(parent=None), dict(offsets=None), dict(rot_col=None), dict(rot_axis=None), dict(pos_col=None),
           dict(pick=None), dict(basis=None), dict(joints_out=None)]
    for change in bad:
        assert call(**change) == 1, change                                      # MDM_ERR_ARG
        assert "B" in change or call(B=0, **change) == 1, change                 # ... whatever B is
    assert call(B=0, num=1, den=2, T_out=4) == 0 and call(B=0, num=3, den=2, T_out=11) == 0   # the longest that the source allows
    # 128 nodes in one chain: the deepest walk the limits allow
    deep = dict(n_nodes=128, parent=list(range(-1, 127)), offsets=[0.0] * 384, rot_col=[-1] * 384, rot_axis=[0] * 384, pick=[127, 0])
    assert call(B=0, **deep) == 0

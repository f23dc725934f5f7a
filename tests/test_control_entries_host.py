"""CPU: the argument handling of the sixteen joint-control entries on the loaded library.

mdm_{joint,canvas}_{joint|scene|tracks|terrain}_{loss_grad,guidance} (the two plain window entries are mdm_joint_loss_grad and
mdm_joint_guidance).  Fake non-null pointers stand in for device memory and B / M = 0, so an accepted call returns 0
(MDM_OK) before anything is launched and a refused one returns 1 (MDM_ERR_ARG).  For every entry: a valid call, then every
rule of its level broken one at a time; then the fall-throughs: an entry whose optional part is absent accepts exactly what
the entry below it accepts, and a null terrain leaves the other terrain arguments unexamined.
"""
import itertools
import math

import pytest

from conftest import pkg

P, OFF4, OFF2 = 0x1000, 0x1004, 0x1002  # 16-byte aligned, off by 4 bytes, off by 2
F, T = 263, 8
LEVELS = ("joint", "scene", "tracks", "terrain")
ENTRIES = list(itertools.product(("joint", "canvas"), LEVELS, ("loss_grad", "guidance")))

VALID = dict(x=P, x0=P, mask=P, length=P, offsets=P, rows=P, mean=P, std=P, targets=P, weights=P, scene=P, K=2, joint_params=P,
             tracks=P, Km=2, track_bounds=P, terrain=P, terrain_rec=P, Gx=4, Gz=4, stand=P, B=0, M=0, T=T, F=F, loss_out=P,
             grad_out=P, scale=0.1, iters=1, coef=P, steps=10, t_dev=P, t_imm=0, workspace=P, stream=0)
TERMS = (("scene", "K", "joint_params"), ("tracks", "Km", "track_bounds"), ("terrain", "terrain_rec", "Gx", "Gz", "stand"))
CLOCK = ("scale", "iters", "coef", "steps", "t_dev", "t_imm")


def name_of(family, level, kind):
    return f"mdm_joint_{kind}" if (family, level) == ("joint", "joint") else f"mdm_{family}_{level}_{kind}"


def order(family, level, kind):
    """The entry's arguments in the order of include/mdm_hip.h."""
    guide = kind == "guidance"
    args = ("x", "x0", "mask") if guide else ("x0",)
    args += ("length",) if family == "joint" else ("offsets", "rows")
    args += ("mean", "std", "targets", "weights")
    for terms in TERMS[:LEVELS.index(level)]:
        args += terms
    args += ("B", "T", "F") if family == "joint" else ("M", "F")
    args += CLOCK if guide else ("loss_out", "grad_out")
    return args + (("workspace",) if family == "canvas" else ()) + ("stream",)


def call(entry, **kw):
    v = dict(VALID, **kw)
    return getattr(pkg("_lib").lib(), name_of(*entry))(*(v[a] for a in order(*entry)))


def limit(entry, K):
    lib = pkg("_lib").lib()
    return lib.mdm_joint_control_max_frames(F) if entry[1] == "joint" else lib.mdm_joint_scene_max_frames(F, K)


def broken(entry, K=VALID["K"]):
    """Every rule of the entry's level, broken one at a time: a list of overrides of VALID (K: the entry's primitive count)."""
    family, level, kind = entry
    lv, guide = LEVELS.index(level), kind == "guidance"
    required = ["x0", "mean", "std"] + (["length"] if family == "joint" else ["offsets", "rows", "workspace"])
    required += ["x", "coef"] if guide else ["loss_out", "grad_out"]
    required += ["targets", "weights"] if lv == 0 else ["joint_params"]  # from the scene level on: both or neither
    out = [{a: 0} for a in required]
    out += [dict(F=262), dict(F=10), dict(B=-1) if family == "joint" else dict(M=-1)]
    if family == "joint":
        out += [dict(T=0), dict(T=limit(entry, K) + 1)]
    if lv >= 1:
        out += [dict(K=-1), dict(K=17), dict(scene=0)]
    if lv >= 2:
        out += [dict(Km=-1), dict(Km=25), dict(tracks=0), dict(tracks=OFF4), dict(track_bounds=OFF4),
                dict(Km=0, tracks=OFF4), dict(Km=0, track_bounds=OFF4), dict(Km=0, tracks=0, track_bounds=OFF4)]
    if lv >= 3:
        out += [dict(Gx=1), dict(Gz=1), dict(Gx=513), dict(Gz=513), dict(terrain_rec=0), dict(terrain_rec=OFF4),
                dict(terrain=OFF2), dict(stand=OFF2)]
    if guide:
        out += [dict(iters=0), dict(iters=33), dict(scale=math.nan), dict(scale=math.inf), dict(scale=-math.inf), dict(steps=0),
                dict(t_dev=0, t_imm=VALID["steps"]), dict(t_dev=0, t_imm=-1)]
    return out


def accepted(entry):
    """Variants of the valid call that stay valid at the entry's level."""
    family, level, kind = entry
    lv = LEVELS.index(level)
    out = [dict(), dict(mask=0)]
    if lv >= 1:
        out += [dict(targets=0, weights=0), dict(K=0, scene=0), dict(K=0, scene=0, targets=0, weights=0), dict(K=16)]
    if lv >= 2:
        out += [dict(Km=0, tracks=0, track_bounds=0), dict(track_bounds=0), dict(Km=24), dict(Km=0)]
    if lv >= 3:
        out += [dict(stand=0), dict(Gx=2, Gz=512, stand=OFF4), dict(Km=0, tracks=0, track_bounds=0, K=0, scene=0)]
    if kind == "guidance":
        out += [dict(iters=32), dict(t_dev=0, t_imm=VALID["steps"] - 1), dict(t_imm=VALID["steps"]), dict(scale=0.0)]
    if family == "joint":
        out += [dict(T=1), dict(T=limit(entry, VALID["K"]))]
    return out


def test_the_entries_are_the_sixteen():
    L = pkg("_lib")
    assert len(ENTRIES) == 16 and all(name_of(*e) in L.PROTOTYPES for e in ENTRIES)
    assert (L.SCENE_MAX_PRIMS, L.SCENE_MAX_TRACKS, L.TERRAIN_MAX_GRID, L.CONTROL_MAX_ITERS) == (16, 24, 512, 32)
    for e in ENTRIES:
        assert len(order(*e)) == len(L.PROTOTYPES[name_of(*e)][1]), e


@pytest.mark.parametrize("entry", ENTRIES, ids=lambda e: name_of(*e))
def test_valid_calls_and_every_broken_rule(entry):
    for kw in accepted(entry):
        assert call(entry, **kw) == 0, kw
    for kw in broken(entry):
        assert call(entry, **kw) == 1, kw
    if entry[1] != "joint":  # targets without weights and the reverse (the plain level: each is required, above)
        assert call(entry, targets=0) == 1 and call(entry, weights=0) == 1


# the optional part of a level, absent (the scene level: no primitives, with targets: the plain kernel's case)
ABSENT = {"scene": dict(K=0, scene=0), "tracks": dict(Km=0, tracks=0, track_bounds=0), "terrain": dict(terrain=0)}


@pytest.mark.parametrize("entry", [e for e in ENTRIES if e[1] != "joint"], ids=lambda e: name_of(*e))
def test_absent_part_falls_through_to_the_entry_below(entry):
    family, level, kind = entry
    below = (family, LEVELS[LEVELS.index(level) - 1], kind)
    absent = ABSENT[level]
    K = absent.get("K", VALID["K"])
    cases = accepted(below) + broken(below, K)
    if below[1] != "joint":
        cases += [dict(targets=0), dict(weights=0)]
    for kw in cases:
        if level == "scene" and "T" in kw:  # the frame limit is the level's own: the last test
            continue
        low, high = call(below, **kw), call(entry, **dict(absent, **kw))
        assert low == high and low in (0, 1), (kw, low, high)


@pytest.mark.parametrize("entry", [e for e in ENTRIES if e[1] == "terrain"], ids=lambda e: name_of(*e))
def test_null_terrain_leaves_its_arguments_unexamined(entry):
    assert call(entry, terrain=0, terrain_rec=0, Gx=0, Gz=0, stand=0) == 0
    assert call(entry, terrain=0, terrain_rec=OFF4, Gx=1, Gz=513, stand=OFF2) == 0
    assert call(entry, terrain=0, joint_params=0) == 1 and call(entry, terrain=0, tracks=OFF4) == 1  # the tracks level's rules stay


def test_window_frame_limit_is_the_level_s_also_on_the_plain_kernel():
    """A scene-level call without primitives runs the plain kernel, but is held to mdm_joint_scene_max_frames(F, 0)."""
    lib = pkg("_lib").lib()
    plain, scene = lib.mdm_joint_control_max_frames(F), lib.mdm_joint_scene_max_frames(F, 0)
    assert 0 < scene <= plain
    for kind in ("loss_grad", "guidance"):
        assert call(("joint", "scene", kind), K=0, scene=0, T=scene) == 0
        assert call(("joint", "scene", kind), K=0, scene=0, T=scene + 1) == 1
        assert call(("joint", "joint", kind), T=plain) == 0 and call(("joint", "joint", kind), T=plain + 1) == 1

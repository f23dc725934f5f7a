"""CPU: characters sampled together: the host tables of ``motion_scene.partner_tables``, every ValueError, the
self-checks of the fp64 restatement in tests/partners_ref.py, and the placement that tests/test_partners_gpu.py relies on,
asserted on the reference alone."""
import math

import numpy as np
import pytest
import torch

import partners_ref as PR
from conftest import pkg
from test_motion_control_host import ref_positions


def _ms():
    return pkg("motion_scene")


def _tables(**kw):
    MS = _ms()
    args = dict(scenes_rows=[[0, 1], [2, 3, 4]], placements=np.zeros((6, 3)), lengths=[10, 7, 10, 10, 4, 10],
                bones=[(0, 1), (1, 2), (2, 3)], T=10, J=22, static_tracks=2)
    args.update(kw)
    return MS.partner_tables(args.pop("scenes_rows"), args.pop("placements"), args.pop("lengths"), args.pop("bones"), **args)


# ---- contact -------------------------------------------------------------------------------------------------------------
def test_contact_fields_and_errors():
    MS = _ms()
    assert tuple(MS.contact(0, 21, 1, 20, range(60, 81))) == (0, 21, 1, 20, 60, 81, 1.0, 0.5)
    assert tuple(MS.contact(1, 2, 0, 3, [4, 5, 6], weight=2, meet=0))[4:] == (4, 7, 2.0, 0.0)
    assert tuple(MS.contact(1, 2, 0, 3, []))[4:6] == (0, 0)
    for bad in (dict(frames=range(5, 2)), dict(frames=[3, 5]), dict(frames=range(0, 8, 2)), dict(meet=-0.1), dict(meet=1.5),
                dict(meet=math.nan), dict(meet=math.inf), dict(weight=-1.0), dict(weight=math.nan), dict(b=0), dict(joint_a=-1)):
        kw = dict(a=0, joint_a=1, b=1, joint_b=2, frames=range(2, 5))
        kw.update(bad)
        with pytest.raises(ValueError):
            MS.contact(**kw)


# ---- partner_tables ------------------------------------------------------------------------------------------------------
def test_slots_padding_and_track_indices():
    t = _tables()
    assert (t.B, t.T, t.J, t.Pm, t.nb, t.Ks, t.Km) == (6, 10, 22, 2, 3, 2, 8)
    assert t.partner_rows.dtype == torch.int32 and t.partner_rows.tolist() == [[1, -1], [0, -1], [3, 4], [2, 4], [2, 3], [-1, -1]]
    assert t.bones.dtype == torch.int32 and t.bones.tolist() == [[0, 1], [1, 2], [2, 3]]
    assert t.contacts.shape == (0, 8) and not t.weights.any()
    # slot q's bone i is track Ks + q nb + i: the reference puts row 4's bone (1, 2) of row 2's slot 1 at index 2 + 3 + 1
    x0 = torch.randn(6, 10, 263, generator=torch.Generator().manual_seed(0)) * 0.5
    mean, std = PR._stats(263, 6, 1)
    W = PR.world_joints(x0, t.lengths, mean, std, t.pose)
    rec = PR.partner_records(W, t.lengths, t, torch.zeros(6, 10, 2, 12))
    assert torch.equal(rec[2, :4, 6, 4:7], W[4][:, 1]) and torch.equal(rec[2, :4, 6, 7:10], W[4][:, 2])  # pose 0: local == world
    assert not rec[2, 4:, 5:8].any() and not rec[5].any() and not rec[0, :, 5:].any() and not rec[:, :, :2].any()
    assert not rec[0, 7:, 2:5].any() and bool((rec[0, :7, 2:5, 0] == 2).all())


def test_a_scene_of_one_and_rows_in_no_scene_have_no_partners():
    t = _tables(scenes_rows=[[0], [3]], static_tracks=0)
    assert t.Pm == 0 and t.Km == 0 and t.partner_rows.shape == (6, 0)
    t = _tables(scenes_rows=[], static_tracks=5)
    assert t.Pm == 0 and t.Km == 5


def test_placements_are_cos_and_sin_in_fp64():
    yaw = np.array([0.0, 0.3, -2.0, 7.0, math.pi, 1e-4])
    pl = np.stack([np.arange(6.0), -np.arange(6.0), yaw], 1)
    t = _tables(placements=pl)
    want = np.stack([pl[:, 0], pl[:, 1], np.cos(yaw), np.sin(yaw)], 1).astype(np.float32)
    assert t.placements.dtype == torch.float32 and np.array_equal(t.placements.numpy(), want)
    assert t.placements[0].tolist() == [0.0, 0.0, 1.0, 0.0]
    assert np.array_equal(t.pose.numpy(), pl)


def test_contact_weights_are_constant_clipped_and_one_sided_at_the_ends_of_meet():
    MS = _ms()
    cs = [MS.contact(0, 20, 1, 21, range(2, 9), weight=3.0, meet=0.5),   # n_1 = 7 clips [2, 9) to [2, 7)
          MS.contact(2, 5, 4, 6, range(0, 10), weight=2.0, meet=0.0),     # n_4 = 4; a does none of the reaching
          MS.contact(3, 5, 2, 6, range(5, 6), weight=4.0, meet=1.0),      # b does none
          MS.contact(3, 7, 4, 7, range(6, 9))]                            # wholly past n_4: no weight at all
    t = _tables(contacts=cs)
    w = torch.zeros(6, 10, 22, 3)
    w[0, 2:7, 20] = 3.0
    w[1, 2:7, 21] = 3.0
    w[4, 0:4, 6] = 2.0
    w[3, 5, 5] = 4.0
    assert torch.equal(t.weights, w)
    words = t.contacts.numpy()
    assert words[:, :6].tolist() == [[0, 20, 1, 21, 2, 9], [2, 5, 4, 6, 0, 10], [3, 5, 2, 6, 5, 6], [3, 7, 4, 7, 6, 9]]
    assert words[:, 6].view(np.float32).tolist() == [0.5, 0.0, 1.0, 0.5] and not words[:, 7].any()
    # static control weights are kept and added to
    cw = torch.zeros(6, 10, 22, 3)
    cw[0, :, 0, 0] = 1.5
    t = _tables(contacts=cs[:1], control_weights=cw)
    assert torch.equal(t.weights[0, :, 0], cw[0, :, 0]) and float(t.weights[0, 3, 20, 1]) == 3.0


def test_partner_tables_errors():
    MS = _ms()
    c = MS.contact(0, 20, 1, 21, range(2, 5))
    cw = torch.zeros(6, 10, 22, 3)
    cw[1, 4, 21, 2] = 0.5
    bad = [dict(scenes_rows=[[0, 6]]), dict(scenes_rows=[[0, -1]]), dict(scenes_rows=[[0, 1], [1, 2]]), dict(scenes_rows=[[0, 0]]),
           dict(static_tracks=19),                                   # 19 + 2 x 3 = 25 tracks
           dict(static_tracks=-1), dict(static_tracks=25, scenes_rows=[]),
           dict(scenes_rows=[[0, 1]], bones=None, static_tracks=4),  # 4 + 21 = 25
           dict(bones=[(0, 22)]), dict(bones=[(-1, 2)]),
           dict(contacts=[MS.contact(0, 22, 1, 3, range(2))]), dict(contacts=[MS.contact(0, 2, 1, 22, range(2))]),
           dict(contacts=[MS.contact(0, 2, 2, 3, range(2))]),        # rows of two scenes
           dict(contacts=[MS.contact(0, 2, 5, 3, range(2))]),        # row 5 is in no scene
           dict(contacts=[MS.contact(0, 2, 6, 3, range(2))]),        # no such row
           dict(contacts=[c, MS.contact(1, 21, 0, 3, range(4, 6))]), # two contacts on (row 1, frame 4, joint 21)
           dict(contacts=[c], control_weights=cw),                   # a contact on a static control weight
           dict(contacts=[(0, 20, 1, 21, 2, 5, 1.0, 0.5)]),          # not made by contact()
           dict(control_weights=torch.zeros(6, 10, 21, 3)),
           dict(placements=np.zeros((6, 2))), dict(placements=np.full((6, 3), np.nan)), dict(lengths=[10] * 5),
           dict(lengths=[11] * 6), dict(radius=0.0), dict(radius=math.inf), dict(weight=-1.0), dict(margin=math.nan)]
    for kw in bad:
        with pytest.raises(ValueError):
            _tables(**kw)
    with pytest.raises(ValueError, match="bones="):
        _tables(static_tracks=19)
    # at the limit, and frames a contact shares with a static weight on another joint, are fine
    assert _tables(static_tracks=18).Km == 24
    cw = torch.zeros(6, 10, 22, 3)
    cw[1, 4, 20, 2] = 0.5
    _tables(contacts=[c], control_weights=cw)


# ---- the runner's kwargs -------------------------------------------------------------------------------------------------
def _runner_kw(B=3, T=10, F=263, **over):
    MS = _ms()
    mean, std = PR._stats(F, B, 3)
    kw = dict(length=torch.tensor([T] * B), control_mean=mean, control_std=std, control_partner_scenes=[[0, 1, 2]],
              control_partner_placements=torch.zeros(B, 3, dtype=torch.float64), control_partner_bones=[(0, 1), (1, 2)],
              control_contact_list=[MS.contact(0, 20, 2, 21, range(3, 6), weight=2.0)])
    kw.update(over)
    return kw


def test_check_control_kwargs_builds_the_tables():
    Cn = pkg("conditioning")
    out = Cn.check_control_kwargs(_runner_kw(), (3, 10, 263))
    t = out["partners"]
    assert (t.Pm, t.nb, t.Ks, t.Km) == (2, 2, 0, 4) and out["scene"].shape == (3, 0, 12)
    assert out["weights"] is t.weights and tuple(out["targets"].shape) == (3, 10, 22, 3) and not out["targets"].any()
    assert float(t.weights[0, 4, 20, 0]) == 2.0 and float(t.weights[2, 3, 21, 2]) == 2.0 and float(t.weights.sum()) == 36.0
    # behind static tracks; the radius, margin and weight are the call's
    trk = _ms().batch_tracks(PR.static_tracks(10), 3, 10)
    out = Cn.check_control_kwargs(_runner_kw(control_tracks=trk, control_partner_radius=0.2, control_partner_margin=0.01,
                                             control_partner_weight=3.0), (3, 10, 263))
    t = out["partners"]
    assert (t.Ks, t.Km, t.radius, t.margin, t.weight) == (3, 7, 0.2, 0.01, 3.0)
    # a weight of 0 leaves the slots out, the contacts stay; without contacts there are no targets
    t = Cn.check_control_kwargs(_runner_kw(control_partner_weight=0.0), (3, 10, 263))["partners"]
    assert (t.Pm, t.Km, len(t.contacts)) == (0, 0, 1)
    out = Cn.check_control_kwargs(_runner_kw(control_contact_list=None), (3, 10, 263))
    assert out["targets"] is None and out["weights"] is None and out["partners"].Km == 4
    # nothing of this without the keys
    plain = {k: v for k, v in _runner_kw().items() if not k.startswith(("control_partner_", "control_contact_"))}
    assert Cn.check_control_kwargs({"length": plain["length"]}, (3, 10, 263)) is None


def test_check_control_kwargs_refusals():
    Cn, D = pkg("conditioning"), pkg("dist")
    MS = _ms()
    for over in (dict(control_partner_scenes=None), dict(control_partner_placements=None), dict(length=None),
                 dict(control_partner_bones=None),                                    # 2 x 21 tracks
                 dict(control_tracks=torch.zeros(3, 10, 21, 12)),                     # 21 + 2 x 2
                 dict(control_mean=None),
                 dict(handshake_offsets=torch.tensor([0])), dict(canvas_control_offsets=torch.tensor([0, 10])),
                 dict(control_contact_list=[MS.contact(0, 20, 3, 21, range(3))]),
                 dict(control_joints=torch.zeros(3, 10, 22, 3), control_weights=torch.ones(3, 10, 22, 3))):  # a contact on a weight
        with pytest.raises(ValueError):
            Cn.check_control_kwargs(_runner_kw(**over), (3, 10, 263))
    with pytest.raises(ValueError):  # T over mdm_joint_scene_max_frames
        Cn.check_control_kwargs(_runner_kw(T=210, control_contact_list=None), (3, 210, 263))
    assert Cn.check_control_kwargs(_runner_kw(T=202, control_contact_list=None), (3, 202, 263))["partners"].T == 202
    with pytest.raises(ValueError, match="control_partner_scenes"):
        Cn.check_control_kwargs({"control_partner_radius": 0.3, "length": torch.tensor([10] * 3)}, (3, 10, 263))
    for k in ("control_partner_scenes", "control_partner_placements", "control_contact_list", "control_partner_weight"):
        with pytest.raises(ValueError, match="sharded"):
            D.shard_kwargs({"length": torch.tensor([10] * 3), k: _runner_kw()[k] if k in _runner_kw() else 1.0}, 0, 1)
    assert D.shard_kwargs({"length": torch.tensor([10] * 3), "control_partner_scenes": None}, 0, 2)["length"].tolist() == [10, 10]


# ---- the reference's self-checks -----------------------------------------------------------------------------------------
def test_swapping_the_characters_and_meet_gives_the_same_meeting_points():
    MS = _ms()
    c = PR.case(4, 40, 263, "pairs", 0)
    a = MS.contact(0, 20, 1, 5, range(3, 35), meet=0.3)
    b = MS.contact(1, 5, 0, 20, range(3, 35), meet=0.7)
    fa, ma = PR.meeting_points(c["W"], c["lens"], a)
    fb, mb = PR.meeting_points(c["W"], c["lens"], b)
    assert fa == fb == list(range(3, 28)) and float((ma - mb).abs().max()) <= 1e-14
    assert torch.equal(PR.meeting_points(c["W"], c["lens"], MS.contact(0, 20, 1, 5, range(3, 35), meet=0.0))[1], c["W"][0][3:28, 20])


@pytest.mark.parametrize("B,T,F,layout,Ks", [(4, 40, 263, "pairs", 3), (4, 40, 251, "trio", 0)])
def test_reference_records_are_character_tracks_of_the_partner_in_the_rows_frame(B, T, F, layout, Ks):
    MS = _ms()
    c = PR.case(B, T, F, layout, Ks)
    t = c["tables"]
    for b in range(B):
        for q in range(t.Pm):
            p = int(t.partner_rows[b, q])
            n = 0 if p < 0 else min(int(c["lens"][b]), int(c["lens"][p]))
            got = c["rec"][b, :, Ks + q * t.nb:Ks + (q + 1) * t.nb]
            assert not got[n:].any()
            if p < 0:
                continue
            P = ref_positions(c["x0"][p, :n], c["mean"][p], c["std"][p]).detach()
            loc = MS.to_local(MS.to_world(P, c["pose"][p, :2].tolist(), float(c["pose"][p, 2])), c["pose"][b, :2].tolist(),
                              float(c["pose"][b, 2]))
            want = torch.stack(MS.character_tracks(loc, PR.RADIUS, margin=PR.MARGIN, weight=PR.WEIGHT, bones=c["bones"]), 1)
            assert torch.equal(got[:n], want)
    if Ks:
        assert torch.equal(c["rec"][:, :, :Ks].float(), c["static"])


def test_targets_of_the_reference_land_where_the_weights_are():
    c = PR.case(4, 40, 263, "pairs", 0)
    w = c["tables"].weights
    assert bool(c["hit"].any()) and not bool(((w.abs().sum(-1) != 0) & ~c["hit"]).any())
    assert float(w[3, 3:17, 5].abs().max()) == 0.0 and bool(c["hit"][3, 3:17, 5].all())  # meet = 0: a's side carries weight 0
    assert bool((w[2, 3:17, 21] == 1.0).all()) and not bool(c["hit"][2, 17:].any())


# ---- the placement of the kernel tests, on the reference alone -----------------------------------------------------------
@pytest.mark.parametrize("B,T,F,layout,Ks", PR.CASES)
def test_placement_puts_every_row_next_to_a_partner(B, T, F, layout, Ks):
    """Every row with a partner has a partner capsule within margin + joint radius (0 here) of at least 5 % of its (t, j): if
    this fails the placement is wrong, not the kernel."""
    c = PR.case(B, T, F, layout, Ks)
    t = c["tables"]
    shares = []
    for b in range(B):
        if not bool((t.partner_rows[b] >= 0).any()):
            continue
        n = int(c["lens"][b])
        P = ref_positions(c["x0"][b, :n], c["mean"][b], c["std"][b]).detach()
        shares.append(PR.near_share(P, c["rec"][b, :, Ks:], n, PR.MARGIN))
    print(f"[partners placement B={B} T={T} F={F} {layout} Ks={Ks}] share of (t, j) near a partner capsule per row: "
          + ", ".join(f"{s:.3f}" for s in shares))
    assert shares and min(shares) >= 0.05, shares

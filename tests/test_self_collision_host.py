"""CPU: self-collision avoidance without a device: the identity between the target term on the produced targets
and L_self, the default mask, every host error, the runner's kwargs and the placement of the kernel cases of
tests/test_self_collision_gpu.py, asserted on the fp64 reference alone."""
import numpy as np
import pytest
import torch

import self_collision_ref as SR
from conftest import pkg
from test_motion_control_host import ref_positions


def _rest(skel):
    MS, MM = pkg("motion_scene"), pkg("motion_mesh")
    off = MS.default_offsets(skel)
    return off, MM.rest_pose(off, skel)


# ---- the identity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [263, 251])
def test_target_term_on_the_produced_targets_has_the_gradient_of_l_self(F):
    c = SR.case(3, 40, F)
    body, worst = c["body"], 0.0
    for b in range(3):
        n = int(c["lens"][b])
        grads = []
        for which in ("self", "targets"):
            x = c["x0"][b, :n].double().clone().requires_grad_(True)
            P = ref_positions(x, c["mean"][b], c["std"][b])
            if which == "self":
                loss = SR.l_self(P, body, SR.WEIGHT)
            else:
                push, depth = SR.push_depth(P.detach()[None], [n], body)
                tg, w = SR.merge(P.detach()[None], push, depth, [n], body, SR.WEIGHT)
                loss = (w[0] * (P - tg[0]) ** 2).sum()
            loss.backward()
            grads.append(x.grad.clone())
        assert float(grads[0].abs().max()) > 0
        worst = max(worst, float((grads[0] - grads[1]).abs().max()) / float(grads[0].abs().max()))
    print(f"[self identity F={F}] gradient of the target term against autograd of L_self: {worst:.2e}")
    assert worst <= 1e-12


def test_weight_and_joint_weights_scale_the_loss():
    c = SR.case(1, 2, 263)
    P = c["P"][0]
    MS = pkg("motion_scene")
    body2 = MS.self_body(MS.default_offsets("t2m"), "t2m", radius_scale=SR.RADIUS_SCALE[263], joint_weights=[2.0] * 22)
    a, b = float(SR.l_self(P, c["body"], 1.0)), float(SR.l_self(P, body2, 3.0))
    assert a > 0 and abs(b - 6 * a) <= 1e-12 * b


# ---- rest pose and mask ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skel", ["t2m", "kit"])
@pytest.mark.parametrize("scale", [1.0, 1.8])
def test_rest_pose_has_depth_zero_under_the_default_mask(skel, scale):
    MS = pkg("motion_scene")
    off, rest = _rest(skel)
    body = MS.self_body(off, skel, radius_scale=scale)
    P = torch.from_numpy(rest)[None, None]
    push, depth = SR.push_depth(P, [1], body)
    assert float(depth.abs().max()) == 0.0 and float(push.abs().max()) == 0.0
    d, s = MS.self_penetration(P, [1], body)
    assert float(s[0]) == 0.0
    assert int(body.allowed.sum()) > 100  # and the mask is not empty: wrists against the trunk and the legs are in
    again = MS.self_body(rest + 3.0, skel, radius_scale=scale, rest_joints=True)
    assert torch.equal(again.allowed, body.allowed) and torch.allclose(again.bone_radius, body.bone_radius)


@pytest.mark.parametrize("skel", ["t2m", "kit"])
@pytest.mark.parametrize("hops", [0, 1, 2, 3])
def test_default_mask_is_the_restated_rule(skel, hops):
    MS, MF, MM = pkg("motion_scene"), pkg("motion_features"), pkg("motion_mesh")
    off, rest = _rest(skel)
    parents = list(MF.get_skeleton(skel).parents)
    radii = np.asarray(MM.BODY_RADII[skel]) * (rest[:, 1].max() - rest[:, 1].min()) * 1.2
    body = MS.self_body(off, skel, radius_scale=1.2, margin=0.03, hops=hops)
    want = SR.ref_mask(parents, rest, radii, radii, 0.03, hops)
    assert np.array_equal(body.allowed.numpy(), want)
    assert torch.allclose(body.bone_radius.double(), torch.from_numpy(radii[1:]), rtol=1e-6)
    assert torch.allclose(body.joint_params[:, 0].double(), torch.from_numpy(radii), rtol=1e-6) and bool((body.joint_params[:, 1] == 1).all())
    assert body.bones.tolist() == [[parents[c], c] for c in range(1, len(parents))]
    for j in range(body.J):
        assert int(body.pair_mask[j]) == sum(1 << i for i in range(body.nb) if want[j, i])
    if hops:  # a joint never meets its own bone or its parent's
        for c in range(1, body.J):
            assert not want[c, c - 1] and not want[parents[c], c - 1]


def test_more_hops_allow_fewer_pairs_and_shoulders_do_not_meet_the_neck():
    MS = pkg("motion_scene")
    from_names = {n: i for i, n in enumerate(pkg("motion_edit").SMPL_JOINTS)}
    off, _ = _rest("t2m")
    counts = [int(MS.self_body(off, "t2m", hops=h).allowed.sum()) for h in (0, 1, 2, 3)]
    assert counts == sorted(counts, reverse=True) and counts[0] > counts[3]
    body = MS.self_body(off, "t2m", hops=0)  # the rest rule alone takes the neighbours out
    assert not bool(body.allowed[from_names["left_hip"], from_names["right_hip"] - 1])
    assert not bool(body.allowed[from_names["left_collar"], from_names["neck"] - 1])
    far = MS.self_body(off, "t2m")
    assert bool(far.allowed[from_names["left_wrist"], from_names["spine2"] - 1])
    assert bool(far.allowed[from_names["left_wrist"], from_names["right_elbow"] - 1])


def test_explicit_pairs_radii_and_joint_parameters():
    MS = pkg("motion_scene")
    off, _ = _rest("t2m")
    pairs = np.zeros((22, 21), dtype=bool)
    pairs[20, 2] = pairs[21, 5] = pairs[3, 20] = True
    body = MS.self_body(off, "t2m", radii=np.full(22, 0.05), radius_scale=2.0, joint_radius=np.full(22, 0.01),
                        joint_weights=np.arange(22) / 10, margin=0.0, pairs=pairs)
    assert np.array_equal(body.allowed.numpy(), pairs) and body.margin == 0.0
    assert int(body.pair_mask[20]) == 4 and int(body.pair_mask[21]) == 32 and int(body.pair_mask[3]) == 1 << 20
    assert int(body.pair_mask.sum()) == 4 + 32 + (1 << 20)
    assert torch.allclose(body.bone_radius, torch.full((21,), 0.1)) and torch.allclose(body.joint_params[:, 0], torch.full((22,), 0.01))
    assert torch.allclose(body.joint_params[:, 1], torch.arange(22) / 10)
    none = MS.self_body(off, "t2m", pairs=np.zeros((22, 21), dtype=bool))
    assert int(none.pair_mask.abs().sum()) == 0


def test_self_body_errors():
    MS = pkg("motion_scene")
    off, _ = _rest("t2m")
    bad = [dict(radii=np.zeros(22)), dict(radii=np.full(22, np.nan)), dict(radii=np.full(22, -1.0)), dict(radii=np.ones(21)),
           dict(radius_scale=0.0), dict(radius_scale=float("inf")), dict(margin=float("nan")), dict(hops=-1), dict(hops=1.5),
           dict(pairs=np.zeros((22, 22), dtype=bool)), dict(pairs=np.zeros((22, 21))), dict(joint_radius=np.ones(5)),
           dict(joint_weights=-np.ones(22))]
    for kw in bad:
        with pytest.raises(ValueError):
            MS.self_body(off, "t2m", **kw)
    with pytest.raises(ValueError):
        MS.self_body(off[:5], "t2m")
    with pytest.raises(ValueError):
        MS.self_body(np.full((22, 3), np.inf), "t2m")
    with pytest.raises(ValueError):
        MS.self_body(off, "smpl")
    sk = pkg("motion_features").get_skeleton("t2m")
    import types
    other = types.SimpleNamespace(**{**vars(sk), "chains": tuple(sk.chains)})  # a skeleton BODY_RADII does not list
    with pytest.raises(ValueError, match="radii are required"):
        MS.self_body(off, other)
    assert MS.self_body(off, other, radii=np.full(22, 0.05)).nb == 21
    big = types.SimpleNamespace(joints=33, parents=tuple([-1] + list(range(32))), chains=(tuple(range(33)),))
    with pytest.raises(ValueError, match="at most 32"):
        MS.self_body(np.zeros((33, 3)), big, radii=np.ones(33))
    for kw in (dict(skeleton="smpl"), dict(height=0.0), dict(height=float("nan"))):
        with pytest.raises(ValueError):
            MS.default_offsets(**kw)
    body = MS.self_body(off, "t2m")
    with pytest.raises(ValueError):
        MS.self_penetration(torch.zeros(1, 2, 21, 3), [2], body)
    with pytest.raises(ValueError):
        MS.self_penetration(torch.zeros(1, 2, 22, 3), [2, 2], body)


def test_self_penetration_is_the_reference_s():
    MS = pkg("motion_scene")
    c = SR.case(3, 40, 263)
    depth, share = MS.self_penetration(c["P"], c["lens"], c["body"])
    for b, (s, _, _) in enumerate(SR.stats(c["P"], c["lens"], c["body"])):
        n = int(c["lens"][b])
        raw = SR.pens(c["P"][b, :n], c["body"])[3]
        deep = float((raw - c["body"].margin)[c["body"].allowed[None].expand_as(raw)].clamp(min=0).max())
        assert abs(float(share[b]) - s) <= 1e-12 and abs(float(depth[b]) - deep) <= 1e-6 and deep > 0


# ---- the runner's kwargs ---------------------------------------------------------------------------------------------------
def _kw(B=2, T=8, F=263, **over):
    MS = pkg("motion_scene")
    body = MS.self_body(MS.default_offsets(SR.SKELETON[F]), SR.SKELETON[F])
    kw = {"control_mean": torch.zeros(B, F), "control_std": torch.ones(B, F), "control_self": {"body": body, "weight": 2.0},
          "length": torch.full((B,), T)}
    kw.update(over)
    return kw


def test_check_control_kwargs_takes_the_key_alone_and_with_the_others():
    Cn, MS = pkg("conditioning"), pkg("motion_scene")
    kw = _kw()
    out = Cn.check_control_kwargs(kw, (2, 8, 263))
    assert out["self"]["body"] is kw["control_self"]["body"] and out["self"]["weight"] == 2.0
    assert out["targets"] is None and out["weights"] is None and "scene" not in out
    tg, w = torch.zeros(2, 8, 22, 3), torch.ones(2, 8)
    out = Cn.check_control_kwargs(dict(kw, control_joints=tg, control_weights=w, control_scene=MS.batch_scene([MS.floor()], 2),
                                       control_tracks=torch.zeros(2, 8, 1, 12)), (2, 8, 263))
    assert "self" in out and tuple(out["weights"].shape) == (2, 8, 22, 3) and "scene" in out and "tracks" in out
    # what changes nothing is the call without the key
    zero = dict(kw, control_self={"body": kw["control_self"]["body"], "weight": 0.0})
    assert Cn.check_control_kwargs(zero, (2, 8, 263)) is None
    off = MS.default_offsets("t2m")
    empty = MS.self_body(off, "t2m", pairs=np.zeros((22, 21), dtype=bool))
    assert Cn.check_control_kwargs(dict(kw, control_self={"body": empty, "weight": 2.0}), (2, 8, 263)) is None
    plain = Cn.check_control_kwargs(dict(zero, control_joints=tg, control_weights=w), (2, 8, 263))
    assert "self" not in plain and plain["targets"] is tg


def test_check_control_kwargs_errors():
    Cn, MS = pkg("conditioning"), pkg("motion_scene")
    kw = _kw()
    body = kw["control_self"]["body"]
    for bad in ((body, 2.0), {"body": body}, {"body": "t2m", "weight": 1.0}, {"body": body, "weight": -1.0},
                {"body": body, "weight": float("nan")}, {"body": body, "weight": 1.0, "margin": 0.1}):
        with pytest.raises(ValueError):
            Cn.check_control_kwargs(dict(kw, control_self=bad), (2, 8, 263))
    with pytest.raises(ValueError):  # a t2m body for KIT rows
        Cn.check_control_kwargs(dict(kw, control_mean=torch.zeros(2, 251), control_std=torch.ones(2, 251)), (2, 8, 251))
    with pytest.raises(ValueError, match="control_mean"):  # it needs mean and std, like every control
        Cn.check_control_kwargs({"control_self": kw["control_self"]}, (2, 8, 263))
    with pytest.raises(ValueError):  # T over the joint control's own limit, far under SELF_MAX_FRAMES
        Cn.check_control_kwargs(_kw(T=300), (2, 300, 263))
    assert MS.SELF_MAX_FRAMES == 3276
    with pytest.raises(ValueError, match="3276"):
        Cn._check_control_self(_kw(T=4000), (2, 4000, 263))
    partner = dict(control_partner_scenes=[[0, 1]], control_partner_placements=torch.zeros(2, 3))
    with pytest.raises(NotImplementedError, match="§33"):
        Cn.check_control_kwargs(dict(kw, **partner), (2, 8, 263))
    with pytest.raises(NotImplementedError, match="§33"):
        Cn.check_control_kwargs(dict(kw, control_contact_list=[MS.contact(0, 1, 1, 2, range(2))]), (2, 8, 263))
    with pytest.raises(NotImplementedError, match="§33"):
        Cn.check_control_kwargs(dict(kw, handshake_offsets=torch.tensor([0, 2], dtype=torch.int32)), (2, 8, 263))
    with pytest.raises(NotImplementedError, match="§33"):
        Cn.check_control_kwargs(dict(kw, canvas_control_offsets=torch.tensor([0, 8], dtype=torch.int32)), (2, 8, 263))


def test_shard_kwargs_passes_the_key_through():
    D = pkg("dist")
    kw = _kw(B=4)
    for lo, hi in ((0, 2), (2, 4), (1, 4)):
        part = D.shard_kwargs(kw, lo, hi)
        assert part["control_self"] is kw["control_self"]  # nothing in it leads with B or names rows
        assert tuple(part["control_mean"].shape) == (hi - lo, 263) and part["length"].numel() == hi - lo
        out = pkg("conditioning").check_control_kwargs(part, (hi - lo, 8, 263))
        assert out["self"]["body"] is kw["control_self"]["body"]


def test_conditioning_and_trainer_arguments():
    Cn, Tr, MS = pkg("conditioning"), pkg("trainer"), pkg("motion_scene")
    mean, std = np.zeros(263), np.ones(263)
    c = Cn.Conditioning(["a", "b", "c"], 263, mean=mean, std=std, self_collision=True)
    kw = c.kwargs(slice(1, 3), 8, "cpu")
    assert kw["control_self"]["weight"] == 5.0 and kw["control_self"]["body"].J == 22 and tuple(kw["control_mean"].shape) == (2, 263)
    assert "control_joints" not in kw and "control_scene" not in kw
    want = MS.self_body(MS.default_offsets("t2m"), "t2m")
    assert torch.equal(kw["control_self"]["body"].pair_mask, want.pair_mask) and kw["control_self"]["body"].margin == 0.02
    assert Cn.check_control_kwargs(dict(kw, length=torch.tensor([8, 8])), (2, 8, 263))["self"]["weight"] == 5.0
    opts = dict(weight=2.0, radius_scale=1.5, margin=0.0, hops=1, radii=np.full(22, 0.04), offsets=MS.default_offsets("t2m", 1.8))
    c = Cn.Conditioning(["a"], 263, mean=mean, std=std, self_collision=opts, control_scale=0.5)
    got = c.kwargs(slice(0, 1), 8, "cpu")["control_self"]
    assert got["weight"] == 2.0 and got["body"].margin == 0.0 and torch.allclose(got["body"].bone_radius, torch.full((21,), 0.06))
    assert Cn.Conditioning(["a"], 251, mean=np.zeros(251), std=np.ones(251),
                           self_collision=dict(height=1.6)).kwargs(slice(0, 1), 8, "cpu")["control_self"]["body"].J == 21
    # None, False and what changes nothing: the call without the argument (mean / std are not asked for)
    for off in (None, False, dict(weight=0.0), dict(pairs=np.zeros((22, 21), dtype=bool))):
        c = Cn.Conditioning(["a"], 263, self_collision=off)
        assert c.self_collision is None and c.kwargs(slice(0, 1), 8, "cpu") == {"text": ["a"]}
    for bad in (dict(weight=-1.0), dict(wieght=1.0), "yes", dict(radius_scale=0.0), dict(height=1.7, offsets=MS.default_offsets("t2m")),
                dict(radii=np.zeros(22))):
        with pytest.raises(ValueError):
            Cn.Conditioning(["a"], 263, mean=mean, std=std, self_collision=bad)
    with pytest.raises(ValueError):  # no skeleton at this width
        Cn.Conditioning(["a"], 131, mean=np.zeros(131), std=np.ones(131), self_collision=True)
    with pytest.raises(ValueError, match="mean and std"):
        Cn.Conditioning(["a"], 263, self_collision=True)
    import types
    tr = Tr.DDPMTrainer.__new__(Tr.DDPMTrainer)
    tr.encoder = types.SimpleNamespace(num_frames=60)  # the output stages plan the canvas before they generate
    with pytest.raises(NotImplementedError, match="§33"):
        tr.generate_long([[("walk", 40)]], 263, self_collision=True)
    with pytest.raises(NotImplementedError, match="§33"):
        tr.generate_long_joints([[("walk", 40)]], 263, mean, std, self_collision=True)
    with pytest.raises(NotImplementedError, match="§33"):
        tr.generate_together([[dict(caption="a", length=8), dict(caption="b", length=8)]], 263, mean, std, mutual=True,
                             self_collision=True)


# ---- placement of the kernel cases -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,F", SR.CASES)
def test_kernel_cases_penetrate_away_from_the_jumps(B, T, F):
    c = SR.case(B, T, F)
    for b, (share, axis, zero) in enumerate(SR.stats(c["P"], c["lens"], c["body"])):
        print(f"[self placement B={B} T={T} F={F}] sample {b}: share of (t, j) penetrating {share:.3f}, least distance of a "
              f"penetrating pair to its axis {axis:.2e} m, of an allowed pair to pen = 0 {zero:.2e} m")
        assert 0.10 <= share <= 0.60, (b, share)
        assert axis >= 1e-3 and zero >= 1e-3, (b, axis, zero)
    sg, sw = c["static"]
    for b in range(B):  # a static target sits on a penetrating joint, and wins there
        on = (sw[b] != 0).any(-1) & (c["depth"][b] > 0)
        assert bool(on[:, 1:].any())
        assert torch.equal(c["targets_static"][b][on], sg[b][on].double()) and torch.equal(c["weights_static"][b][on], sw[b][on].double())
    n = int(c["lens"][-1])
    assert float(c["push"][-1, n:].abs().max() if n < T else 0.0) == 0.0
    assert torch.equal(c["targets_static"][-1, n:], sg[-1, n:].double())

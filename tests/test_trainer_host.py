"""Host: the Python layer between the kernels' wrapper modules and ``DDPMTrainer``'s public methods; no device.

* the generate methods pass their conditioning on as keywords: an unknown one is a TypeError that names it, a known one reaches
  ``conditioning.Conditioning``, and ``generate_bucketed`` takes no latents;
* ``motion_long.canvas_conditioning``: every ValueError it raises, and the joint-clip branch with the CPU restatement
  tests/motion_features_ref.py injected for the kernel, equal to the same rows given as ``edit_motion``;
* ``motion_features.skeleton_for_feats`` and what its callers raise for a width that is neither skeleton's;
* ``_lib.check_lengths`` / ``_lib.mean_std``: the messages of the five callers, letter for letter;
* ``motion_outputs``: the small helpers of the output chain.
"""
import types

import numpy as np
import pytest
import torch

from conftest import pkg

import motion_features_ref as MR


def _trainer():
    Tr = pkg("trainer")
    tr = Tr.DDPMTrainer.__new__(Tr.DDPMTrainer)
    tr.encoder = types.SimpleNamespace(num_frames=16, eval=lambda: None)
    tr.device = "cpu"
    return tr


def test_generate_methods_pass_conditioning_keywords_on():
    tr = _trainer()
    caps, lens = ["a", "b"], torch.tensor([16, 12])
    for method in (tr.generate_batch, tr.generate, tr.generate_bucketed):
        with pytest.raises(TypeError, match="edit_motoin"):
            method(caps, lens, 263, edit_motoin=torch.zeros(2, 16, 263))
        with pytest.raises(ValueError, match="edit_motion and edit_mask go together"):  # a known one reaches Conditioning
            method(caps, lens, 263, edit_motion=torch.zeros(2, 16, 263))
        with pytest.raises(ValueError, match="strength goes with"):
            method(caps, lens, 263, strength=0.5)
    lat = torch.zeros(2, 16, 263)
    with pytest.raises(TypeError, match="latents"):
        tr.generate_bucketed(caps, lens, 263, latents=lat, latent_step=3)
    with pytest.raises(TypeError, match="latent_step"):
        tr.generate_bucketed(caps, lens, 263, latent_step=3)
    with pytest.raises(ValueError, match="latents and latent_step go together"):  # generate takes them
        tr.generate(caps, lens, 263, latents=lat)
    with pytest.raises(TypeError, match="edit_motoin"):
        tr.generate_long([[("a", 16)]], 263, overlap=4, edit_motoin=[torch.zeros(16, 263)])
    with pytest.raises(TypeError, match="edit_motoin"):  # through an output method's **kw
        tr.generate_joints(caps, lens, 263, np.zeros(263), np.ones(263), edit_motoin=1)


def _ref_skel():
    sk = pkg("motion_features").SKELETONS["t2m"]
    return MR.skeleton_from_tables(sk.chains, sk.raw_offsets, sk.face, sk.feet, sk.legs)


def _to_motion(clips, lengths, mean, std, *, skeleton="t2m"):
    """``motion_features.joints_to_motion``'s signature on the CPU restatement."""
    assert lengths is None and skeleton == "t2m"
    rows, _ = MR.joints_to_motion(_ref_skel(), [c.numpy().astype(np.float64) for c in clips], mean, std)
    return torch.from_numpy(rows)


def test_canvas_conditioning_joint_clips_are_their_rows():
    ML, E = pkg("motion_long"), pkg("motion_edit")
    plans = ML.script_plans([[("a", 16), ("b", 16)], [("c", 12)]], 4, 16)
    assert [p[3] for p in plans] == [28, 12]
    sk = _ref_skel()
    gen = torch.Generator().manual_seed(2)
    mean, std = (torch.randn(263, generator=gen) * 0.1).numpy(), (0.5 + torch.rand(263, generator=gen)).numpy()
    clips = [torch.from_numpy(MR.synth_clip(sk, n, 300 + n)).float() for n in (13, 5)]
    masks = [E.prefix_mask(28, 12), E.prefix_mask(12, 3)]
    rows = _to_motion(clips, None, mean, std)
    known = [torch.zeros(28, 263), torch.zeros(12, 263)]
    known[0][:12], known[1][:4] = rows[0, :12], rows[1, :4]
    a = ML.canvas_conditioning(plans, 263, edit_joints=clips, edit_mask=masks, mean=mean, std=std, to_motion=_to_motion)
    b = ML.canvas_conditioning(plans, 263, edit_motion=known, edit_mask=masks)
    for idx, T in (([0, 1], 16), ([1], 12)):
        ra, rb = a(idx, T), b(idx, T)
        assert sorted(ra) == sorted(rb) == ["edit_mask", "edit_motion"]
        assert ra["edit_motion"].shape == (sum(len(plans[i][1]) for i in idx), T, 263)
        assert torch.equal(ra["edit_motion"], rb["edit_motion"]) and torch.equal(ra["edit_mask"], rb["edit_mask"])
    both = a([0, 1], 16)["edit_motion"]
    assert torch.equal(both[0, :12], rows[0, :12]) and not both[0, 12:].any()  # window 0 of motion 0: the clip's rows, then zeros
    assert not both[1].any() and torch.equal(both[2, :4], rows[1, :4])         # window 1 starts at canvas frame 12
    assert bool(both[0, :12].any())
    assert ML.canvas_conditioning(plans, 263)([0, 1], 16) == {}


def test_canvas_conditioning_errors():
    ML, E = pkg("motion_long"), pkg("motion_edit")
    plans = ML.script_plans([[("a", 16), ("b", 16)], [("c", 12)]], 4, 16)
    mean, std = np.zeros(263, np.float32), np.ones(263, np.float32)
    clips = [torch.randn(13, 22, 3, generator=torch.Generator().manual_seed(1)), torch.randn(5, 22, 3, generator=torch.Generator().manual_seed(2))]
    masks = [E.prefix_mask(28, 12), E.prefix_mask(12, 4)]
    canv = [torch.zeros(28, 263), torch.zeros(12, 263)]

    def stub(clips, lengths, mean, std, *, skeleton="t2m"):
        return torch.ones(len(clips), max(c.shape[0] for c in clips) - 1, 263)

    def cc(**kw):
        return ML.canvas_conditioning(plans, 263, to_motion=stub, **kw)

    bad = [
        (dict(bvh_options=dict(scale=2.0)), "bvh_options goes with edit_bvh"),
        (dict(edit_bvh=["a.bvh", "b.bvh"], edit_joints=clips, edit_mask=masks), "edit_bvh, edit_joints and edit_motion are exclusive"),
        (dict(edit_bvh=["a.bvh", "b.bvh"], edit_motion=canv, edit_mask=masks), "edit_bvh, edit_joints and edit_motion are exclusive"),
        (dict(edit_bvh=["a.bvh", "b.bvh"], bvh_options=dict(euler="ZXY"), edit_mask=masks), "bvh_options takes"),
        (dict(edit_joints=clips, edit_motion=canv, edit_mask=masks, mean=mean, std=std), "edit_joints and edit_motion are exclusive"),
        (dict(edit_joints=clips, mean=mean, std=std), r"edit_joints needs one clip and one edit_mask per motion \(2\)"),
        (dict(edit_joints=clips[:1], edit_mask=masks, mean=mean, std=std), "one clip and one edit_mask per motion"),
        (dict(edit_joints=clips, edit_mask=masks[:1], mean=mean, std=std), "one clip and one edit_mask per motion"),
        (dict(edit_joints=clips, edit_mask=[masks[0], None], mean=mean, std=std), "one clip and one edit_mask per motion"),
        (dict(edit_joints=clips, edit_mask=masks), "edit_joints needs the dataset's mean and std"),
        (dict(edit_joints=[clips[0], torch.zeros(14, 22, 3)], edit_mask=masks, mean=mean, std=std),
         "motion 1: a clip of 13 rows does not fit its canvas of 12 frames"),
        (dict(edit_joints=clips, edit_mask=[masks[0], E.prefix_mask(12, 5)], mean=mean, std=std), "one frame short"),
        (dict(init_motion=canv), "init_motion and strength go together"),
        (dict(strength=0.5), "init_motion and strength go together"),
        (dict(noise=canv[:1]), r"noise must hold one entry per motion \(2\), not 1"),
        (dict(init_motion=canv + canv, strength=0.5), r"init_motion must hold one entry per motion \(2\), not 4"),
        (dict(edit_motion=canv), "edit_motion and edit_mask go together: give both or neither"),
        (dict(edit_mask=masks), "edit_motion and edit_mask go together: give both or neither"),
        (dict(edit_motion=canv, edit_mask=[masks[0], None]), "motion 1: edit_motion and edit_mask go together"),
        (dict(edit_motion=[canv[0], None], edit_mask=[masks[0], None]), "edit_motion must be given for every motion of the call or for none"),
        (dict(noise=[None, canv[1]]), "noise must be given for every motion of the call or for none"),
        (dict(init_motion=[canv[0], None], strength=0.5), "init_motion must be given for every motion"),
    ]
    for kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            cc(**kw)
    with pytest.raises(TypeError, match="control_joints"):
        cc(control_joints=canv)
    # what only a batch can tell: a canvas of another shape, a mask that does not broadcast to its canvas
    for name, kw in (("noise", {}), ("init_motion", dict(strength=0.5)), ("edit_motion", dict(edit_mask=masks))):
        rows = cc(**{name: [canv[0], torch.zeros(11, 263)]}, **kw)
        assert rows([0], 16)[name].shape == (2, 16, 263)
        with pytest.raises(ValueError, match=rf"{name} of motion 1 must be \(12, 263\)"):
            rows([0, 1], 16)
    with pytest.raises(ValueError, match=r"edit_mask of motion 1 has shape \(11, 1\), not broadcastable to its canvas \(12, 263\)"):
        cc(edit_motion=canv, edit_mask=[masks[0], E.prefix_mask(11, 3)])([1], 12)


def test_skeleton_for_feats_and_its_callers():
    MF, Cd, MO = pkg("motion_features"), pkg("conditioning"), pkg("motion_outputs")
    assert MF.skeleton_for_feats(263) == "t2m" and MF.skeleton_for_feats(251) == "kit" and MF.skeleton_for_feats(100) is None
    assert MF.skeleton_for_feats(263, strict=True) == "t2m" and MF.skeleton_for_feats(251, strict=True) == "kit"
    assert all(MF.SKELETONS[MF.skeleton_for_feats(f)].feats == f for f in (263, 251))
    with pytest.raises(KeyError, match="100"):
        MF.skeleton_for_feats(100, strict=True)
    mean, std = np.zeros(100), np.ones(100)
    with pytest.raises(ValueError, match=r"edit_joints needs dim_pose 263 \(HumanML3D\) or 251 \(KIT\), not 100"):
        Cd.edit_rows_from_joints([torch.zeros(4, 22, 3)], mean, std, 100)
    with pytest.raises(KeyError, match="100"):
        _trainer().refeaturize([torch.zeros(6, 100)], [6], mean, std)
    with pytest.raises(ValueError, match=r"fix_feet needs dim_pose 263 \(22 joints\) or 251 \(21\), not 100 \(22\)"):
        MO.to_joints([torch.zeros(6, 100)], [6], 100, mean, std, 22, 1.0, fix_feet=True)
    with pytest.raises(ValueError, match=r"forward kinematics needs dim_pose 263 \(22 joints\) or 251 \(21\), not 100 \(8\)"):
        MO.to_bvh([torch.zeros(6, 100)], [6], 100, mean, std, None, False, 5, None, None, None, "ZXY", 1.0)
    assert MO.to_gifs([], 100, None, None) == [] and MO.to_gifs([], 251, [], None) == []  # any width has a default frame rate


def test_check_lengths_and_mean_std_messages():
    L = pkg("_lib")
    got = L.check_lengths(torch.tensor([[3.0, 1.0]]), 2, 3)
    assert got.dtype == torch.int64 and got.device.type == "cpu" and got.tolist() == [3, 1]
    assert L.check_lengths([2, 5], 2, 5, least=2).tolist() == [2, 5] and L.check_lengths([], 0, 4).numel() == 0
    for least, why in ((1, ""), (2, ": n frames give n - 1 rows")):
        with pytest.raises(ValueError, match=r"^lengths must have 2 entries$"):
            L.check_lengths([4], 2, 4, least, why)
        for bad in ([least - 1, 4], [4, 5]):
            with pytest.raises(ValueError) as e:
                L.check_lengths(bad, 2, 4, least, why)
            assert str(e.value) == f"every length must lie in [{least}, 4]" + why
    for bad in ([4], [0, 4], [4, 5]):
        with pytest.raises(ValueError) as e:
            L.check_lengths(bad, 2, 4, message="lengths must have 2 entries in [1, 4]")
        assert str(e.value) == "lengths must have 2 entries in [1, 4]"
    mean, std = L.mean_std([0.0] * 4, np.ones((2, 2)), 4)
    assert mean.dtype == std.dtype == torch.float32 and mean.shape == std.shape == (4,)
    third = L.mean_std(np.full(4, 1 / 3), np.ones(4), 4, torch.float64)[0]
    assert third.dtype == torch.float64 and float(third[0]) == 1 / 3  # fp64 in, fp64 kept
    for m, s in ((np.zeros(3), np.ones(4)), (np.zeros(4), np.ones(5))):
        with pytest.raises(ValueError, match=r"^mean/std must have 4 entries$"):
            L.mean_std(m, s, 4)
    for m, s in ((np.full(4, np.inf), np.ones(4)), (np.zeros(4), np.full(4, np.nan))):
        with pytest.raises(ValueError, match=r"^mean / std have non-finite values$"):
            L.mean_std(m, s, 4)
    with pytest.raises(ValueError, match=r"^std has zero entries$"):
        L.mean_std(np.zeros(4), np.array([1.0, 0.0, 1.0, 1.0]), 4)
    L.mean_std(np.full(4, np.nan), np.zeros(4), 4, values=False)  # the caller checks what it reads
    # through the callers: the same words
    P, MF, MRig = pkg("postprocess"), pkg("motion_features"), pkg("motion_rig")
    z, o = np.zeros(263), np.ones(263)
    sk = MF.SKELETONS["t2m"]
    with pytest.raises(ValueError, match=r"^every length must lie in \[1, 6\]$"):
        P.check_fk(torch.zeros(2, 6, 263), z, o, [0, 6], None, sk)
    with pytest.raises(ValueError, match=r"^lengths must have 2 entries$"):
        P.check_foot_skate(torch.zeros(2, 6, 22, 3), [6], None, None, sk)
    with pytest.raises(ValueError, match=r"^mean/std must have 263 entries$"):
        P.check_foot_skate(torch.zeros(2, 6, 22, 3), None, (torch.zeros(2, 6, 263), z[:262], o), None, sk)
    with pytest.raises(ValueError, match=r"^every length must lie in \[2, 6\]: n frames give n - 1 rows$"):
        MF.check_joints(torch.zeros(2, 6, 22, 3), [1, 6], None, None, sk)
    with pytest.raises(ValueError, match=r"^std has zero entries$"):
        MF.check_joints(torch.zeros(2, 6, 22, 3), None, z, z, sk)
    with pytest.raises(ValueError, match=r"^every length must lie in \[1, 6\]$"):
        MRig.check_rig(torch.zeros(2, 6, 22, 3), torch.zeros(2, 6, 22, 3, 3), [6, 7], "t2m")


def test_output_chain_helpers():
    MO, Tr = pkg("motion_outputs"), pkg("trainer")
    motions = [torch.zeros(16, 263), torch.zeros(16, 263), torch.zeros(12, 263)]
    assert MO.valid_lengths(motions, torch.tensor([16, 9, 13])) == [16, 9, 12]  # the third batch was cut to the window
    assert MO.valid_lengths(motions) == [16, 16, 12]
    MO.check_paths(None, 3, "caption")
    MO.check_paths(["a", None, "c"], 3, "caption")
    with pytest.raises(ValueError, match=r"^paths must hold one entry per caption \(3\), or None$"):
        MO.check_paths(["a"], 3, "caption")
    with pytest.raises(ValueError, match=r"^paths must hold one entry per motion \(1\), or None$"):
        MO.check_paths([], 1, "motion")
    P = pkg("postprocess")
    assert MO.canvas_frame_limit() == MO.MAX_JOINTS_FRAMES == Tr.MAX_JOINTS_FRAMES == 3276
    assert MO.canvas_frame_limit(True) == P.fk_max_frames()
    tr = _trainer()
    mean, std = np.zeros(263), np.ones(263)
    with pytest.raises(ValueError, match="a canvas of 6004 frames: joint recovery takes at most 3276 frames"):
        tr.generate_long_joints([[("a", 16)] * 500], 263, mean, std, overlap=4, batch_size=500)
    with pytest.raises(ValueError, match=f"a canvas of 6004 frames: forward kinematics takes at most {P.fk_max_frames()} frames"):
        tr.generate_long_bvh([[("a", 16)] * 500], 263, mean, std, overlap=4, batch_size=500)
    for call in (lambda: tr.generate_bvh(["a"], [16], 263, mean, std, paths=[]),
                 lambda: tr.generate_gif(["a"], [16], 263, mean, std, paths=["a", "b"])):
        with pytest.raises(ValueError, match=r"one entry per caption \(1\)"):
            call()
    for call in (lambda: tr.generate_long_bvh([[("a", 16)]], 263, mean, std, paths=[]),
                 lambda: tr.generate_long_gif([[("a", 16)]], 263, mean, std, paths=["a", "b"])):
        with pytest.raises(ValueError, match=r"one entry per motion \(1\)"):
            call()

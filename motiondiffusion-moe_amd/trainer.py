"""Sampling half of the reference's ``DDPMTrainer`` (text2motion/trainers/ddpm_trainer.py:28-71,145-199,246-289).

Same constructor arguments (``args.device``, ``args.diffusion_steps``, ``args.is_train``, optional ``cfg_scale``),
same ``generate(caption, m_lens, dim_pose, batch_size)`` -> list of (T, dim_pose) tensors, same checkpoint dict keys
(``encoder``, ``ep``, ``total_it``, ``opt_encoder``).  The generate methods also take ``sampler`` ("ddpm" | "ddim" |
"dpmpp2m"), ``sample_steps`` and ``eta``: few-step guided sampling of the same model on a respaced schedule; the defaults
run the reference's guided DDPM over every step.  ``edit_motion`` / ``edit_mask`` turn any of them into motion editing
(prefix completion, in-betweening, body-part regeneration; masks from ``motion_edit``).  ``prompt_weights`` with K
captions per sample composes them under per-prompt weight maps (time-varied and body-part control, negative prompts;
weights from ``motion_compose``).  ``edit_joints`` gives the known motion of an edit as joint positions, ``edit_bvh`` as
BVH files from any rig (``motion_rig.bvh_to_joints``), and
``refeaturize`` makes all columns of generated rows describe the joints they show (``motion_features``).
``control_joints`` / ``control_weights`` (with ``mean`` / ``std``) steer joint positions:
trajectories, keyframes, end positions (targets from ``motion_control``).  ``generate_long`` samples motions longer than
the model's window from scripts of ``(caption, length)`` segments, overlapping windows tied together on every step
(``motion_long``).  ``generate_bvh`` / ``generate_long_bvh`` end in BVH text for a rig (``motion_rig``,
DESIGN.md §19).  ``init_motion`` / ``init_joints`` / ``init_bvh`` with ``strength`` start from a given motion instead of
from noise: the motion is noised part of the way and only the remaining steps run; ``invert`` runs DDIM inversion and
``generate(latents=, latent_step=)`` continues from its result.  Every generate method checks its
conditioning once (``conditioning.Conditioning``, the one description of its keywords) and samples each batch's rows through
``_sample_rows``; the output methods run ``motion_outputs`` on what a generate method returned.  The training loop
(forward/backward/update/train) is out of scope for this build and raises.
"""
from __future__ import annotations

import numpy as np
import torch
from torch.nn.utils.rnn import pad_sequence

from . import motion_long as ML
from . import motion_outputs as MO
from .conditioning import Conditioning, LatentStep, pad_frames, strength_steps
from .diffusion import (GaussianDiffusion, LossType, ModelMeanType, ModelVarType, SpacedDiffusion, get_named_beta_schedule,
                        space_timesteps)
from .motion_outputs import MAX_JOINTS_FRAMES  # noqa: F401  (the longest canvas generate_long_joints takes)

SAMPLERS = ("ddpm", "ddim", "dpmpp2m")


class DDPMTrainer(object):
    def __init__(self, args, encoder):
        self.opt = args
        self.device = args.device
        self.encoder = encoder
        self.diffusion_steps = args.diffusion_steps
        self._diffusion_kw = dict(betas=get_named_beta_schedule("linear", self.diffusion_steps),
                                  model_mean_type=ModelMeanType.EPSILON, model_var_type=ModelVarType.FIXED_SMALL,
                                  loss_type=LossType.MSE)
        self.diffusion = GaussianDiffusion(**self._diffusion_kw)
        self._spaced = {}  # (sampler, steps) -> SpacedDiffusion
        self.sampler_name = "uniform"
        self.to(self.device)
        self.cfg_scale = getattr(args, "cfg_scale", 7.5)

    def _model(self):
        return self.encoder.module if hasattr(self.encoder, "module") else self.encoder

    def to(self, device):
        self._model().to(device)

    def train_mode(self):
        self._model().train()

    def eval_mode(self):
        self._model().eval()

    def sampling_diffusion(self, sampler: str = "ddpm", sample_steps=None) -> GaussianDiffusion:
        """The diffusion a generate call samples with: the trainer's own schedule when ``sample_steps`` is None or the
        whole schedule, else a SpacedDiffusion of ``sample_steps`` steps (stride-spaced "ddimN" when an integer stride
        gives exactly that many, evenly spaced over the whole schedule otherwise), cached per (sampler, steps)."""
        if sampler not in SAMPLERS:
            raise ValueError(f"sampler must be one of {SAMPLERS}, not {sampler!r}")
        n = self.diffusion_steps if sample_steps is None else int(sample_steps)
        if not 1 <= n <= self.diffusion_steps:
            raise ValueError(f"sample_steps must lie in [1, {self.diffusion_steps}]")
        if n == self.diffusion_steps:
            return self.diffusion
        if (sampler, n) not in self._spaced:
            try:
                use = space_timesteps(self.diffusion_steps, f"ddim{n}")
            except ValueError:
                use = space_timesteps(self.diffusion_steps, [n])
            self._spaced[(sampler, n)] = SpacedDiffusion(use, **self._diffusion_kw)
        return self._spaced[(sampler, n)]

    def _sample_rows(self, cond, rows, lengths, T, sampler, sample_steps, eta, extra=None, **kw):
        """Sample the batch of rows ``rows`` (a slice or an index tensor) of the call ``cond`` conditions, at T frames,
        with the call's sampler: ``model_kwargs`` are the rows' share of the conditioning, ``lengths`` and ``extra``."""
        m, shape = self._model(), (len(cond.captions_of(rows)), T, cond.dim_pose)
        kw = dict(kw, cfg_scale=self.cfg_scale, clip_denoised=False,
                  model_kwargs={**cond.kwargs(rows, T, self.device), "length": lengths, **(extra or {})})
        if eta != 0.0 and sampler != "ddim":
            raise ValueError("eta applies to the ddim sampler only")
        d = self.sampling_diffusion(sampler, sample_steps)
        start, done = cond.start_kwargs(rows, T, lengths, d.num_timesteps, sampler, self.device)
        if done is not None:  # a strength that runs no step: the given motion
            return done
        if "noise" in start and kw.get("noise") is not None:
            raise ValueError("latents are the start of the loop: noise / noises cannot be given as well")
        kw.update(start)
        if sampler == "ddpm":
            return d.p_sample_loop_with_cfg(m, shape, **kw)
        if sampler == "ddim":
            return d.ddim_sample_loop_with_cfg(m, shape, eta=eta, **kw)
        return d.dpm_solver_sample_loop_with_cfg(m, shape, order=2, **kw)

    @torch.no_grad()
    def generate_batch(self, caption, m_lens, dim_pose, *, noise=None, step_noise=None, progress=True, seed=None,
                       sample_offset=0, sampler="ddpm", sample_steps=None, eta=0.0, **conditioning):
        """One batch.  ``noise`` / ``step_noise`` replace the draws; with ``seed`` sample i's noise is a function of (seed,
        ``sample_offset`` + i).  ``**conditioning``: the edit, prompt, control, start and latent inputs, each described once in
        ``conditioning.Conditioning`` (N = B there)."""
        cond = Conditioning(caption, dim_pose, device=self.device, **conditioning)
        m_lens = torch.as_tensor(m_lens)
        T = min(int(m_lens.max()), self._model().num_frames)
        return self._sample_rows(cond, slice(0, len(caption)), m_lens, T, sampler, sample_steps, eta, progress=progress,
                                 noise=noise, step_noise=step_noise, seed=seed, sample_offset=sample_offset)

    @torch.no_grad()
    def generate(self, caption, m_lens, dim_pose, batch_size=8, *, progress=False, seed=None, noises=None, sampler="ddpm",
                 sample_steps=None, eta=0.0, sample_offset=0, model_extra=None, **conditioning):
        """``seed``: sample i's noise is then a function of (seed, i) only (counter-based device generator), so the result
        does not depend on ``batch_size``; without it the torch generator is used, as in the reference.
        ``noises``: optional list with one ``(x_T, [step noise, ...])`` pair per batch, replacing the draws (parity tests).
        ``sampler`` / ``sample_steps`` / ``eta``: see ``sampling_diffusion``; e.g. ``sampler="dpmpp2m", sample_steps=20``.
        ``**conditioning``: motion editing, composed prompts, joint-position control, a motion or latents to start from; see
        ``conditioning.Conditioning``, the one description of every such keyword.  Each batch takes its samples' rows and
        its first T frames of them.  ``sample_offset``: the call's samples are samples ``sample_offset`` ... of a larger one
        (under ``seed`` sample i's noise is a function of (seed, sample_offset + i)).  ``model_extra``: further ``model_kwargs``
        that name the rows of one batch (``control_partner_*`` / ``control_contact_*``): the call must then
        be one batch."""
        N = len(caption)
        if model_extra and N > batch_size:
            raise ValueError(f"model_extra names the rows of one batch: {N} samples do not fit batch_size = {batch_size}")
        self.eval_mode()
        cond = Conditioning(caption, dim_pose, device=self.device, **conditioning)
        all_output = []
        for cur in range(0, N, batch_size):
            end = min(cur + batch_size, N)
            x_T, step_noise = noises[cur // batch_size] if noises is not None else (None, None)
            lens = torch.as_tensor(m_lens[cur:end])
            T = min(int(lens.max()), self._model().num_frames)
            out = self._sample_rows(cond, slice(cur, end), lens, T, sampler, sample_steps, eta, progress=progress,
                                    noise=x_T, step_noise=step_noise, seed=seed, sample_offset=sample_offset + cur,
                                    **({"extra": model_extra} if model_extra else {}))
            all_output.extend(out[i] for i in range(out.shape[0]))
        return all_output

    @torch.no_grad()
    def generate_bucketed(self, caption, m_lens, dim_pose, batch_size=32, *, unit_length=4, seed=None, group=None,
                          progress=False, sampler="ddpm", sample_steps=None, eta=0.0, **conditioning):
        """Evaluation-scale variant of ``generate``: same inputs and the same kind of result (a
        list of per-sample ``(T_batch, dim_pose)`` tensors in the caller's order, valid up to each sample's length),
        but batches hold samples of similar length (less padded work) and, under ``torch.distributed``, are dealt over
        the ranks with one all_gather at the end.  With ``seed`` every sample's noise is a function of (seed, its index in
        ``caption``) only -- the same as ``generate(..., seed=)`` -- so on each sample's valid frames the two give identical
        results whatever the bucketing (tests/test_sampler_gpu.py).  ``**conditioning``: as in ``generate``, each bucket taking
        its samples' rows and its first T frames, but for ``latents`` / ``latent_step``, which it does not take."""
        from . import dist as D
        for name in ("latents", "latent_step"):
            if name in conditioning:
                raise TypeError(f"generate_bucketed() got an unexpected keyword argument {name!r}")
        m = self._model()
        self.eval_mode()
        cond = Conditioning(caption, dim_pose, device=self.device, **conditioning)
        lens = torch.as_tensor(m_lens).flatten().long().cpu()
        plan = D.plan_buckets(lens, batch_size, m.num_frames, unit_length)

        def run_bucket(k, idx, T):  # noise keyed on each row's index in the CALLER's list: == generate(seed=)
            return self._sample_rows(cond, idx, lens[idx].clamp(max=T).to(self.device), T, sampler, sample_steps, eta,
                                     progress=progress, seed=seed, sample_offset=idx)

        return D.run_plan(plan, run_bucket, len(caption), m.num_frames, dim_pose, self.device, group)

    @torch.no_grad()
    def invert(self, caption, motions, m_lens, dim_pose, *, sample_steps=50, to_strength=1.0, cfg_scale=1.0, batch_size=8,
               progress=False):
        """DDIM inversion of given motions under their captions (``ddim_invert_loop``): ``motions`` is
        (N, T_max, dim_pose) or a list of (T_i, dim_pose), normalised, each covering its ``m_lens`` entry.  Runs upwards on
        the ``sample_steps``-step DDIM schedule to the step a ``strength=to_strength`` call would start at,
        ``round(to_strength * sample_steps) - 1``, at ``cfg_scale`` (1.0: the caption alone, the scale at which a
        regeneration under the same caption retraces the inversion).  Returns ``(latents, latent_step)``: a list of
        (T_batch, dim_pose) tensors and the step they stand at, for ``generate(..., sampler="ddim", sample_steps=,
        latents=, latent_step=)``."""
        N = len(caption)
        self.eval_mode()
        d = self.sampling_diffusion("ddim", sample_steps)
        n_run = strength_steps(to_strength, d.num_timesteps)
        if n_run < 1:
            raise ValueError("to_strength maps to no step: nothing to invert to")
        if not torch.is_tensor(motions):
            clips = [torch.as_tensor(v) for v in motions]
            motions = torch.stack([pad_frames(v[None], max(u.shape[0] for u in clips))[0] for v in clips])
        if motions.dim() != 3 or motions.shape[0] != N or motions.shape[2] != dim_pose:
            raise ValueError(f"motions of shape {tuple(motions.shape)} must be (N = {N}, T_max, {dim_pose})")
        out = []
        for cur in range(0, N, batch_size):
            end = min(cur + batch_size, N)
            lens = torch.as_tensor(m_lens[cur:end])
            T = min(int(lens.max()), self._model().num_frames)
            if motions.shape[1] < T:
                raise ValueError(f"motions has {motions.shape[1]} frames, the batch {T}")
            x = d.ddim_invert_loop(self._model(), motions[cur:end, :T].to(self.device, torch.float32),
                                   {"text": caption[cur:end], "length": lens}, to_step=n_run - 1, cfg_scale=cfg_scale,
                                   progress=progress)
            out.extend(x[i] for i in range(x.shape[0]))
        return out, LatentStep(n_run - 1, d.num_timesteps)

    @torch.no_grad()
    def generate_for_evaluation(self, caption, m_lens, dim_pose, *, mm_num_samples=0, mm_num_repeats=1, unit_length=4,
                                max_motion_length=196, dataset_name="t2m", seed=None, batch_size=32, sampler="ddpm",
                                sample_steps=None, eta=0.0, group=None, consistent_features=False, mean=None, std=None):
        """The generation half of the reference's ``EvaluationDataset`` (datasets1/evaluator.py:16-121) on
        ``generate_bucketed``: lengths snapped to ``max(m // unit * unit, min_mov_length * unit)`` (min_mov_length 10 for
        t2m, 6 for KIT) and capped at ``max_motion_length``; ``mm_num_samples`` captions, drawn with
        ``RandomState(seed).choice(N, mm_num_samples, replace=False)`` and sorted, are generated ``mm_num_repeats`` times.
        Frames at or past each length are zero, as the reference's dataset pads them.  Returns a dict:
          motions (N, max_motion_length, dim_pose) and m_lens (N,): the first generation of every caption
          mm_idxs (P,), mm_motions (P, mm_num_repeats, max_motion_length, dim_pose), mm_lens (P, mm_num_repeats).
        ``consistent_features`` (with ``mean`` / ``std``): every generated motion goes through ``refeaturize`` before it is
        padded, so all its columns describe the joints its root and position columns show; a motion of n frames then has
        n - 1 rows, and ``m_lens`` / ``mm_lens`` count those.  Off by default: the result is then unchanged."""
        import numpy as np
        N = len(caption)
        if mm_num_samples and not mm_num_samples < N:
            raise ValueError("mm_num_samples must be smaller than the number of captions (evaluator.py:19)")
        min_mov = 10 if dataset_name == "t2m" else 6
        lens = torch.as_tensor(m_lens).flatten().long().cpu()
        lens = torch.clamp(torch.clamp(lens // unit_length * unit_length, min=min_mov * unit_length), max=max_motion_length)
        mm_idxs = np.sort(np.random.RandomState(seed).choice(N, mm_num_samples, replace=False)) if mm_num_samples else \
            np.zeros(0, dtype=np.int64)
        mm_set = set(mm_idxs.tolist())
        all_cap, all_len, first = [], [], []
        for i in range(N):
            first.append(len(all_cap))
            for _ in range(mm_num_repeats if i in mm_set else 1):
                all_cap.append(caption[i])
                all_len.append(int(lens[i]))
        gen = self.generate_bucketed(all_cap, torch.tensor(all_len), dim_pose, batch_size, unit_length=unit_length, seed=seed,
                                     group=group, sampler=sampler, sample_steps=sample_steps, eta=eta)
        if consistent_features:
            if mean is None or std is None:
                raise ValueError("consistent_features needs the dataset's mean and std")
            all_len = MO.valid_lengths(gen, all_len)
            gen = self.refeaturize(gen, all_len, mean, std)
            all_len, lens = [n - 1 for n in all_len], lens - 1
        allm = torch.zeros((len(all_cap), max_motion_length, dim_pose), dtype=torch.float32, device=gen[0].device)
        for k, (mo, n) in enumerate(zip(gen, all_len)):
            n = min(n, mo.shape[0])
            allm[k, :n] = mo[:n]  # frames at or past the length stay zero
        sel = torch.tensor(first, dtype=torch.long, device=allm.device)
        out = {"motions": allm.index_select(0, sel), "m_lens": lens.clone(), "mm_idxs": mm_idxs}
        rows = [first[i] + r for i in mm_idxs.tolist() for r in range(mm_num_repeats)]
        P = len(mm_idxs)
        out["mm_motions"] = allm[torch.tensor(rows, dtype=torch.long, device=allm.device)].reshape(
            P, mm_num_repeats, max_motion_length, dim_pose) if P else allm[:0].reshape(0, mm_num_repeats, max_motion_length, dim_pose)
        out["mm_lens"] = lens[torch.as_tensor(mm_idxs, dtype=torch.long)].reshape(P, 1).repeat(1, mm_num_repeats)
        return out

    @torch.no_grad()
    def refeaturize(self, motions, m_lens, mean, std):
        """``motion_features.refeaturize`` over the first ``m_lens[i]`` frames of every motion (normalised rows, as the
        generate methods return them): a list of ``(m_len - 1, dim_pose)`` rows that show the same joints under
        ``recover_from_ric`` and whose rot6d, velocity and foot-contact columns describe those joints.  One launch of each
        kernel for all."""
        from .motion_features import refeaturize, skeleton_for_feats
        lens = MO.valid_lengths(motions, m_lens)
        x = pad_sequence([mo[:n] for mo, n in zip(motions, lens)], batch_first=True)
        rows = refeaturize(x, mean, std, torch.tensor(lens), skeleton=skeleton_for_feats(x.shape[-1], strict=True))
        return [rows[i, :n - 1] for i, n in enumerate(lens)]

    @torch.no_grad()
    def generate_joints(self, caption, m_lens, dim_pose, mean, std, batch_size=8, *, joints_num=22, sigma=1.0,
                        bucketed=False, from_rotations=False, offsets=None, fix_feet=False, blend=5, pin_targets=False,
                        pin_blend=5, **kw):
        """``generate`` followed by the reference's post-processing (tools/visualization.py:21-27,89) on the device:
        list of ``(m_len, joints_num, 3)`` joint positions, temporally smoothed with a gaussian of width ``sigma``.
        ``edit_motion`` / ``edit_mask``: motion editing in normalised feature space, as in ``generate``;
        ``prompt_weights``: composed prompts, as in ``generate``; ``control_joints`` / ``control_weights`` /
        ``control_scale`` / ``control_iters``: joint-position control under this call's ``mean`` / ``std``; ``scene`` /
        ``scene_joint_radius`` / ``scene_joint_weights``: obstacles the joints keep out of, under the same;
        ``scene_tracks``: obstacles that move, e.g. ``motion_scene.character_tracks`` of another character;
        ``edit_joints`` (through ``**kw``): joint clips in place of ``edit_motion``, converted under the same ``mean`` /
        ``std``.  ``from_rotations``: joints by forward kinematics of the rot6d columns (``postprocess.motion_to_joints_fk``,
        DESIGN.md §17: rigid bones) on ``offsets`` (J, 3) or one (J, 3) per motion; None: every motion's own mean bone
        lengths.  ``fix_feet``: foot-skate clean-up after the temporal filter (``postprocess.remove_foot_skate``, DESIGN.md
        §18), the labels being the generated rows' own foot-contact columns; ``blend`` frames of fade either side of a contact.
        ``pin_targets``: exact reach (``postprocess.pin_limbs``) as the last stage: where this call's
        ``control_joints`` / ``control_weights`` weight all three coordinates of a wrist or an ankle, the joint is put on its
        target by two-bone IK of its limb, ``pin_blend`` frames of fade either side; without them a ValueError."""
        pin = MO.pin_of(pin_targets, kw)
        gen = self.generate_bucketed if bucketed else self.generate  # mean / std go along: unused without control
        motions = gen(caption, m_lens, dim_pose, batch_size, mean=mean, std=std, **kw)
        return MO.to_joints(motions, MO.valid_lengths(motions, m_lens), dim_pose, mean, std, joints_num, sigma, from_rotations,
                            offsets, fix_feet=fix_feet, blend=blend, **MO.pin_kw(pin, pin_blend))

    @torch.no_grad()
    def generate_together(self, scenes, dim_pose, mean, std, *, radius=0.08, margin=0.05, weight=5.0, bones=None, seed=None,
                          mutual=False, contacts=None, **kw):
        """Several characters in one world: ``scenes`` is a list of scenes, each a list of characters
        ``dict(caption=, length=, position=(x, z), yaw=, control_joints=, control_weights=, scene=)``; ``position`` / ``yaw``
        (default the origin, 0) place the character's own frame in the world (``motion_scene.to_world``), and targets
        (length, J, 3), their weights (aligned on the frame dim) and the static primitives of ``scene`` are given in world
        coordinates.  Stage i generates character i of every scene that has one in one ``generate_joints`` batch: the
        characters 0 ... i - 1 of its scene, already generated, are obstacles that move, ``motion_scene.character_tracks``
        of their joints (capsules of ``radius`` along ``bones``, ``margin`` and ``weight`` as a primitive's; padding past an
        earlier character's length), moved with the world targets and primitives into character i's own frame.  Earlier
        characters do not react to later ones.  A frame takes ``motion_scene.MAX_TRACKS`` tracks: two earlier characters
        need a ``bones`` subset.  ``weight`` follows §14's rule, ``control_scale`` x curvature < 2.  Returns
        the joints in the world, one list of (length, J, 3) per scene.  ``seed``: stage i samples under ``seed + i``;
        ``**kw`` goes to ``generate_joints`` (``control_scale``, ``control_iters``, the sampler, ``sigma``, ...; with
        ``pin_targets=True`` every character's wrists and ankles end on their targets, moved into its own frame, §28; a stage
        none of whose characters has targets runs without pins).  A scene of
        one character is ``generate_joints`` followed by ``to_world``, bit for bit.
        ``mutual=True``: the characters of a scene are sampled together, rows of one ``generate_joints``
        batch, and on every step each avoids the capsules of the others' current estimate: nobody is furniture, and the
        result depends on no order among them.  Scenes are dealt whole, in order, into batches of at most ``batch_size``
        rows; sample i's noise is a function of (``seed``, its index in the scene-then-character order).  ``contacts``: one
        list per scene of ``motion_scene.contact(a, joint_a, b, joint_b, frames, weight, meet)`` between its characters
        ``a`` / ``b``: both joints are drawn to the meeting point of the current estimate.  ``weight=0`` leaves the avoidance
        out.  With ``pin_targets=True`` every contact's meeting point, computed from the final joints, joins both characters'
        pin targets (``postprocess.pin_limbs`` decides what it can pin).  ValueError for ``contacts`` without ``mutual``, a
        scene of more characters than ``batch_size`` and one whose (C - 1) x len(bones) partner capsules do not fit the
        ``motion_scene.MAX_TRACKS`` tracks of a frame (give a ``bones=`` subset).  ``self_collision`` goes to
        every stage of the sequential mode with the rest of ``**kw``; with ``mutual=True`` it is a NotImplementedError."""
        from . import motion_scene as MS
        J = (dim_pose + 1) // 12
        if contacts is not None and not mutual:
            raise ValueError("contacts join characters that are sampled together: pass mutual=True")
        if mutual and kw.get("self_collision") is not None:
            raise NotImplementedError("self-collision avoidance for characters sampled together is out of scope (DESIGN.md §33): "
                                      "both rewrite the guidance's targets on every step; use mutual=False")
        if mutual:
            return self._generate_mutual(scenes, dim_pose, mean, std, radius, margin, weight, bones, seed, contacts, kw)
        pin = bool(kw.pop("pin_targets", False))
        if pin and not any(c.get("control_joints") is not None for s in scenes for c in s):
            raise ValueError("pin_targets=True pins the characters' own control_joints / control_weights: none has any")
        out = [[None] * len(s) for s in scenes]
        for i in range(max([len(s) for s in scenes] + [0])):
            rows = [k for k, s in enumerate(scenes) if len(s) > i]
            chars = [scenes[k][i] for k in rows]
            lens = [int(c["length"]) for c in chars]
            place = [(tuple(c.get("position", (0.0, 0.0))), float(c.get("yaw", 0.0))) for c in chars]
            tracks = [[t for prev in out[k][:i] for t in MS.character_tracks(MS.to_local(prev, *pl), radius, margin=margin,
                                                                              weight=weight, bones=bones)]
                      for k, pl in zip(rows, place)]
            if max(len(t) for t in tracks) > MS.MAX_TRACKS:
                raise ValueError(f"{max(len(t) for t in tracks)} tracks for character {i} of a scene: a frame takes at most "
                                 f"{MS.MAX_TRACKS}; give a bones= subset")
            static = [MS.records_to_local(MS.pack_scene(c.get("scene") or []), *pl).to(torch.float32) for c, pl in zip(chars, place)]
            cond = {}
            if any(tracks):
                cond["scene_tracks"] = tracks
            if any(s.shape[0] for s in static):
                rec = torch.zeros((len(chars), max(s.shape[0] for s in static), MS.REC))
                for n, s in enumerate(static):
                    rec[n, :s.shape[0]] = s
                cond["scene"] = rec
            if any(c.get("control_joints") is not None for c in chars):
                g, w = torch.zeros((len(chars), max(lens), J, 3)), torch.zeros((len(chars), max(lens), J, 3))
                for n, (c, pl) in enumerate(zip(chars, place)):
                    if c.get("control_joints") is None:
                        continue
                    tg = torch.as_tensor(c["control_joints"], dtype=torch.float32)
                    wt = torch.as_tensor(c["control_weights"], dtype=torch.float32)
                    if tuple(tg.shape) != (lens[n], J, 3):
                        raise ValueError(f"control_joints of shape {tuple(tg.shape)} must be {(lens[n], J, 3)}, in the world")
                    g[n, :lens[n]] = MS.to_local(tg, *pl)
                    w[n, :lens[n]] = wt.reshape(tuple(wt.shape) + (1,) * (3 - wt.dim())).expand(lens[n], J, 3)
                cond.update(control_joints=g, control_weights=w)
            joints = self.generate_joints([c["caption"] for c in chars], torch.tensor(lens), dim_pose, mean, std,
                                          seed=None if seed is None else seed + i, **cond, **kw,
                                          **(dict(pin_targets=True) if pin and "control_joints" in cond else {}))
            for k, pl, j in zip(rows, place, joints):
                out[k][i] = MS.to_world(j, *pl)
        return out

    def _generate_mutual(self, scenes, dim_pose, mean, std, radius, margin, weight, bones, seed, contacts, kw):
        """``generate_together(mutual=True)``: see there."""
        from . import motion_scene as MS
        from .motion_features import skeleton_for_feats
        from .postprocess import pin_limbs
        J = (dim_pose + 1) // 12
        kw = dict(kw)
        pin, pin_blend, batch_size = bool(kw.pop("pin_targets", False)), kw.pop("pin_blend", 5), int(kw.pop("batch_size", 8))
        contacts = [[] for _ in scenes] if contacts is None else [list(c) for c in contacts]
        if len(contacts) != len(scenes):
            raise ValueError(f"contacts must hold one list per scene ({len(scenes)}), not {len(contacts)}")
        if pin and not any(c.get("control_joints") is not None for s in scenes for c in s) and not any(contacts):
            raise ValueError("pin_targets=True pins control_joints / control_weights and contacts: the scenes have neither")
        bone_list = MS.skeleton_bones(J) if bones is None else [(int(p), int(c)) for p, c in bones]
        avoid = float(weight) > 0
        for k, (s, cs) in enumerate(zip(scenes, contacts)):
            if len(s) > batch_size:
                raise ValueError(f"scene {k} has {len(s)} characters, a batch {batch_size} rows: raise batch_size (characters "
                                 "sampled together share a batch; a bones= subset makes room for more partners)")
            if avoid and (len(s) - 1) * len(bone_list) > MS.MAX_TRACKS:
                raise ValueError(f"scene {k}: {len(s) - 1} partners x {len(bone_list)} bones = {(len(s) - 1) * len(bone_list)} "
                                 f"tracks a frame, at most {MS.MAX_TRACKS} are allowed: give a bones= subset")
            for c in cs:
                if not isinstance(c, MS.Contact) or max(c[0], c[2]) >= len(s):
                    raise ValueError(f"scene {k}: contacts are motion_scene.contact(...) entries between its {len(s)} characters")
        batches, cur = [], []  # whole scenes, in order
        for k, s in enumerate(scenes):
            if cur and sum(len(scenes[i]) for i in cur) + len(s) > batch_size:
                batches.append(cur)
                cur = []
            if len(s):
                cur.append(k)
        if cur:
            batches.append(cur)
        first = np.cumsum([0] + [len(s) for s in scenes]).tolist()  # a scene's first row in the flattened order
        out = [[None] * len(s) for s in scenes]
        for batch in batches:
            chars = [c for k in batch for c in scenes[k]]
            base = first[batch[0]]
            row_of = {(k, i): first[k] - base + i for k in batch for i in range(len(scenes[k]))}
            lens = [int(c["length"]) for c in chars]
            place = [(tuple(c.get("position", (0.0, 0.0))), float(c.get("yaw", 0.0))) for c in chars]
            static = [MS.records_to_local(MS.pack_scene(c.get("scene") or []), *pl).to(torch.float32) for c, pl in zip(chars, place)]
            cond = {}
            if any(s.shape[0] for s in static):
                rec = torch.zeros((len(chars), max(s.shape[0] for s in static), MS.REC))
                for n, s in enumerate(static):
                    rec[n, :s.shape[0]] = s
                cond["scene"] = rec
            g = w = None
            if any(c.get("control_joints") is not None for c in chars):
                g, w = torch.zeros((len(chars), max(lens), J, 3)), torch.zeros((len(chars), max(lens), J, 3))
                for n, (c, pl) in enumerate(zip(chars, place)):
                    if c.get("control_joints") is None:
                        continue
                    tg = torch.as_tensor(c["control_joints"], dtype=torch.float32)
                    wt = torch.as_tensor(c["control_weights"], dtype=torch.float32)
                    if tuple(tg.shape) != (lens[n], J, 3):
                        raise ValueError(f"control_joints of shape {tuple(tg.shape)} must be {(lens[n], J, 3)}, in the world")
                    g[n, :lens[n]] = MS.to_local(tg, *pl)
                    w[n, :lens[n]] = wt.reshape(tuple(wt.shape) + (1,) * (3 - wt.dim())).expand(lens[n], J, 3)
                cond.update(control_joints=g, control_weights=w)
            rows_contacts = [MS.Contact((row_of[k, c[0]], c[1], row_of[k, c[2]], c[3]) + tuple(c[4:]))
                             for k in batch for c in contacts[k]]
            multi = avoid and any(len(scenes[k]) > 1 for k in batch)
            extra = None
            if multi or rows_contacts:  # else: nothing to avoid and nothing to reach for, the call generate_joints makes
                extra = dict(control_partner_scenes=[[row_of[k, i] for i in range(len(scenes[k]))] for k in batch],
                             control_partner_placements=torch.tensor([[pl[0][0], pl[0][1], pl[1]] for pl in place],
                                                                     dtype=torch.float64),
                             control_partner_bones=bone_list, control_partner_radius=radius, control_partner_margin=margin,
                             control_partner_weight=weight, control_contact_list=rows_contacts)
                if "scene" not in cond and "control_joints" not in cond:
                    cond["scene"] = []  # the guidance needs mean / std: an empty scene switches it on
            joints = self.generate_joints([c["caption"] for c in chars], torch.tensor(lens), dim_pose, mean, std,
                                          batch_size=len(chars), seed=seed, sample_offset=base,
                                          **(dict(model_extra=extra) if extra else {}), **cond, **kw)
            world = [MS.to_world(j, *pl) for j, pl in zip(joints, place)]
            if pin and (g is not None or rows_contacts):
                tg = torch.zeros((len(chars), max(lens), J, 3)) if g is None else g.clone()
                wt = torch.zeros_like(tg) if w is None else w.clone()
                for a, ja, b, jb, f0, f1, cw, meet in rows_contacts:
                    f1 = min(f1, lens[a], lens[b])
                    if f0 >= f1 or cw <= 0:
                        continue
                    m = world[a][f0:f1, ja] + meet * (world[b][f0:f1, jb] - world[a][f0:f1, ja])
                    for r, jr in ((a, ja), (b, jb)):
                        tg[r, f0:f1, jr] = MS.to_local(m, *place[r]).to(tg)
                        wt[r, f0:f1, jr] = cw
                padded = pad_sequence(list(joints), batch_first=True)
                pinned = pin_limbs(padded, torch.tensor(lens), tg, wt, skeleton=skeleton_for_feats(dim_pose, strict=True),
                                   blend=pin_blend)
                world = [MS.to_world(pinned[n, :lens[n]], *pl) for n, pl in enumerate(place)]
            for k in batch:
                for i in range(len(scenes[k])):
                    out[k][i] = world[row_of[k, i]]
        return out

    @torch.no_grad()
    def generate_rotations(self, caption, m_lens, dim_pose, mean, std, batch_size=8, *, offsets=None, fix_feet=False,
                           blend=5, pin_targets=False, pin_blend=5, **kw):
        """``generate`` followed by forward kinematics (``postprocess.motion_to_joints_fk``): per sample
        ``(joints (m, J, 3), rotations (m, J, 3, 3), offsets (J, 3))``: the joints on rigid bones, unfiltered so that they
        agree with the rotations, the global rotation matrix of every joint (the root's at joint 0) and the bone offsets
        used (``offsets``, or the sample's own mean bone lengths).  ``fix_feet`` / ``blend``: foot-skate clean-up as in
        ``generate_joints``; the rotations of knees, ankles and toes turn with their bones.  ``pin_targets`` / ``pin_blend``:
        exact reach as in ``generate_joints``; the rotations of the pinned limbs turn with them.  ``**kw`` as for ``generate``."""
        pin = MO.pin_of(pin_targets, kw)
        motions = self.generate(caption, m_lens, dim_pose, batch_size, mean=mean, std=std, **kw)  # unused without an edit or control
        return MO.to_joints(motions, MO.valid_lengths(motions, m_lens), dim_pose, mean, std, (dim_pose + 1) // 12, 0.0, True,
                            offsets, True, fix_feet=fix_feet, blend=blend, **MO.pin_kw(pin, pin_blend))

    @torch.no_grad()
    def generate_bvh(self, caption, m_lens, dim_pose, mean, std, batch_size=8, *, paths=None, fps=None, fps_out=None,
                     euler="ZXY", scale=1.0, offsets=None, fix_feet=False, blend=5, target_rig=None, target_joint_map=None,
                     target_up="Y", leg_ik=None, pin_targets=False, pin_blend=5, **kw):
        """``generate`` followed by forward kinematics and the rig export (``motion_rig``): one BVH text per
        sample, written to ``paths[i]`` where given.  ``fps`` (default 20 at dim_pose 263, 12.5 at 251) / ``fps_out``: retimed
        to the frame rate a tool works at; ``euler``: the channels' rotation order; ``scale``: of positions and offsets (100
        for centimetres).  ``offsets`` / ``fix_feet`` / ``blend`` as in ``generate_rotations``, ``**kw`` as for ``generate``:
        with ``edit_bvh=`` / ``edit_mask=`` a file from a rig is continued and written back as one (converted under this
        call's ``mean`` / ``std``).  ``target_rig`` (BVH text, a path or ``motion_rig.target_rig``'s namespace; with
        ``target_joint_map`` / ``target_up``, and ``leg_ik``): the motion is written onto that character's own hierarchy
        (``motion_rig.retarget_to_rig``) in its units, so ``scale`` is refused.  ``pin_targets`` /
        ``pin_blend``: exact reach before the export, as in ``generate_rotations``."""
        MO.check_paths(paths, len(caption), "caption")
        pin = MO.pin_of(pin_targets, kw)
        motions = self.generate(caption, m_lens, dim_pose, batch_size, mean=mean, std=std, **kw)  # unused without an edit or control
        return MO.to_bvh(motions, MO.valid_lengths(motions, m_lens), dim_pose, mean, std, offsets, fix_feet, blend, paths, fps,
                         fps_out, euler, scale, target_rig, target_joint_map, target_up, leg_ik, **MO.pin_kw(pin, pin_blend))

    @torch.no_grad()
    def generate_long(self, scripts, dim_pose, *, overlap=20, blend="linear", batch_size=32, seed=None, sampler="ddpm",
                      sample_steps=None, eta=0.0, progress=False, control_joints=None, control_weights=None, control_scale=None,
                      control_iters=None, scene=None, scene_joint_radius=None, scene_joint_weights=None, scene_tracks=None,
                      terrain=None, terrain_stand=None, terrain_stand_threshold=0.5, self_collision=None, **conditioning):
        """Long motions: ``scripts`` is a list of long motions, each a list of ``(caption, length)``
        segments of at most ``num_frames`` frames; neighbouring segments share ``overlap`` canvas frames, whose eps is
        blended on every step (``blend`` "linear" crossfade or "uniform") while x_T and the step noise come from the left
        window.  Returns one ``(canvas_len, dim_pose)`` tensor per motion, canvas_len = sum(length) - (n - 1) overlap.
        ``batch_size`` counts windows; a motion's windows stay in one batch.  ``seed``: window k of the call (counting
        the windows of all motions in order) is global sample k of the counter-based generator, so the result does not
        depend on ``batch_size``.  ``edit_motion`` / ``edit_mask``: one (canvas_len, dim_pose) known motion per motion and
        a mask broadcastable to it (or None entries), kept where the mask is 1, e.g. a prefix to continue.  ``noise``: one
        (canvas_len, dim_pose) x_T per motion.  ``sampler`` / ``sample_steps`` / ``eta`` as in ``generate``.
        ``edit_joints`` (with ``mean`` / ``std``): one joint clip (n_i, J, 3) per motion in place of ``edit_motion``, e.g. the
        joints ``generate_long_joints`` returned, to be continued: its n_i - 1 rows start the canvas, and every motion
        needs its mask.  ``edit_bvh`` / ``bvh_options``: one BVH file per motion in place of ``edit_joints``, as in
        ``generate``.  ``init_motion`` with ``strength``: one (canvas_len, dim_pose) motion per long motion to start from, as
        in ``generate``: each window takes its frames of the canvas, and an overlap starts from its owner
        window's noised values.  ``control_joints`` / ``control_weights`` (with ``mean`` / ``std``; ``control_scale`` /
        ``control_iters``): one (canvas_len, J, 3) array of target joint positions per motion, in canvas frames, and weights
        broadcastable to it, as in ``generate`` but over the whole canvas (targets from
        ``motion_control.root_path_targets`` / ``keyframe_targets`` at T = canvas_len): a target late in the canvas moves the
        root path of every window before it.  It combines with every sampler and with the edit and start inputs
        (``motion_long.canvas_control`` checks it).  ``scene`` (with ``mean`` / ``std``; ``scene_joint_radius`` /
        ``scene_joint_weights`` (J,)): one list of ``motion_scene`` primitives per motion, in its canvas frame, that the joints
        keep out of on every step, through the same canvas-wide guidance and with or without targets.
        ``scene_tracks``: one list of ``motion_scene`` track stacks per motion, moving obstacles over its canvas frames
        (DESIGN.md §25), under the same.  ``terrain``: one ``motion_scene`` terrain per motion, a height-map ground in its
        canvas frame, with ``terrain_stand`` None, ``"contacts"`` (over ``terrain_stand_threshold``) or one
        (canvas_len, J) array of stand weights per motion, under the same.
        The other per-motion inputs are ``**conditioning``, checked by
        ``motion_long.canvas_conditioning``.  ``self_collision`` is not supported on a canvas (NotImplementedError)."""
        if self_collision is not None:
            raise NotImplementedError("self-collision avoidance over a long motion's canvas is out of scope (DESIGN.md §33): "
                                      "generate the motion in one window, or leave self_collision out")
        m = self._model()
        self.eval_mode()
        plans = ML.script_plans(scripts, overlap, m.num_frames)
        device = getattr(self, "device", None)  # none on a trainer made without __init__ (host tests of the checks)
        window_rows = ML.canvas_conditioning(plans, dim_pose, device=device, **conditioning)
        control = ML.canvas_control(plans, dim_pose, control_joints, control_weights, control_scale, control_iters,
                                    conditioning.get("mean"), conditioning.get("std"), device, scene, scene_joint_radius,
                                    scene_joint_weights, scene_tracks, terrain, terrain_stand, terrain_stand_threshold)
        out, first = [None] * len(plans), 0
        for idx in ML.plan_batches(plans, batch_size):
            caps = [c for i in idx for c in plans[i][0]]
            lens = [n for i in idx for n in plans[i][1]]
            T = max(lens) + max(lens) % 2  # the denoiser takes even T
            kw = ML.batch_tables(plans, idx, T, overlap, blend)
            rows = window_rows(idx, T)  # the per-motion canvases given, as window rows
            if "edit_motion" in rows:
                kw.update(inpaint_motion=rows["edit_motion"], inpaint_mask=rows["edit_mask"])
            kw.update(control(idx, T))
            cond = Conditioning(caps, dim_pose, init_motion=rows.get("init_motion"), strength=conditioning.get("strength"))
            res = self._sample_rows(cond, slice(None), torch.tensor(lens), T, sampler, sample_steps, eta, extra=kw,
                                    progress=progress, noise=rows.get("noise"), seed=seed, sample_offset=first)
            first += len(caps)
            row = 0
            for i in idx:
                n = len(plans[i][1])
                out[i] = ML.windows_to_canvas(res[row:row + n], plans[i][2], plans[i][1])
                row += n
        return out

    def _long_motions(self, scripts, dim_pose, mean, std, most, what, kw):
        """``generate_long`` for an output stage of at most ``most`` canvas frames, clips converted under its ``mean`` / ``std``."""
        longest = max(p[3] for p in ML.script_plans(scripts, kw.get("overlap", 20), self._model().num_frames))
        if longest > most:
            raise ValueError(f"a canvas of {longest} frames: {what} takes at most {most} frames")
        if kw.get("edit_joints") is not None or kw.get("edit_bvh") is not None or kw.get("control_joints") is not None or \
                kw.get("scene") is not None or kw.get("scene_tracks") is not None or kw.get("terrain") is not None:
            kw = dict(kw, mean=mean, std=std)
        return self.generate_long(scripts, dim_pose, **kw)

    @torch.no_grad()
    def generate_long_joints(self, scripts, dim_pose, mean, std, *, joints_num=22, sigma=1.0, from_rotations=False,
                             offsets=None, fix_feet=False, feet_blend=5, pin_targets=False, pin_blend=5, **kw):
        """``generate_long`` followed by ``postprocess.motion_to_joints`` over each whole canvas (one continuous root
        path): a list of ``(canvas_len, joints_num, 3)`` joint positions.  The post-processing kernel holds a canvas in
        LDS: at most MAX_JOINTS_FRAMES frames.  ``edit_joints`` / ``edit_mask`` (through ``**kw``): continue joint clips, as
        in ``generate_long``, under this call's ``mean`` / ``std``.  ``from_rotations`` / ``offsets``: forward kinematics,
        as in ``generate_joints`` (at most ``postprocess.fk_max_frames()`` frames).  ``fix_feet`` / ``feet_blend``:
        foot-skate clean-up over each whole canvas, as ``fix_feet`` / ``blend`` of ``generate_joints`` (``blend`` is
        ``generate_long``'s here): a contact that spans an overlap is one run.  ``pin_targets`` / ``pin_blend``: exact reach
         over each whole canvas on the call's canvas ``control_joints`` / ``control_weights``, one pair per motion."""
        pin = MO.pin_of(pin_targets, kw)
        motions = self._long_motions(scripts, dim_pose, mean, std, MO.canvas_frame_limit(from_rotations), "joint recovery", kw)
        return MO.to_joints(motions, MO.valid_lengths(motions), dim_pose, mean, std, joints_num, sigma, from_rotations, offsets,
                            fix_feet=fix_feet, blend=feet_blend, **MO.pin_kw(pin, pin_blend))

    @torch.no_grad()
    def generate_long_bvh(self, scripts, dim_pose, mean, std, *, paths=None, fps=None, fps_out=None, euler="ZXY", scale=1.0,
                          offsets=None, fix_feet=False, feet_blend=5, target_rig=None, target_joint_map=None, target_up="Y",
                          leg_ik=None, pin_targets=False, pin_blend=5, **kw):
        """``generate_long`` followed by forward kinematics over each whole canvas and the rig export, as ``generate_bvh``:
        one BVH text per motion (at most ``postprocess.fk_max_frames()`` canvas frames).  ``feet_blend`` is ``generate_bvh``'s
        ``blend`` (``blend`` is ``generate_long``'s here); ``target_rig`` / ``target_joint_map`` / ``target_up`` / ``leg_ik`` as
        in ``generate_bvh``; ``pin_targets`` / ``pin_blend`` as in ``generate_long_joints``; ``**kw`` as for ``generate_long``."""
        MO.check_paths(paths, len(scripts), "motion")
        pin = MO.pin_of(pin_targets, kw)
        motions = self._long_motions(scripts, dim_pose, mean, std, MO.canvas_frame_limit(True), "forward kinematics", kw)
        return MO.to_bvh(motions, MO.valid_lengths(motions), dim_pose, mean, std, offsets, fix_feet, feet_blend, paths, fps,
                         fps_out, euler, scale, target_rig, target_joint_map, target_up, leg_ik, **MO.pin_kw(pin, pin_blend))

    @torch.no_grad()
    def generate_mesh(self, caption, m_lens, dim_pose, mean, std, batch_size=8, *, mesh=None, normals=False, offsets=None,
                      fix_feet=False, blend=5, pin_targets=False, pin_blend=5, **kw):
        """``generate`` followed by forward kinematics and linear blend skinning on the device (``motion_mesh``, DESIGN.md
        §30): per sample ``(vertices (m, V, 3), faces (F, 3))``, with ``normals`` ``(vertices, normals (m, V, 3), faces)``;
        ``faces`` is one tensor that all samples share.  ``mesh``: a ``motion_mesh.Mesh`` (``from_dense_weights`` for a
        user's own); None: ``motion_mesh.capsule_body`` of the offsets used, one body per sample.  ``offsets`` / ``fix_feet`` /
        ``blend`` / ``pin_targets`` / ``pin_blend`` as in ``generate_rotations``: the vertices follow the same joints and
        rotations; ``**kw`` as for ``generate``."""
        pin = MO.pin_of(pin_targets, kw)
        motions = self.generate(caption, m_lens, dim_pose, batch_size, mean=mean, std=std, **kw)  # unused without an edit or control
        return MO.to_meshes(motions, MO.valid_lengths(motions, m_lens), dim_pose, mean, std, offsets, fix_feet, blend, mesh,
                            normals, **MO.pin_kw(pin, pin_blend))

    @torch.no_grad()
    def generate_glb(self, caption, m_lens, dim_pose, mean, std, batch_size=8, *, paths=None, fps=None, fps_out=None,
                     scale=1.0, mesh=None, offsets=None, fix_feet=False, blend=5, pin_targets=False, pin_blend=5, **kw):
        """``generate`` followed by forward kinematics, the rig's local quaternions and ``motion_mesh.glb_bytes`` (DESIGN.md
        §30): one glTF 2.0 binary (``bytes``) per sample -- the mesh, its skin on the node tree of ``motion_rig.rig_of`` and
        the animation -- written to ``paths[i]`` where given.  ``fps`` / ``fps_out`` / ``scale`` as in ``generate_bvh``;
        ``mesh`` and the rest as in ``generate_mesh``."""
        MO.check_paths(paths, len(caption), "caption")
        pin = MO.pin_of(pin_targets, kw)
        motions = self.generate(caption, m_lens, dim_pose, batch_size, mean=mean, std=std, **kw)  # unused without an edit or control
        return MO.to_glb(motions, MO.valid_lengths(motions, m_lens), dim_pose, mean, std, offsets, fix_feet, blend, paths, fps,
                         fps_out, scale, mesh, **MO.pin_kw(pin, pin_blend))

    @torch.no_grad()
    def generate_long_mesh(self, scripts, dim_pose, mean, std, *, mesh=None, normals=False, offsets=None, fix_feet=False,
                           feet_blend=5, pin_targets=False, pin_blend=5, **kw):
        """``generate_long`` followed by forward kinematics over each whole canvas and the skinning, as ``generate_mesh``: per
        motion ``(vertices (canvas_len, V, 3)[, normals], faces)`` (at most ``postprocess.fk_max_frames()`` canvas frames).
        ``feet_blend`` is ``generate_mesh``'s ``blend`` (``blend`` is ``generate_long``'s here); ``pin_targets`` / ``pin_blend`` as
        in ``generate_long_joints``; ``**kw`` as for ``generate_long``."""
        pin = MO.pin_of(pin_targets, kw)
        motions = self._long_motions(scripts, dim_pose, mean, std, MO.canvas_frame_limit(True), "forward kinematics", kw)
        return MO.to_meshes(motions, MO.valid_lengths(motions), dim_pose, mean, std, offsets, fix_feet, feet_blend, mesh, normals,
                            **MO.pin_kw(pin, pin_blend))

    @torch.no_grad()
    def generate_long_glb(self, scripts, dim_pose, mean, std, *, paths=None, fps=None, fps_out=None, scale=1.0, mesh=None,
                          offsets=None, fix_feet=False, feet_blend=5, pin_targets=False, pin_blend=5, **kw):
        """``generate_long`` followed by forward kinematics over each whole canvas and the glTF export, as ``generate_glb``:
        one binary per motion (at most ``postprocess.fk_max_frames()`` canvas frames).  ``feet_blend`` is ``generate_glb``'s
        ``blend`` (``blend`` is ``generate_long``'s here); ``pin_targets`` / ``pin_blend`` as in ``generate_long_joints``;
        ``**kw`` as for ``generate_long``."""
        MO.check_paths(paths, len(scripts), "motion")
        pin = MO.pin_of(pin_targets, kw)
        motions = self._long_motions(scripts, dim_pose, mean, std, MO.canvas_frame_limit(True), "forward kinematics", kw)
        return MO.to_glb(motions, MO.valid_lengths(motions), dim_pose, mean, std, offsets, fix_feet, feet_blend, paths, fps,
                         fps_out, scale, mesh, **MO.pin_kw(pin, pin_blend))

    def _body_frames(self, motions, lens, dim_pose, mean, std, size, camera, palette, style, mesh, body):
        """The body view of generated rows, ``body`` holding ``generate_mesh``'s output arguments."""
        return MO.to_body_frames(motions, lens, dim_pose, mean, std, body["offsets"], body["fix_feet"], body["blend"], mesh, size,
                                 camera, palette, style, **MO.pin_kw(body["pin"], body["pin_blend"]))

    @staticmethod
    def _body_args(view, mesh, kw, blend_name="blend"):
        """``view`` / ``mesh`` of the preview methods: None for the joint views (``mesh`` must then be None), else the output
        arguments of ``generate_mesh`` taken out of ``kw``; any view but "root", "world" and "body" is a ValueError."""
        if view != "body":
            if view not in ("root", "world"):
                raise ValueError(f"view must be \"root\", \"world\" or \"body\", not {view!r}")
            if mesh is not None:
                raise ValueError("mesh= belongs to view=\"body\"")
            return None
        pin = MO.pin_of(kw.pop("pin_targets", False), kw)
        return dict(pin=pin, offsets=kw.pop("offsets", None), fix_feet=kw.pop("fix_feet", False),
                    blend=kw.pop(blend_name, 5), pin_blend=kw.pop("pin_blend", 5))

    @torch.no_grad()
    def generate_frames(self, caption, m_lens, dim_pose, mean, std, batch_size=8, *, size=(480, 480), camera=None,
                        palette=False, style=None, view="root", mesh=None, **kw):
        """``generate_joints`` followed by the motion preview (``motion_render.render_motion``) on the device:
        a list of ``(m_len, H, W, 3)`` uint8 frames, ``size`` = (H, W); with ``palette`` ``(m_len, H, W)`` indices into
        ``motion_render.PALETTE``.  ``camera``: a ``motion_render.Camera`` or a dict of its fields; ``style``: a dict of
        ``render_motion``'s colour and width arguments.  ``**kw`` goes to ``generate_joints`` untouched: ``from_rotations``,
        ``fix_feet``, ``pin_targets``, the sampler, edit and control arguments.  ``view="world"``: the world view instead
        (``motion_render.render_world``): each character in world coordinates with the ``scene`` /
        ``scene_tracks`` that steered it; ``camera`` None then fits one camera to the batch, ``style`` is ``render_world``'s.
        ``view="body"``: the body view (``motion_render.render_mesh``) of the skinned mesh that ``generate_mesh``
        returns for the same arguments (forward kinematics of the rotations, no temporal filter, ``offsets`` / ``fix_feet`` /
        ``blend`` / ``pin_targets`` / ``pin_blend`` as there, ``**kw`` as for ``generate``): ``mesh`` a ``motion_mesh.Mesh``, None
        ``motion_mesh.capsule_body`` of the offsets used; ``style`` is ``render_mesh``'s."""
        body = self._body_args(view, mesh, kw)
        if body is not None:
            motions = self.generate(caption, m_lens, dim_pose, batch_size, mean=mean, std=std, **kw)
            return self._body_frames(motions, MO.valid_lengths(motions, m_lens), dim_pose, mean, std, size, camera, palette, style,
                                     mesh, body)
        joints = self.generate_joints(caption, m_lens, dim_pose, mean, std, batch_size, **kw)
        return MO.to_frames_view(view, joints, kw, size, camera, palette, style)

    @torch.no_grad()
    def generate_gif(self, caption, m_lens, dim_pose, mean, std, batch_size=8, *, paths=None, fps=None, size=(480, 480),
                     camera=None, style=None, view="root", mesh=None, **kw):
        """``generate_frames`` in palette mode followed by ``motion_render.write_gif``: one animated GIF per caption, as
        bytes, or written to ``paths[i]`` where given (the path is then returned in its place).  ``fps`` defaults to
        ``motion_rig.DEFAULT_FPS`` (20 at dim_pose 263, 12.5 at 251); a GIF's frame delay is whole centiseconds.  ``view`` /
        ``mesh`` as in ``generate_frames``."""
        MO.check_paths(paths, len(caption), "caption")
        frames = self.generate_frames(caption, m_lens, dim_pose, mean, std, batch_size, size=size, camera=camera, palette=True,
                                      style=style, view=view, mesh=mesh, **kw)
        return MO.to_gifs(frames, dim_pose, paths, fps)

    @torch.no_grad()
    def generate_long_gif(self, scripts, dim_pose, mean, std, *, paths=None, fps=None, size=(480, 480), camera=None,
                          style=None, view="root", mesh=None, **kw):
        """``generate_long_joints`` followed by the motion preview and ``write_gif``, as ``generate_gif``: one GIF per long
        motion.  ``**kw`` goes to ``generate_long_joints`` untouched.  ``view="world"``: the world view with each motion's
        ``scene`` and its canvas ``scene_tracks`` (targets are not drawn).  ``view="body"`` / ``mesh``: the body view of the
        skinned mesh that ``generate_long_mesh`` returns for the same arguments (``feet_blend`` is its ``blend``)."""
        MO.check_paths(paths, len(scripts), "motion")
        body = self._body_args(view, mesh, kw, "feet_blend")
        if body is not None:
            motions = self._long_motions(scripts, dim_pose, mean, std, MO.canvas_frame_limit(True), "forward kinematics", kw)
            frames = self._body_frames(motions, MO.valid_lengths(motions), dim_pose, mean, std, size, camera, True, style, mesh, body)
            return MO.to_gifs(frames, dim_pose, paths, fps)
        joints = self.generate_long_joints(scripts, dim_pose, mean, std, **kw)
        return MO.to_gifs(MO.to_frames_view(view, joints, kw, size, camera, True, style), dim_pose, paths, fps)

    @torch.no_grad()
    def generate_together_frames(self, scenes, dim_pose, mean, std, *, size=(480, 480), camera=None, palette=False, style=None,
                                 **kw):
        """``generate_together`` followed by the world view (``motion_render.render_world``): per scene
        ``(n, H, W, 3)`` uint8 frames (``(n, H, W)`` palette indices with ``palette``), n the length of its longest character,
        showing every character of the scene and the union of the characters' ``scene`` primitives (already in world
        coordinates).  ``camera`` None: one camera fitted to all scenes of the call; ``style``: a dict of ``render_world``'s
        style arguments.  ``**kw`` goes to ``generate_together``, ``mutual=`` and ``contacts=`` included."""
        worlds = self.generate_together(scenes, dim_pose, mean, std, **kw)
        return MO.to_world_frames(worlds, [MO.world_scene(s) for s in scenes], None, size, camera, palette, style)

    @torch.no_grad()
    def generate_together_gif(self, scenes, dim_pose, mean, std, *, paths=None, fps=None, size=(480, 480), camera=None,
                              style=None, **kw):
        """``generate_together_frames`` in palette mode followed by ``motion_render.write_gif``, as ``generate_gif``: one GIF
        per scene, the length of its longest character."""
        MO.check_paths(paths, len(scenes), "scene")
        frames = self.generate_together_frames(scenes, dim_pose, mean, std, size=size, camera=camera, palette=True, style=style,
                                               **kw)
        return MO.to_gifs(frames, dim_pose, paths, fps)

    def save(self, file_name, ep, total_it):
        state = {"opt_encoder": getattr(self, "opt_encoder_state", {}), "ep": ep, "total_it": total_it,
                 "encoder": self._model().state_dict()}
        torch.save(state, file_name)

    def load(self, model_dir):
        ckpt = torch.load(model_dir, map_location=self.device)
        self._model().load_state_dict(ckpt["encoder"], strict=False)
        return ckpt["ep"], ckpt.get("total_it", 0)

    def train(self, *a, **k):
        raise NotImplementedError("whole-model training is outside this build's scope (SURVEY.md section 8(f)): DDPMTrainer "
                                  "provides the sampling API; the training step of the MoE feed-forward block is "
                                  "moe_train.MoEFFNTrainer")

    forward = backward_G = update = train

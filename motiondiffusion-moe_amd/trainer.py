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
conditioning once (``conditioning.Conditioning``) and samples each batch's rows through ``_sample_rows``.  The training loop (forward/backward/update/train) is out of scope for
this build and raises.
"""
from __future__ import annotations

import torch

from . import motion_long as ML
from .conditioning import (Conditioning, LatentStep, check_joint_edit_mask, edit_rows_from_joints, expand_to,
                           joint_clips_from_bvh, pad_frames, strength_steps)
from .diffusion import (GaussianDiffusion, LossType, ModelMeanType, ModelVarType, SpacedDiffusion, get_named_beta_schedule,
                        space_timesteps)

SAMPLERS = ("ddpm", "ddim", "dpmpp2m")
MAX_JOINTS_FRAMES = 3276  # frames of mdm_motion_postprocess: 5 T floats of LDS per workgroup, 64 KiB


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
                       sample_offset=0, sampler="ddpm", sample_steps=None, eta=0.0, edit_motion=None, edit_mask=None,
                       prompt_weights=None, control_joints=None, control_weights=None, control_scale=1.0,
                       control_iters=1, mean=None, std=None, edit_joints=None, edit_bvh=None, bvh_options=None,
                       init_motion=None, init_joints=None, init_bvh=None, strength=None, latents=None, latent_step=None):
        """``edit_motion`` (B, T_max, dim_pose), normalised, and ``edit_mask`` broadcastable to it, values in [0, 1]: the
        batch's first T frames of both are kept where the mask is 1 (exactly, for a binary mask) and generated elsewhere.
        ``prompt_weights`` (B, K, ...) broadcastable to (B, K, T_max, dim_pose): ``caption[i]`` is then a sequence of K
        captions, composed on every step under these weights.
        ``control_joints`` (B, T_max, J, 3) target joint positions and ``control_weights`` (B, ...) broadcastable to them, with
        the dataset's ``mean`` / ``std`` (dim_pose,): every step's x0 is moved ``control_iters`` times down the gradient of
        the weighted squared distance, scaled by ``control_scale`` (units in ``motion_control``).
        ``edit_joints``: B joint clips (n_i, J, 3) in place of ``edit_motion`` (needs ``mean`` / ``std``), turned into
        feature rows once per call (``motion_features.joints_to_motion``); a clip of n frames gives n - 1
        rows, so the mask may keep frames up to n - 2.  ``edit_bvh``: B BVH texts, paths or parsed files in place of
        ``edit_joints``, read at the model's frame rate by ``motion_rig.bvh_to_joints`` under
        ``bvh_options`` (a dict of its ``joint_map`` / ``scale`` / ``up`` / ``basis`` / ``fps_out``) and from there on
        treated as ``edit_joints``; exclusive with ``edit_joints`` and ``edit_motion``.
        ``init_motion`` (B, T_max, dim_pose), normalised, with ``strength`` in [0, 1]: motion-to-motion.
        The motion is noised to an intermediate level of the chosen sampler's schedule and ``round(strength * steps)``
        steps run from there under the caption: 1 is the plain call (the motion is ignored), 0 returns the motion, values
        in between stay the closer to it the smaller they are.  ``init_joints`` (B joint clips, needs ``mean`` / ``std``) or
        ``init_bvh`` (B files, read under ``bvh_options``) in place of ``init_motion``, converted as ``edit_joints`` /
        ``edit_bvh`` are; a clip must cover its sample's length.  It composes with the edit, prompt and control inputs,
        which act on every step that runs.  ``latents`` (B, T, dim_pose) with ``latent_step``: x at that step of this
        call's schedule, as ``invert`` returns them, to continue from; needs ``sampler="ddim"`` and the ``sample_steps``
        of the inversion."""
        cond = Conditioning(caption, dim_pose, edit_motion, edit_mask, prompt_weights, control_joints, control_weights,
                            control_scale, control_iters, mean, std, edit_joints, self.device, edit_bvh=edit_bvh,
                            bvh_options=bvh_options, init_motion=init_motion, init_joints=init_joints, init_bvh=init_bvh,
                            strength=strength, latents=latents, latent_step=latent_step)
        m_lens = torch.as_tensor(m_lens)
        T = min(int(m_lens.max()), self._model().num_frames)
        return self._sample_rows(cond, slice(0, len(caption)), m_lens, T, sampler, sample_steps, eta, progress=progress,
                                 noise=noise, step_noise=step_noise, seed=seed, sample_offset=sample_offset)

    @torch.no_grad()
    def generate(self, caption, m_lens, dim_pose, batch_size=8, *, progress=False, seed=None, noises=None, sampler="ddpm",
                 sample_steps=None, eta=0.0, edit_motion=None, edit_mask=None, prompt_weights=None, control_joints=None,
                 control_weights=None, control_scale=1.0, control_iters=1, mean=None, std=None, edit_joints=None,
                 edit_bvh=None, bvh_options=None, init_motion=None, init_joints=None, init_bvh=None, strength=None,
                 latents=None, latent_step=None):
        """``seed``: sample i's noise is then a function of (seed, i) only (counter-based device generator), so the result
        does not depend on ``batch_size``; without it the torch generator is used, as in the reference.
        ``noises``: optional list with one ``(x_T, [step noise, ...])`` pair per batch, replacing the draws (parity tests).
        ``sampler`` / ``sample_steps`` / ``eta``: see ``sampling_diffusion``; e.g. ``sampler="dpmpp2m", sample_steps=20``.
        ``edit_motion`` (N, T_max, dim_pose) and ``edit_mask`` (broadcastable to it): motion editing, see ``generate_batch``;
        each batch takes its samples' rows.  ``prompt_weights`` (N, K, ...): composed prompts, see ``generate_batch``; each
        batch takes its samples' rows.  ``control_joints`` (N, T_max, J, 3), ``control_weights``, ``control_scale``,
        ``control_iters``, ``mean``, ``std``: joint-position control, see ``generate_batch``; each batch takes its samples'
        rows.  ``edit_joints``: N joint clips in place of ``edit_motion``, see ``generate_batch``; ``edit_bvh`` /
        ``bvh_options``: N BVH files in place of those, see ``generate_batch``.  ``init_motion`` (N, T_max, dim_pose) /
        ``init_joints`` / ``init_bvh`` with ``strength``: start from a given motion, see ``generate_batch``; each batch takes
        its samples' rows and its first T frames, and with ``seed`` the noise mixed into sample i is a function of (seed, i).
        ``latents`` (N, T, dim_pose, or a list of (T_i, dim_pose)) with ``latent_step``: continue from ``invert``'s result."""
        N = len(caption)
        self.eval_mode()
        cond = Conditioning(caption, dim_pose, edit_motion, edit_mask, prompt_weights, control_joints, control_weights,
                            control_scale, control_iters, mean, std, edit_joints, self.device, edit_bvh=edit_bvh,
                            bvh_options=bvh_options, init_motion=init_motion, init_joints=init_joints, init_bvh=init_bvh,
                            strength=strength, latents=latents, latent_step=latent_step)
        all_output = []
        for cur in range(0, N, batch_size):
            end = min(cur + batch_size, N)
            x_T, step_noise = noises[cur // batch_size] if noises is not None else (None, None)
            lens = torch.as_tensor(m_lens[cur:end])
            T = min(int(lens.max()), self._model().num_frames)
            out = self._sample_rows(cond, slice(cur, end), lens, T, sampler, sample_steps, eta, progress=progress,
                                    noise=x_T, step_noise=step_noise, seed=seed, sample_offset=cur)
            all_output.extend(out[i] for i in range(out.shape[0]))
        return all_output

    @torch.no_grad()
    def generate_bucketed(self, caption, m_lens, dim_pose, batch_size=32, *, unit_length=4, seed=None, group=None,
                          progress=False, sampler="ddpm", sample_steps=None, eta=0.0, edit_motion=None, edit_mask=None,
                          prompt_weights=None, control_joints=None, control_weights=None, control_scale=1.0,
                          control_iters=1, mean=None, std=None, edit_joints=None, edit_bvh=None, bvh_options=None,
                          init_motion=None, init_joints=None, init_bvh=None, strength=None):
        """Evaluation-scale variant of ``generate``: same inputs and the same kind of result (a
        list of per-sample ``(T_batch, dim_pose)`` tensors in the caller's order, valid up to each sample's length),
        but batches hold samples of similar length (less padded work) and, under ``torch.distributed``, are dealt over
        the ranks with one all_gather at the end.  With ``seed`` every sample's noise is a function of (seed, its index in
        ``caption``) only -- the same as ``generate(..., seed=)`` -- so on each sample's valid frames the two give identical
        results whatever the bucketing (tests/test_sampler_gpu.py).  ``edit_motion`` / ``edit_mask``: as in ``generate``;
        each bucket takes its samples' rows and its first T frames; so do ``prompt_weights`` and the ``control_*`` tensors.
        ``edit_joints``: joint clips in place of ``edit_motion``, as in ``generate``; so are ``edit_bvh`` / ``bvh_options``.
        ``init_motion`` / ``init_joints`` / ``init_bvh`` with ``strength``: as in ``generate``, each bucket taking its
        samples' rows and its first T frames."""
        from . import dist as D
        m = self._model()
        self.eval_mode()
        cond = Conditioning(caption, dim_pose, edit_motion, edit_mask, prompt_weights, control_joints, control_weights,
                            control_scale, control_iters, mean, std, edit_joints, self.device, edit_bvh=edit_bvh,
                            bvh_options=bvh_options, init_motion=init_motion, init_joints=init_joints, init_bvh=init_bvh,
                            strength=strength)
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
            all_len = [min(n, mo.shape[0]) for mo, n in zip(gen, all_len)]
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
        from .motion_features import refeaturize
        lens = [min(int(n), mo.shape[0]) for n, mo in zip(torch.as_tensor(m_lens).flatten().tolist(), motions)]
        dim_pose = motions[0].shape[-1]
        x = torch.zeros((len(motions), max(lens), dim_pose), device=motions[0].device)
        for i, (mo, n) in enumerate(zip(motions, lens)):
            x[i, :n] = mo[:n]
        rows = refeaturize(x, mean, std, torch.tensor(lens), skeleton={263: "t2m", 251: "kit"}[dim_pose])
        return [rows[i, :n - 1] for i, n in enumerate(lens)]

    @torch.no_grad()
    def generate_joints(self, caption, m_lens, dim_pose, mean, std, batch_size=8, *, joints_num=22, sigma=1.0,
                        bucketed=False, sampler="ddpm", sample_steps=None, eta=0.0, edit_motion=None, edit_mask=None,
                        prompt_weights=None, control_joints=None, control_weights=None, control_scale=1.0,
                        control_iters=1, from_rotations=False, offsets=None, fix_feet=False, blend=5, **kw):
        """``generate`` followed by the reference's post-processing (tools/visualization.py:21-27,89) on the device:
        list of ``(m_len, joints_num, 3)`` joint positions, temporally smoothed with a gaussian of width ``sigma``.
        ``edit_motion`` / ``edit_mask``: motion editing in normalised feature space, as in ``generate``;
        ``prompt_weights``: composed prompts, as in ``generate``; ``control_joints`` / ``control_weights`` /
        ``control_scale`` / ``control_iters``: joint-position control under this call's ``mean`` / ``std``;
        ``edit_joints`` (through ``**kw``): joint clips in place of ``edit_motion``, converted under the same ``mean`` /
        ``std``.  ``from_rotations``: joints by forward kinematics of the rot6d columns (``postprocess.motion_to_joints_fk``,
        DESIGN.md §17: rigid bones) on ``offsets`` (J, 3) or one (J, 3) per motion; None: every motion's own mean bone
        lengths.  ``fix_feet``: foot-skate clean-up after the temporal filter (``postprocess.remove_foot_skate``, DESIGN.md
        §18), the labels being the generated rows' own foot-contact columns; ``blend`` frames of fade either side of a contact."""
        gen = self.generate_bucketed if bucketed else self.generate  # mean / std go along: unused without control
        motions = gen(caption, m_lens, dim_pose, batch_size, sampler=sampler, sample_steps=sample_steps, eta=eta,
                      edit_motion=edit_motion, edit_mask=edit_mask, prompt_weights=prompt_weights,
                      control_joints=control_joints, control_weights=control_weights, control_scale=control_scale,
                      control_iters=control_iters, mean=mean, std=std, **kw)
        lens = [min(int(n), mo.shape[0]) for n, mo in zip(torch.as_tensor(m_lens).flatten().tolist(), motions)]
        return self._to_joints(motions, lens, dim_pose, mean, std, joints_num, sigma, from_rotations, offsets,
                               fix_feet=fix_feet, blend=blend)

    @staticmethod
    def _to_joints(motions, lens, dim_pose, mean, std, joints_num, sigma, from_rotations=False, offsets=None,
                   return_rotations=False, fix_feet=False, blend=5):
        """``postprocess.motion_to_joints`` over the first ``lens[i]`` frames of every motion, or with ``from_rotations``
        ``postprocess.motion_to_joints_fk``: one launch for all.  ``return_rotations`` (forward kinematics only): a list of
        (joints, rotations, offsets) per motion.  ``fix_feet``: ``postprocess.remove_foot_skate`` on the result, filtered
        first (filtering afterwards would smear the pins), labels from the rows' contact columns read in place; rotations go
        through it, so that joints and rotations still agree."""
        from .postprocess import motion_to_joints, motion_to_joints_fk, remove_foot_skate
        skel = {263: "t2m", 251: "kit"}.get(dim_pose)
        if fix_feet and (skel is None or dim_pose != 12 * joints_num - 1):
            raise ValueError(f"fix_feet needs dim_pose 263 (22 joints) or 251 (21), not {dim_pose} ({joints_num})")
        if (offsets is not None or return_rotations) and not from_rotations:
            raise ValueError("offsets and rotations belong to forward kinematics: pass from_rotations=True")
        x = torch.zeros((len(motions), max(mo.shape[0] for mo in motions), dim_pose), device=motions[0].device)
        for i, mo in enumerate(motions):
            x[i, :mo.shape[0]] = mo
        if not from_rotations:
            j = motion_to_joints(x, mean, std, torch.tensor(lens), joints_num, sigma)
            if fix_feet:
                j = remove_foot_skate(j, torch.tensor(lens), (x, mean, std), skeleton=skel, blend=blend)
            return [j[i, :n] for i, n in enumerate(lens)]
        if dim_pose != 12 * joints_num - 1 or dim_pose not in (263, 251):
            raise ValueError(f"forward kinematics needs dim_pose 263 (22 joints) or 251 (21), not {dim_pose} ({joints_num})")
        if isinstance(offsets, (list, tuple)):
            offsets = torch.stack([torch.as_tensor(o).to("cpu", torch.float32) for o in offsets])
        j, r, o = motion_to_joints_fk(x, mean, std, torch.tensor(lens), offsets, skeleton=skel, sigma=sigma,
                                      return_rotations=True, return_offsets=True)
        if fix_feet:
            j, r = remove_foot_skate(j, torch.tensor(lens), (x, mean, std), skeleton=skel, blend=blend, rotations=r)
        if return_rotations:
            return [(j[i, :n], r[i, :n], o[i]) for i, n in enumerate(lens)]
        return [j[i, :n] for i, n in enumerate(lens)]

    @torch.no_grad()
    def generate_rotations(self, caption, m_lens, dim_pose, mean, std, batch_size=8, *, offsets=None, fix_feet=False,
                           blend=5, **kw):
        """``generate`` followed by forward kinematics (``postprocess.motion_to_joints_fk``): per sample
        ``(joints (m, J, 3), rotations (m, J, 3, 3), offsets (J, 3))``: the joints on rigid bones, unfiltered so that they
        agree with the rotations, the global rotation matrix of every joint (the root's at joint 0) and the bone offsets
        used (``offsets``, or the sample's own mean bone lengths).  ``fix_feet`` / ``blend``: foot-skate clean-up as in
        ``generate_joints``; the rotations of knees, ankles and toes turn with their bones.  ``**kw`` as for ``generate``."""
        motions = self.generate(caption, m_lens, dim_pose, batch_size, mean=mean, std=std, **kw)  # unused without an edit or control
        lens = [min(int(n), mo.shape[0]) for n, mo in zip(torch.as_tensor(m_lens).flatten().tolist(), motions)]
        return self._to_joints(motions, lens, dim_pose, mean, std, (dim_pose + 1) // 12, 0.0, True, offsets, True,
                               fix_feet=fix_feet, blend=blend)

    @staticmethod
    def _to_bvh(motions, lens, dim_pose, mean, std, offsets, fix_feet, blend, paths, fps, fps_out, euler, scale):
        """Rows -> one BVH text per motion: ``_to_joints`` with rotations and no filter, one
        ``motion_rig.rotations_to_rig`` over the padded batch, ``motion_rig.bvh_text`` per sample."""
        from .motion_rig import bvh_text, retime_ratio, rig_of, rotations_to_rig
        res = DDPMTrainer._to_joints(motions, lens, dim_pose, mean, std, (dim_pose + 1) // 12, 0.0, True, offsets, True,
                                     fix_feet=fix_feet, blend=blend)
        skel = {263: "t2m", 251: "kit"}[dim_pose]
        rig = rig_of(skel)
        j = torch.zeros((len(res), max(lens)) + tuple(res[0][0].shape[1:]), device=res[0][0].device)
        r = torch.zeros(tuple(j.shape[:3]) + (3, 3), device=j.device)
        for i, (ji, ri, _) in enumerate(res):
            j[i, :lens[i]], r[i, :lens[i]] = ji, ri
        chan, lens_out = rotations_to_rig(j, r, torch.tensor(lens), skeleton=skel, euler=euler, fps=fps, fps_out=fps_out,
                                          scale=scale)
        num, den, fps = retime_ratio(skel, fps, fps_out)
        frame_time = den / (num * float(fps))
        chan, texts = chan.cpu(), []
        for i, (_, _, o) in enumerate(res):
            texts.append(bvh_text(rig, o, chan[i], int(lens_out[i]), frame_time, euler=euler, scale=scale))
            if paths is not None and paths[i] is not None:
                with open(paths[i], "w") as f:
                    f.write(texts[-1])
        return texts

    @torch.no_grad()
    def generate_bvh(self, caption, m_lens, dim_pose, mean, std, batch_size=8, *, paths=None, fps=None, fps_out=None,
                     euler="ZXY", scale=1.0, offsets=None, fix_feet=False, blend=5, **kw):
        """``generate`` followed by forward kinematics and the rig export (``motion_rig``): one BVH text per
        sample, written to ``paths[i]`` where given.  ``fps`` (default 20 at dim_pose 263, 12.5 at 251) / ``fps_out``: retimed
        to the frame rate a tool works at; ``euler``: the channels' rotation order; ``scale``: of positions and offsets (100
        for centimetres).  ``offsets`` / ``fix_feet`` / ``blend`` as in ``generate_rotations``, ``**kw`` as for ``generate``:
        with ``edit_bvh=`` / ``edit_mask=`` a file from a rig is continued and written back as one (converted under this
        call's ``mean`` / ``std``)."""
        if paths is not None and len(paths) != len(caption):
            raise ValueError(f"paths must hold one entry per caption ({len(caption)}), or None")
        motions = self.generate(caption, m_lens, dim_pose, batch_size, mean=mean, std=std, **kw)  # unused without an edit or control
        lens = [min(int(n), mo.shape[0]) for n, mo in zip(torch.as_tensor(m_lens).flatten().tolist(), motions)]
        return self._to_bvh(motions, lens, dim_pose, mean, std, offsets, fix_feet, blend, paths, fps, fps_out, euler, scale)

    @torch.no_grad()
    def generate_long(self, scripts, dim_pose, *, overlap=20, blend="linear", batch_size=32, seed=None, sampler="ddpm",
                      sample_steps=None, eta=0.0, edit_motion=None, edit_mask=None, noise=None, progress=False,
                      edit_joints=None, mean=None, std=None, edit_bvh=None, bvh_options=None, init_motion=None,
                      strength=None):
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
        window's noised values."""
        m = self._model()
        self.eval_mode()
        plans = ML.script_plans(scripts, overlap, m.num_frames)
        N = len(plans)
        if edit_bvh is not None or bvh_options is not None:
            edit_joints = joint_clips_from_bvh(edit_bvh, bvh_options, edit_joints, edit_motion, self.device)
        if edit_joints is not None:
            if edit_motion is not None:
                raise ValueError("edit_joints and edit_motion are exclusive: the known motion is given as joints or as rows")
            if edit_mask is None or len(edit_joints) != N or len(edit_mask) != N or any(mk is None for mk in edit_mask):
                raise ValueError(f"edit_joints needs one clip and one edit_mask per motion ({N})")
            rows, nrows = edit_rows_from_joints(edit_joints, mean, std, dim_pose, self.device)
            edit_motion = []
            for i, n in enumerate(nrows):
                if n > plans[i][3]:
                    raise ValueError(f"motion {i}: a clip of {n} rows does not fit its canvas of {plans[i][3]} frames")
                edit_motion.append(pad_frames(rows[i:i + 1, :n], plans[i][3])[0])
                check_joint_edit_mask(expand_to(edit_mask[i], None, edit_motion[i].shape, "edit_mask")[None], [n])
        per = {}
        if (init_motion is None) != (strength is None):
            raise ValueError("init_motion and strength go together: give both or neither")
        for name, v in (("edit_motion", edit_motion), ("edit_mask", edit_mask), ("noise", noise), ("init_motion", init_motion)):
            if v is not None and len(v) != N:
                raise ValueError(f"{name} must hold one entry per motion ({N}), not {len(v)}")
            per[name] = [None] * N if v is None else list(v)
        if (edit_motion is None) != (edit_mask is None):
            raise ValueError("edit_motion and edit_mask go together: give both or neither")
        for i, (km, mk) in enumerate(zip(per["edit_motion"], per["edit_mask"])):
            if (km is None) != (mk is None):
                raise ValueError(f"motion {i}: edit_motion and edit_mask go together")
        for name in ("edit_motion", "noise", "init_motion"):
            if any(x is not None for x in per[name]) and not all(x is not None for x in per[name]):
                raise ValueError(f"{name} must be given for every motion of the call or for none")
        out, first = [None] * N, 0
        for idx in ML.plan_batches(plans, batch_size):
            caps = [c for i in idx for c in plans[i][0]]
            lens = [n for i in idx for n in plans[i][1]]
            T = max(lens) + max(lens) % 2  # the denoiser takes even T
            kw = ML.batch_tables(plans, idx, T, overlap, blend)
            rows = {}  # the per-motion canvases given, as window rows
            for name in ("edit_motion", "edit_mask", "noise", "init_motion"):
                if per[name][idx[0]] is None:
                    continue
                for i in idx:
                    if name != "edit_mask" and tuple(torch.as_tensor(per[name][i]).shape) != (plans[i][3], dim_pose):
                        raise ValueError(f"{name} of motion {i} must be {(plans[i][3], dim_pose)}")
                rows[name] = ML.gather_canvases(per[name], plans, idx, T, dim_pose, name).to(self.device)
            if "edit_motion" in rows:
                kw.update(inpaint_motion=rows["edit_motion"], inpaint_mask=rows["edit_mask"])
            cond = Conditioning(caps, dim_pose, init_motion=rows.get("init_motion"), strength=strength)
            res = self._sample_rows(cond, slice(None), torch.tensor(lens), T, sampler, sample_steps, eta, extra=kw,
                                    progress=progress, noise=rows.get("noise"), seed=seed, sample_offset=first)
            first += len(caps)
            row = 0
            for i in idx:
                n = len(plans[i][1])
                out[i] = ML.windows_to_canvas(res[row:row + n], plans[i][2], plans[i][1])
                row += n
        return out

    @torch.no_grad()
    def generate_long_joints(self, scripts, dim_pose, mean, std, *, joints_num=22, sigma=1.0, from_rotations=False,
                             offsets=None, fix_feet=False, feet_blend=5, **kw):
        """``generate_long`` followed by ``postprocess.motion_to_joints`` over each whole canvas (one continuous root
        path): a list of ``(canvas_len, joints_num, 3)`` joint positions.  The post-processing kernel holds a canvas in
        LDS: at most MAX_JOINTS_FRAMES frames.  ``edit_joints`` / ``edit_mask`` (through ``**kw``): continue joint clips, as
        in ``generate_long``, under this call's ``mean`` / ``std``.  ``from_rotations`` / ``offsets``: forward kinematics,
        as in ``generate_joints`` (at most ``postprocess.fk_max_frames()`` frames).  ``fix_feet`` / ``feet_blend``:
        foot-skate clean-up over each whole canvas, as ``fix_feet`` / ``blend`` of ``generate_joints`` (``blend`` is
        ``generate_long``'s here): a contact that spans an overlap is one run."""
        plans = ML.script_plans(scripts, kw.get("overlap", 20), self._model().num_frames)
        longest = max(p[3] for p in plans)
        most = MAX_JOINTS_FRAMES
        if from_rotations:
            from .postprocess import fk_max_frames
            most = fk_max_frames()
        if longest > most:
            raise ValueError(f"a canvas of {longest} frames: joint recovery takes at most {most} frames")
        if kw.get("edit_joints") is not None or kw.get("edit_bvh") is not None:  # converted under the same mean / std
            kw = dict(kw, mean=mean, std=std)
        motions = self.generate_long(scripts, dim_pose, **kw)
        return self._to_joints(motions, [mo.shape[0] for mo in motions], dim_pose, mean, std, joints_num, sigma,
                               from_rotations, offsets, fix_feet=fix_feet, blend=feet_blend)

    @torch.no_grad()
    def generate_long_bvh(self, scripts, dim_pose, mean, std, *, paths=None, fps=None, fps_out=None, euler="ZXY", scale=1.0,
                          offsets=None, fix_feet=False, feet_blend=5, **kw):
        """``generate_long`` followed by forward kinematics over each whole canvas and the rig export, as ``generate_bvh``:
        one BVH text per motion (at most ``postprocess.fk_max_frames()`` canvas frames).  ``feet_blend`` is ``generate_bvh``'s
        ``blend`` (``blend`` is ``generate_long``'s here); ``**kw`` as for ``generate_long``."""
        from .postprocess import fk_max_frames
        if paths is not None and len(paths) != len(scripts):
            raise ValueError(f"paths must hold one entry per motion ({len(scripts)}), or None")
        plans = ML.script_plans(scripts, kw.get("overlap", 20), self._model().num_frames)
        longest = max(p[3] for p in plans)
        if longest > fk_max_frames():
            raise ValueError(f"a canvas of {longest} frames: forward kinematics takes at most {fk_max_frames()} frames")
        if kw.get("edit_joints") is not None or kw.get("edit_bvh") is not None:
            kw = dict(kw, mean=mean, std=std)
        motions = self.generate_long(scripts, dim_pose, **kw)
        return self._to_bvh(motions, [mo.shape[0] for mo in motions], dim_pose, mean, std, offsets, fix_feet, feet_blend, paths,
                            fps, fps_out, euler, scale)

    @staticmethod
    def _to_frames(joints, size, camera, palette, style):
        """``motion_render.render_motion`` over a list of (n_i, J, 3) joint clips, one launch for all: a list of
        ``(n_i, H, W, 3)`` uint8 frames, or ``(n_i, H, W)`` palette indices."""
        from .motion_features import pad_clips
        from .motion_render import render_motion
        x, lens = pad_clips(joints, joints[0].shape[1])
        frames = render_motion(x, lens, size=size, camera=camera, palette=palette, **(style or {}))
        return [frames[i, :n] for i, n in enumerate(lens.tolist())]

    @staticmethod
    def _to_gifs(frames, dim_pose, paths, fps):
        from .motion_render import gif_bytes, write_gif
        from .motion_rig import DEFAULT_FPS
        if fps is None:
            fps = DEFAULT_FPS.get({263: "t2m", 251: "kit"}.get(dim_pose), DEFAULT_FPS["t2m"])
        if paths is None:
            return [gif_bytes(f, fps) for f in frames]
        return [gif_bytes(f, fps) if p is None else write_gif(f, p, fps) for f, p in zip(frames, paths)]

    @torch.no_grad()
    def generate_frames(self, caption, m_lens, dim_pose, mean, std, batch_size=8, *, size=(480, 480), camera=None,
                        palette=False, style=None, **kw):
        """``generate_joints`` followed by the motion preview (``motion_render.render_motion``) on the device:
        a list of ``(m_len, H, W, 3)`` uint8 frames, ``size`` = (H, W); with ``palette`` ``(m_len, H, W)`` indices into
        ``motion_render.PALETTE``.  ``camera``: a ``motion_render.Camera`` or a dict of its fields; ``style``: a dict of
        ``render_motion``'s colour and width arguments.  ``**kw`` goes to ``generate_joints`` untouched: ``from_rotations``,
        ``fix_feet``, the sampler, edit and control arguments."""
        joints = self.generate_joints(caption, m_lens, dim_pose, mean, std, batch_size, **kw)
        return self._to_frames(joints, size, camera, palette, style)

    @torch.no_grad()
    def generate_gif(self, caption, m_lens, dim_pose, mean, std, batch_size=8, *, paths=None, fps=None, size=(480, 480),
                     camera=None, style=None, **kw):
        """``generate_frames`` in palette mode followed by ``motion_render.write_gif``: one animated GIF per caption, as
        bytes, or written to ``paths[i]`` where given (the path is then returned in its place).  ``fps`` defaults to
        ``motion_rig.DEFAULT_FPS`` (20 at dim_pose 263, 12.5 at 251); a GIF's frame delay is whole centiseconds."""
        if paths is not None and len(paths) != len(caption):
            raise ValueError(f"paths must hold one entry per caption ({len(caption)}), or None")
        frames = self.generate_frames(caption, m_lens, dim_pose, mean, std, batch_size, size=size, camera=camera, palette=True,
                                      style=style, **kw)
        return self._to_gifs(frames, dim_pose, paths, fps)

    @torch.no_grad()
    def generate_long_gif(self, scripts, dim_pose, mean, std, *, paths=None, fps=None, size=(480, 480), camera=None,
                          style=None, **kw):
        """``generate_long_joints`` followed by the motion preview and ``write_gif``, as ``generate_gif``: one GIF per long
        motion.  ``**kw`` goes to ``generate_long_joints`` untouched."""
        if paths is not None and len(paths) != len(scripts):
            raise ValueError(f"paths must hold one entry per motion ({len(scripts)}), or None")
        joints = self.generate_long_joints(scripts, dim_pose, mean, std, **kw)
        return self._to_gifs(self._to_frames(joints, size, camera, True, style), dim_pose, paths, fps)

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

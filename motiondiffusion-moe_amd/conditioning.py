"""Host side of every conditioning input of the sampler: what a generate call is given besides captions and lengths.

``expand_to`` is the one align-and-expand of a weight / mask tensor.  ``strength_steps`` and ``init_rows_from`` are the host
side of motion-to-motion generation (a given motion as the start of a partial loop).  The
``check_*_kwargs`` functions validate the ``model_kwargs`` of one sampler batch (motion editing, composed prompts, joint
control, long-motion handshakes, joint control over a long motion's canvas) for
``diffusion._StepRunner``; ``diffusion`` imports them under the same names.  ``Conditioning``
holds the checked conditioning of one public ``DDPMTrainer`` call and hands out each batch's share as ``model_kwargs``.
Host logic only: runs on CPU tensors and never loads the HIP library.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib as L

# runner modes with classifier-free guidance: [cond | uncond] = 2B rows, (K + 1)B with K composed prompts
GUIDED = ("cfg", "cfg_ddim", "cfg_dpmpp")


def expand_to(t, lead, shape, name, lead_msg="", fail_msg="{name} of shape {shape} does not broadcast to {target}"):
    """``t`` expanded to ``shape`` (a view; nothing is copied; -1 keeps a dim).  With ``lead`` an int, ``t`` must have
    at most ``len(shape)`` dims and lead with ``shape[:lead]``, and is aligned on its leading dims: padded with trailing
    size-1 dims, so (B,) is per sample and (B, T) per frame.  ``lead=None``: ordinary trailing-aligned broadcasting.
    Raises ValueError ``"{name} of shape ... {lead_msg}"`` for the leading dims and ``fail_msg`` (formatted with name, the
    given shape, the padded shape and target) for a tensor that does not broadcast."""
    t = torch.as_tensor(t)
    shape, had = tuple(shape), tuple(t.shape)
    if lead is not None:
        if t.dim() < lead or t.dim() > len(shape) or had[:lead] != shape[:lead]:
            raise ValueError(f"{name} of shape {had} {lead_msg}")
        t = t.reshape(had + (1,) * (len(shape) - t.dim()))
    try:
        return t.expand(shape)
    except RuntimeError:
        raise ValueError(fail_msg.format(name=name, shape=had, padded=tuple(t.shape), target=shape)) from None


def check_inpaint_kwargs(kw, shape):
    """The editing inputs of ``model_kwargs`` for a sample of ``shape`` (B, T, F): None when neither ``inpaint_motion`` nor
    ``inpaint_mask`` is given, else (known, mask) with ``mask`` broadcast to ``shape`` (a view; nothing is copied).
    A mask of fewer dims than the sample is aligned on its leading (batch) dim: (B,) is per sample, (B, T) per frame.
    Raises ValueError for one without the other, a motion not shaped ``shape``, a mask whose leading dim is not B or that
    does not broadcast, values outside [0, 1] or non-finite values.  Host logic: runs on CPU tensors as well."""
    known, mask = kw.get("inpaint_motion"), kw.get("inpaint_mask")
    if known is None and mask is None:
        return None
    if known is None or mask is None:
        raise ValueError("inpaint_motion and inpaint_mask go together: give both or neither")
    known = torch.as_tensor(known)
    shape = tuple(int(v) for v in shape)
    if tuple(known.shape) != shape:
        raise ValueError(f"inpaint_motion has shape {tuple(known.shape)}, the sample {shape}")
    mask = expand_to(mask, 1, shape, "inpaint_mask", f"must lead with the batch size {shape[0]}")
    if not (known.is_floating_point() and mask.is_floating_point()):
        raise ValueError("inpaint_motion and inpaint_mask must be floating point")
    if not bool(torch.isfinite(known).all()):
        raise ValueError("inpaint_motion has non-finite values")
    if not bool(((mask >= 0) & (mask <= 1)).all()):  # NaN fails both comparisons
        raise ValueError("inpaint_mask values must lie in [0, 1]")
    return known, mask


def check_compose_kwargs(kw, shape, mode=None):
    """The composition inputs of ``model_kwargs`` for a sample of ``shape`` (B, T, F): None when no ``compose_*`` key is
    given, else a dict with ``weights`` broadcast to (B, K, T, F) (a view), ``K``, and either ``xf_proj`` (B, K, Dt) and
    ``xf_out`` (B, K, N, Dt) or ``text`` (B lists of K captions, for ``model.encode_text``).  Every input leads with B, so
    dist.shard_kwargs slices them.  The weights lead with (B, K) and are aligned on those dims: (B, K) is per sample and
    prompt, (B, K, T) per frame, (B, K, 1, F) per feature column.
    Raises ValueError for weights without prompts or prompts without weights, both embeddings and captions, one embedding
    without the other, shape or broadcast errors, K differing between samples or above MDM_COMPOSE_MAX_K, non-finite
    weights, ``xf_proj`` / ``xf_out`` given as well, and (with ``mode``) a mode without guidance.  Host logic."""
    w, cp, co, ct = (kw.get(k) for k in ("compose_weights", "compose_xf_proj", "compose_xf_out", "compose_text"))
    if w is None and cp is None and co is None and ct is None:
        return None
    if mode is not None and mode not in GUIDED:
        raise ValueError(f"composed prompts need classifier-free guidance; mode {mode!r} has none")
    if kw.get("xf_proj") is not None or kw.get("xf_out") is not None:
        raise ValueError("xf_proj / xf_out and compose_* are exclusive: the prompts of a composed sample are compose_*")
    if w is None:
        raise ValueError("compose_weights is required with composed prompts")
    if ct is not None and (cp is not None or co is not None):
        raise ValueError("give compose_text or compose_xf_proj / compose_xf_out, not both")
    if ct is None and (cp is None or co is None):
        raise ValueError("composed prompts need compose_text or both compose_xf_proj and compose_xf_out")
    B, T, F_ = (int(v) for v in shape)
    if ct is not None:
        if isinstance(ct, str) or len(ct) != B:
            raise ValueError(f"compose_text must hold {B} sequences of captions, one per sample")
        for seq in ct:
            if isinstance(seq, str) or not all(isinstance(c, str) for c in seq):
                raise ValueError("each entry of compose_text must be a sequence of caption strings")
        ks = {len(seq) for seq in ct}
        if len(ks) != 1:
            raise ValueError(f"every sample must have the same number of prompts, not {sorted(ks)}")
        K = ks.pop()
        ct = [list(seq) for seq in ct]
    else:
        cp, co = torch.as_tensor(cp), torch.as_tensor(co)
        if cp.dim() != 3 or co.dim() != 4 or cp.shape[0] != B or co.shape[0] != B or cp.shape[1] != co.shape[1]:
            raise ValueError(f"compose_xf_proj {tuple(cp.shape)} / compose_xf_out {tuple(co.shape)} must be (B={B}, K, Dt) "
                             "and (B, K, N, Dt)")
        K = int(cp.shape[1])
    if not 1 <= K <= L.COMPOSE_MAX_K:
        raise ValueError(f"{K} prompts per sample: the composed update takes 1 to {L.COMPOSE_MAX_K}")
    w = torch.as_tensor(w)
    if not w.is_floating_point():
        raise ValueError("compose_weights must be floating point")
    w = expand_to(w, 2, (B, K, T, F_), "compose_weights", f"must lead with (B, K) = {(B, K)} and have at most 4 dims")
    if not bool(torch.isfinite(w).all()):
        raise ValueError("compose_weights has non-finite values")
    return {"weights": w, "K": K, "xf_proj": cp, "xf_out": co, "text": ct}


def check_control_kwargs(kw, shape):
    """The joint-control inputs of ``model_kwargs`` for a sample of ``shape`` (B, T, F): None when none of the ``control_*``
    keys is given, else a dict with ``targets`` (B, T, J, 3), ``weights`` broadcast to it (a view), ``mean`` / ``std``
    (B, F), ``scale`` (float, default 1) and ``iters`` (int, default 1).  Every tensor leads with B, so dist.shard_kwargs
    slices them; the weights are aligned on that dim: (B,) per sample, (B, T) per frame, (B, T, J) per joint.
    Raises ValueError when only some of the four tensors are given (or a scale / iters without them), for an F not of the
    form 12 J - 1, a T over the kernels' LDS limit, shape or broadcast errors, non-finite targets, weights, mean or std,
    negative weights, a zero std, a non-finite scale or iters outside [1, MDM_CONTROL_MAX_ITERS].
    Scene constraints: ``control_scene`` (B, K, 12) primitive records (``motion_scene.pack_scene``) and
    ``control_joint_params`` (B, J, 2), the joints' radius and weight (default: 0 and 1), come back as ``scene`` /
    ``joint_params`` (absent without a scene).  A scene needs ``control_mean`` / ``control_std`` but no targets: ``targets``
    and ``weights`` are then None.  Raises ValueError for joint parameters without a scene, records
    ``motion_scene.check_records`` refuses, joint parameters of another shape, negative or not finite, and a T over the
    limit of a scene of K primitives.
    Tracks: ``control_tracks`` (B, T, Km, 12), per-frame records (``motion_scene.batch_tracks``), with or
    without a scene (one of no primitives then stands in) and with or without targets, come back as ``tracks`` and
    ``track_bounds`` (B, T, 4), the balls of the kernels' broad phase, computed here, once.  Raises ValueError for records
    ``motion_scene.check_tracks`` refuses and another shape.
    Terrain: ``control_terrain`` (B, Gz, Gx) height grids with ``control_terrain_rec`` (B, 8), their records
    (``motion_scene.batch_terrain``), with or without a scene, tracks and targets, come back as ``terrain`` / ``terrain_rec``;
    ``control_stand``, the stand weights (B, T, J) >= 0, or ``"contacts"`` (the step's own foot-contact labels over
    ``control_stand_threshold``, default 0.5, on the feet of the skeleton of width F), as ``stand`` (a tensor, or the feet and
    the threshold as ``stand_feet`` / ``stand_threshold``).  Raises ValueError for a record or stand weights without a grid, a
    grid without a record, what ``motion_scene.check_terrain`` / ``check_stand`` refuse, another batch size, ``"contacts"`` at
    a feature width without a skeleton and a non-finite threshold.
    Characters sampled together: ``control_partner_scenes`` (one list of batch rows per scene) with
    ``control_partner_placements`` (B, 3) = x, z, yaw and optionally ``control_partner_bones`` / ``control_partner_radius`` /
    ``control_partner_margin`` / ``control_partner_weight`` and ``control_contact_list`` (``motion_scene.contact`` entries
    between batch rows; a ``control_partner_weight`` of 0 leaves the partner slots out), with or without ``control_tracks`` (the static tracks in front of the partner slots), a scene, targets
    and a terrain, come back as ``partners``, the ``motion_scene.PartnerTables`` (made with ``model_kwargs["length"]``); the
    returned ``weights`` are then the tables' (the static weights plus the contacts') and ``targets`` zeros where none are
    given.  Raises ValueError for the other partner / contact keys without the scenes and placements and for everything
    ``motion_scene.partner_tables`` refuses.
    Self-collision avoidance: ``control_self``, a dict of ``body`` (a ``motion_scene.SelfBody``) and ``weight``
    >= 0, with ``control_mean`` / ``control_std`` and with or without targets, a scene, tracks and a terrain, comes back as
    ``self`` (the body and the weight); a weight of 0 or a body whose mask allows no pair is the call without the key.  Raises
    ValueError for another type, a body of another joint count, a weight that is negative or not finite and a T over
    ``motion_scene.SELF_MAX_FRAMES``; NotImplementedError together with the partner / contact keys (both rewrite the targets),
    handshake tables and ``canvas_control_*``.  Host logic."""
    from .motion_control import joints_for_feats, max_frames
    names = ("control_joints", "control_weights", "control_mean", "control_std")
    own = _check_control_self(kw, shape)
    partner = {k: kw.get(k) for k in PARTNER_KEYS}
    if any(v is not None for v in partner.values()):
        if partner["control_partner_scenes"] is None or partner["control_partner_placements"] is None:
            raise ValueError("characters sampled together need control_partner_scenes and control_partner_placements")
        if kw.get("length") is None:
            raise ValueError("characters sampled together need model_kwargs['length']")
        long = [k for k, v in kw.items() if v is not None and (k.startswith("handshake_") or k.startswith("canvas_control_"))]
        if long:
            raise ValueError(f"characters sampled together (control_partner_* / control_contact_*) cannot be combined with "
                             f"{', '.join(sorted(long))}: long motions are out of their scope")
    else:
        partner = None
    g, w, mean, std = (kw.get(k) for k in names)
    scene, jp, tracks = kw.get("control_scene"), kw.get("control_joint_params"), kw.get("control_tracks")
    terrain, trec, stand = kw.get("control_terrain"), kw.get("control_terrain_rec"), kw.get("control_stand")
    if terrain is None and any(kw.get(k) is not None for k in ("control_terrain_rec", "control_stand", "control_stand_threshold")):
        raise ValueError("control_terrain_rec / control_stand / control_stand_threshold given without control_terrain")
    if (tracks is not None or terrain is not None or partner is not None) and scene is None:
        scene = torch.zeros((int(shape[0]), 0, L.SCENE_REC))
    given = [k for k, v in zip(names, (g, w, mean, std)) if v is not None]
    extra = [k for k in ("control_scale", "control_iters") if kw.get(k) is not None]
    if jp is not None and scene is None:
        raise ValueError("control_joint_params given without control_scene")
    if not given and scene is None and own is None:
        if extra and not any(kw.get(k) is not None for k in CANVAS_CONTROL_KEYS + CANVAS_SCENE_KEYS + (CANVAS_TRACKS_KEY,) + CANVAS_TERRAIN_KEYS):  # canvas control's
            raise ValueError(f"{' / '.join(extra)} given without control_joints / control_weights / control_mean / control_std")
        return None
    if own is None and kw.get("control_self") is not None and scene is None and g is None and w is None:
        return None  # an inactive body and nothing else to steer by: the plain call, whatever mean / std say
    need = names[2:] if (scene is not None or own is not None) and g is None and w is None else names
    if any(k not in given for k in need):
        raise ValueError(f"joint control needs all of {', '.join(need)}; missing "
                         f"{', '.join(k for k in need if k not in given)}")
    B, T, F_ = (int(v) for v in shape)
    J = joints_for_feats(F_)
    out = {}
    limit = max_frames(F_)
    if scene is not None:
        from .motion_scene import check_records, max_frames as scene_max_frames
        scene = check_records(scene, "control_scene")
        if scene.dim() != 3 or scene.shape[0] != B:
            raise ValueError(f"control_scene has shape {tuple(scene.shape)}, expected ({B}, K, {L.SCENE_REC})")
        limit = scene_max_frames(F_, int(scene.shape[1]))
        if jp is None:
            jp = torch.tensor([0.0, 1.0]).expand(B, J, 2)
        jp = torch.as_tensor(jp)
        if tuple(jp.shape) != (B, J, 2) or not jp.is_floating_point():
            raise ValueError(f"control_joint_params of shape {tuple(jp.shape)} must be floating point {(B, J, 2)}")
        if not bool(torch.isfinite(jp).all()) or bool((jp < 0).any()):
            raise ValueError("control_joint_params (joint radius, joint weight) must be finite and >= 0")
        out = {"scene": scene, "joint_params": jp}
    if tracks is not None:
        from .motion_scene import check_tracks, track_bounds
        tracks = check_tracks(tracks, "control_tracks")
        if tracks.dim() != 4 or tuple(tracks.shape[:2]) != (B, T):
            raise ValueError(f"control_tracks has shape {tuple(tracks.shape)}, expected ({B}, {T}, Km, {L.SCENE_REC})")
        out.update(tracks=tracks, track_bounds=track_bounds(tracks))
    if terrain is not None:
        out.update(_terrain_inputs(terrain, trec, stand, kw.get("control_stand_threshold"), B, (B, T, J), F_, "control_"))
    if T > limit:
        raise ValueError(f"T = {T}: joint control takes at most {limit} frames at F = {F_}"
                         + (f" with {scene.shape[1]} primitives" if scene is not None else ""))
    mean, std = torch.as_tensor(mean), torch.as_tensor(std)
    if g is not None:
        g, w = torch.as_tensor(g), torch.as_tensor(w)
    for name, v in zip(names, (g, w, mean, std)):
        if v is not None and not v.is_floating_point():
            raise ValueError(f"{name} must be floating point")
    if g is not None:
        if tuple(g.shape) != (B, T, J, 3):
            raise ValueError(f"control_joints has shape {tuple(g.shape)}, expected {(B, T, J, 3)}")
        w = expand_to(w, 1, (B, T, J, 3), "control_weights", f"must lead with the batch size {B}")
    for name, v in (("control_mean", mean), ("control_std", std)):
        if tuple(v.shape) != (B, F_):
            raise ValueError(f"{name} has shape {tuple(v.shape)}, expected {(B, F_)} (one row per sample)")
    if g is not None:
        if not bool(torch.isfinite(g).all()):
            raise ValueError("control_joints has non-finite values")
        if not bool(torch.isfinite(w).all()):
            raise ValueError("control_weights has non-finite values")
        if not bool((w >= 0).all()):
            raise ValueError("control_weights must be >= 0")
    if not (bool(torch.isfinite(mean).all()) and bool(torch.isfinite(std).all())):
        raise ValueError("control_mean / control_std have non-finite values")
    if bool((std == 0).any()):
        raise ValueError("control_std has zero entries")
    scale = kw.get("control_scale")
    scale = 1.0 if scale is None else float(scale)
    if not math.isfinite(scale):
        raise ValueError("control_scale must be finite")
    iters = kw.get("control_iters")
    iters = 1 if iters is None else iters
    if isinstance(iters, bool) or int(iters) != iters or not 1 <= int(iters) <= L.CONTROL_MAX_ITERS:
        raise ValueError(f"control_iters must be an integer in [1, {L.CONTROL_MAX_ITERS}]")
    if partner is not None:
        from .motion_scene import partner_tables
        opts = {k: partner["control_partner_" + k] for k in ("radius", "margin", "weight") if partner["control_partner_" + k] is not None}
        tables = partner_tables(partner["control_partner_scenes"], partner["control_partner_placements"], kw["length"],
                                partner["control_partner_bones"], T=T, J=J, contacts=partner["control_contact_list"] or (),
                                static_tracks=0 if tracks is None else int(tracks.shape[2]), control_weights=w,
                                avoid=float(opts.get("weight", 1.0)) > 0, **opts)
        out["partners"] = tables
        if len(tables.contacts) or g is not None:
            g, w = torch.zeros((B, T, J, 3)) if g is None else g, tables.weights
    if own is not None:
        out["self"] = own
    return {"targets": g, "weights": w, "mean": mean, "std": std, "scale": scale, "iters": int(iters), **out}


def _check_control_self(kw, shape):
    """``control_self`` of ``model_kwargs`` checked: None without the key or when it changes nothing (weight 0, or a mask that
    allows no pair), else ``{"body": SelfBody, "weight": float}``."""
    own = kw.get("control_self")
    if own is None:
        return None
    from .motion_control import joints_for_feats
    from .motion_scene import SELF_MAX_FRAMES, SelfBody
    if not isinstance(own, dict) or set(own) != {"body", "weight"} or not isinstance(own["body"], SelfBody):
        raise ValueError("control_self must be a dict of body (a motion_scene.SelfBody, see motion_scene.self_body) and weight")
    body, weight = own["body"], float(own["weight"])
    if not (math.isfinite(weight) and weight >= 0):
        raise ValueError(f"control_self: weight must be finite and >= 0, not {weight}")
    B, T, F_ = (int(v) for v in shape)
    if body.J != joints_for_feats(F_):
        raise ValueError(f"control_self: a body of {body.J} joints for feature rows of {joints_for_feats(F_)} joints (F = {F_})")
    both = [k for k in PARTNER_KEYS if kw.get(k) is not None]
    if both:
        raise NotImplementedError(f"self-collision avoidance (DESIGN.md §33) cannot be combined with {', '.join(both)}: both "
                                  "rewrite the targets on every step")
    long = [k for k, v in kw.items() if v is not None and (k.startswith("handshake_") or k.startswith("canvas_control_"))]
    if long:
        raise NotImplementedError(f"self-collision avoidance (DESIGN.md §33) cannot be combined with {', '.join(sorted(long))}: "
                                  "long motions are out of its scope")
    if T > SELF_MAX_FRAMES:
        raise ValueError(f"T = {T}: self-collision avoidance takes at most {SELF_MAX_FRAMES} frames")
    if weight == 0 or not bool(body.allowed.any()):
        return None
    return {"body": body, "weight": weight}


PARTNER_KEYS = ("control_partner_scenes", "control_partner_placements", "control_partner_bones", "control_partner_radius",
                "control_partner_margin", "control_partner_weight", "control_contact_list")


def _terrain_inputs(terrain, trec, stand, threshold, N, stand_shape, F_, prefix):
    """The checked terrain entries of ``check_control_kwargs`` (N = B) and ``check_canvas_control_kwargs`` (N = M): ``terrain``
    (N, Gz, Gx), ``terrain_rec`` (N, 8) and ``stand`` of ``stand_shape`` or, for "contacts", ``stand_feet`` / ``stand_threshold``."""
    from .motion_scene import check_stand, check_terrain
    if trec is None:
        raise ValueError(f"{prefix}terrain given without {prefix}terrain_rec")
    terrain, trec = check_terrain(terrain, trec, prefix + "terrain")
    if terrain.dim() != 3 or terrain.shape[0] != N:
        raise ValueError(f"{prefix}terrain has shape {tuple(terrain.shape)}, expected ({N}, Gz, Gx)")
    out = {"terrain": terrain.cpu(), "terrain_rec": trec.cpu()}
    if isinstance(stand, str):
        from .motion_features import SKELETONS, skeleton_for_feats
        name = skeleton_for_feats(F_)
        if stand != "contacts" or name is None:
            raise ValueError(f'{prefix}stand must be stand weights {tuple(stand_shape)} or "contacts" (at a feature width with a '
                             f"skeleton), not {stand!r} at F = {F_}")
        thr = 0.5 if threshold is None else float(threshold)
        if not math.isfinite(thr):
            raise ValueError(f"{prefix}stand_threshold must be finite")
        out.update(stand_feet=tuple(SKELETONS[name].feet), stand_threshold=thr)
    else:
        if threshold is not None:
            raise ValueError(f'{prefix}stand_threshold goes with {prefix}stand="contacts"')
        if stand is not None:
            out.update(stand=check_stand(stand, stand_shape, prefix + "stand").cpu())
    return out


CANVAS_SCENE_KEYS = ("canvas_control_scene", "canvas_control_joint_params")
CANVAS_TRACKS_KEY = "canvas_control_tracks"
CANVAS_TERRAIN_KEYS = ("canvas_control_terrain", "canvas_control_terrain_rec", "canvas_control_stand", "canvas_control_stand_threshold")
CANVAS_CONTROL_KEYS = ("canvas_control_offsets", "canvas_control_rows", "canvas_control_joints", "canvas_control_weights",
                       "canvas_control_mean", "canvas_control_std")


def check_canvas_control_kwargs(kw, shape):
    """The canvas joint-control inputs of ``model_kwargs`` for a sample of ``shape`` (B, T, F): None when none
    of the ``canvas_control_*`` keys is given, else a dict of CPU tensors ``offsets`` int32 (M + 1), ``rows`` int32 (total),
    ``targets`` (total, J, 3), ``weights`` broadcast to it (a view), ``mean`` / ``std`` (M, F), and ``M``, ``total``, ``scale``
    (default 1) and ``iters`` (default 1).  Motion m's canvas frames are ``[offsets[m], offsets[m + 1])``; frame c lives in row
    ``rows[c]`` = window row * T + frame of the batch.  The tables describe whole motions, not batch rows: dist.shard_kwargs
    refuses them.
    Raises ValueError when only some of the six are given, without handshake tables when a motion spans several windows, for
    offsets that do not rise from 0 to the row count, rows outside [0, B T), repeated, at or past their window's ``length`` or
    naming a shared frame's copy instead of its owner, shape or broadcast errors, non-finite values, negative weights, a zero
    std, a non-finite scale, iters outside [1, MDM_CONTROL_MAX_ITERS], and together with per-window control or composed
    prompts.
    Scene constraints: ``canvas_control_scene`` (M, K, 12) records in the canvas frame and
    ``canvas_control_joint_params`` (M, J, 2) come back as ``scene`` / ``joint_params`` (absent without a scene), checked as
    ``check_control_kwargs`` checks its own; with a scene ``canvas_control_joints`` / ``canvas_control_weights`` may both be
    left out (``targets`` / ``weights`` None).
    Tracks: ``canvas_control_tracks`` (total, Km, 12), per-frame records in canvas order, with or without a
    scene and targets, come back as ``tracks`` and ``track_bounds`` (total, 4).
    Terrain: ``canvas_control_terrain`` (M, Gz, Gx) with ``canvas_control_terrain_rec`` (M, 8), one ground per
    motion in its canvas frame, with or without a scene, tracks and targets, come back as ``terrain`` / ``terrain_rec``;
    ``canvas_control_stand``, stand weights (total, J) in canvas order or ``"contacts"`` (with
    ``canvas_control_stand_threshold``, default 0.5), as ``stand`` or ``stand_feet`` / ``stand_threshold``, checked as
    ``check_control_kwargs`` checks its own.  Host logic."""
    from .motion_control import joints_for_feats
    names = CANVAS_CONTROL_KEYS
    vals = [kw.get(k) for k in names]
    scene, jp = (kw.get(k) for k in CANVAS_SCENE_KEYS)
    tracks = kw.get(CANVAS_TRACKS_KEY)
    terrain, trec, stand, sthr = (kw.get(k) for k in CANVAS_TERRAIN_KEYS)
    if terrain is None and (trec is not None or stand is not None or sthr is not None):
        raise ValueError("canvas_control_terrain_rec / canvas_control_stand / canvas_control_stand_threshold given without "
                         "canvas_control_terrain")
    if (tracks is not None or terrain is not None) and scene is None and vals[0] is not None:
        scene = torch.zeros((max(torch.as_tensor(vals[0]).numel() - 1, 0), 0, L.SCENE_REC))
    given = [k for k, v in zip(names, vals) if v is not None]
    if jp is not None and scene is None:
        raise ValueError("canvas_control_joint_params given without canvas_control_scene")
    if not given and scene is None and tracks is None and terrain is None:
        return None
    aim = scene is None or vals[2] is not None or vals[3] is not None
    need = names if aim else names[:2] + names[4:]
    if any(k not in given for k in need):
        raise ValueError(f"canvas joint control needs all of {', '.join(need)}; missing "
                         f"{', '.join(k for k in need if k not in given)}")
    if not aim:
        vals[2] = vals[3] = torch.zeros(0)  # placeholders through the common conversions below
    if any(kw.get(k) is not None for k in ("control_joints", "control_weights", "control_mean", "control_std", "control_scene",
                                           "control_tracks", "control_terrain")):
        raise ValueError("canvas_control_* and the per-window control_joints / control_weights are exclusive")
    if any(kw.get(k) is not None for k in ("compose_weights", "compose_xf_proj", "compose_xf_out", "compose_text")):
        raise ValueError("canvas joint control does not combine with composed prompts")
    B, T, F_ = (int(v) for v in shape)
    J = joints_for_feats(F_)
    off, rows, g, w, mean, std = (torch.as_tensor(v).detach().cpu() for v in vals)
    for name, v in ((names[0], off), (names[1], rows)):
        if v.dim() != 1 or v.is_floating_point() or v.is_complex() or v.dtype == torch.bool:
            raise ValueError(f"{name} must be a 1-D integer tensor, not {v.dtype} of shape {tuple(v.shape)}")
    for name, v in zip(names[2:], (g, w, mean, std)):
        if not v.is_floating_point():
            raise ValueError(f"{name} must be floating point")
    off, rows = off.to(torch.int64), rows.to(torch.int64)
    total, M = rows.numel(), off.numel() - 1
    if M < 0 or int(off[0]) != 0 or int(off[-1]) != total or bool((off[1:] < off[:-1]).any()):
        raise ValueError(f"canvas_control_offsets must rise from 0 to the row count {total}")
    if total and (int(rows.min()) < 0 or int(rows.max()) >= B * T):
        raise ValueError(f"canvas_control_rows must lie in [0, B * T) = [0, {B * T})")
    if torch.unique(rows).numel() != total:
        raise ValueError("canvas_control_rows repeats a row: every canvas frame has one owner row")
    length = kw.get("length")
    if length is not None and total:
        length = torch.as_tensor(length).detach().cpu().flatten().to(torch.int64)
        if length.numel() != B:
            raise ValueError(f"length must have {B} entries")
        if bool((rows % T >= length[rows // T]).any()):
            raise ValueError("canvas_control_rows points at a frame at or past its window's length")
    hs_names = ("handshake_offsets", "handshake_rows", "handshake_weights", "handshake_owner_rows")
    if all(kw.get(k) is None for k in hs_names):
        win = rows // T
        for m in range(M):
            seg = win[int(off[m]):int(off[m + 1])]
            if seg.numel() and int(seg.min()) != int(seg.max()):
                raise ValueError(f"motion {m} spans several windows: canvas joint control needs the handshake tables that tie "
                                 "them together")
    elif kw.get("handshake_owner_rows") is not None and kw.get("handshake_offsets") is not None:
        own = torch.as_tensor(kw["handshake_owner_rows"]).detach().cpu().flatten().to(torch.int64)
        first = torch.zeros(own.numel(), dtype=torch.bool)
        first[torch.as_tensor(kw["handshake_offsets"]).detach().cpu().flatten().to(torch.int64)[:-1]] = True
        if bool(torch.isin(rows, own[~first]).any()):
            raise ValueError("canvas_control_rows names a copy of a shared frame: every canvas frame is steered in its owner "
                             "(left) window's row, and the copy takes the owner's values")
    out = {}
    if scene is not None:
        from .motion_scene import check_records
        scene = check_records(scene, "canvas_control_scene").cpu()
        if scene.dim() != 3 or scene.shape[0] != M:
            raise ValueError(f"canvas_control_scene has shape {tuple(scene.shape)}, expected ({M}, K, {L.SCENE_REC})")
        jp = torch.tensor([0.0, 1.0]).expand(M, J, 2) if jp is None else torch.as_tensor(jp).detach().cpu()
        if tuple(jp.shape) != (M, J, 2) or not jp.is_floating_point():
            raise ValueError(f"canvas_control_joint_params of shape {tuple(jp.shape)} must be floating point {(M, J, 2)}")
        if not bool(torch.isfinite(jp).all()) or bool((jp < 0).any()):
            raise ValueError("canvas_control_joint_params (joint radius, joint weight) must be finite and >= 0")
        out = {"scene": scene, "joint_params": jp}
    if tracks is not None:
        from .motion_scene import check_tracks, track_bounds
        tracks = check_tracks(tracks, CANVAS_TRACKS_KEY).cpu()
        if tracks.dim() != 3 or tracks.shape[0] != total:
            raise ValueError(f"canvas_control_tracks has shape {tuple(tracks.shape)}, expected ({total}, Km, {L.SCENE_REC})")
        out.update(tracks=tracks, track_bounds=track_bounds(tracks))
    if terrain is not None:
        out.update(_terrain_inputs(terrain, trec, stand, sthr, M, (total, J), F_, "canvas_control_"))
    if aim:
        if tuple(g.shape) != (total, J, 3):
            raise ValueError(f"canvas_control_joints has shape {tuple(g.shape)}, expected {(total, J, 3)}")
        w = expand_to(w, 1, (total, J, 3), "canvas_control_weights", f"must lead with the row count {total}")
    for name, v in (("canvas_control_mean", mean), ("canvas_control_std", std)):
        if tuple(v.shape) != (M, F_):
            raise ValueError(f"{name} has shape {tuple(v.shape)}, expected {(M, F_)} (one row per motion)")
    if not bool(torch.isfinite(g).all()):
        raise ValueError("canvas_control_joints has non-finite values")
    if not bool(torch.isfinite(w).all()):
        raise ValueError("canvas_control_weights has non-finite values")
    if not bool((w >= 0).all()):
        raise ValueError("canvas_control_weights must be >= 0")
    if not (bool(torch.isfinite(mean).all()) and bool(torch.isfinite(std).all())):
        raise ValueError("canvas_control_mean / canvas_control_std have non-finite values")
    if bool((std == 0).any()):
        raise ValueError("canvas_control_std has zero entries")
    scale = kw.get("control_scale")
    scale = 1.0 if scale is None else float(scale)
    if not math.isfinite(scale):
        raise ValueError("control_scale must be finite")
    iters = kw.get("control_iters")
    iters = 1 if iters is None else iters
    if isinstance(iters, bool) or int(iters) != iters or not 1 <= int(iters) <= L.CONTROL_MAX_ITERS:
        raise ValueError(f"control_iters must be an integer in [1, {L.CONTROL_MAX_ITERS}]")
    return {"offsets": off.to(torch.int32), "rows": rows.to(torch.int32), "targets": g if aim else None,
            "weights": w if aim else None, "mean": mean, "std": std, "M": M, "total": total, "scale": scale, "iters": int(iters),
            **out}


def check_handshake_kwargs(kw, shape):
    """The long-motion tables of ``model_kwargs`` for a sample of ``shape`` (B, T, F): None when none of the ``handshake_*``
    keys is given or the tables have no shared frame, else a dict of CPU tensors ``offsets`` (nshared + 1), ``rows`` and
    ``owner_rows`` int32 and ``weights`` float32 (one per entry), and ``nshared``.  The entries of shared frame c are
    ``[offsets[c], offsets[c + 1])``, each a batch row times T plus a frame.
    Raises ValueError when only some of the four are given, for tables that are not 1-D or whose sizes disagree, offsets
    that do not start at 0, decrease or do not end at the entry count, a frame of fewer than two entries, rows outside
    [0, B T) or repeated, owner rows that are not a reordering of each frame's rows, and weights that are not finite or do
    not sum to 1 per frame (within 1e-5).  Raises NotImplementedError together with composed prompts or joint control.
    Host logic."""
    names = ("handshake_offsets", "handshake_rows", "handshake_weights", "handshake_owner_rows")
    vals = [kw.get(k) for k in names]
    given = [k for k, v in zip(names, vals) if v is not None]
    if not given:
        return None
    if len(given) != 4:
        raise ValueError(f"long-motion handshakes need all of {', '.join(names)}; missing "
                         f"{', '.join(k for k in names if k not in given)}")
    if any(kw.get(k) is not None for k in ("compose_weights", "compose_xf_proj", "compose_xf_out", "compose_text")):
        raise NotImplementedError("composed prompts over a long motion are not supported yet")
    if any(kw.get(k) is not None for k in ("control_joints", "control_weights", "control_mean", "control_std", "control_scene",
                                           "control_tracks", "control_terrain")):
        raise NotImplementedError("per-window joint control over a long motion is not supported: targets need canvas "
                                  "coordinates; give them as canvas_control_* (generate_long(control_joints=))")
    B, T, _ = (int(v) for v in shape)
    off, rows, w, own = (torch.as_tensor(v).detach().cpu() for v in vals)
    for name, v in zip(names, (off, rows, w, own)):
        if v.dim() != 1:
            raise ValueError(f"{name} must be 1-D, not of shape {tuple(v.shape)}")
    for name, v in ((names[0], off), (names[1], rows), (names[3], own)):
        if v.is_floating_point() or v.is_complex() or v.dtype == torch.bool:
            raise ValueError(f"{name} must be integer")
    if not w.is_floating_point():
        raise ValueError("handshake_weights must be floating point")
    off, rows, own = off.to(torch.int64), rows.to(torch.int64), own.to(torch.int64)
    ne = rows.numel()
    if off.numel() < 1 or int(off[0]) != 0 or int(off[-1]) != ne:
        raise ValueError(f"handshake_offsets must run from 0 to the entry count {ne}")
    if w.numel() != ne or own.numel() != ne:
        raise ValueError(f"handshake_weights ({w.numel()}) and handshake_owner_rows ({own.numel()}) need one value per "
                         f"entry of handshake_rows ({ne})")
    ns = off.numel() - 1
    cnt = off[1:] - off[:-1]
    if ns and int(cnt.min()) < 2:
        raise ValueError("every shared frame needs at least two entries, and offsets must not decrease")
    for name, v in ((names[1], rows), (names[3], own)):
        if ne and (int(v.min()) < 0 or int(v.max()) >= B * T):
            raise ValueError(f"{name} must lie in [0, B * T) = [0, {B * T})")
        if torch.unique(v).numel() != ne:
            raise ValueError(f"{name} repeats a row: every element must belong to one shared frame")
    fid = torch.repeat_interleave(torch.arange(ns), cnt)
    key = lambda v: torch.sort(fid * (B * T) + v).values  # noqa: E731
    if ne and not torch.equal(key(rows), key(own)):
        raise ValueError("handshake_owner_rows must list each shared frame's rows (owner first), as handshake_rows does")
    w64 = w.double()
    if not bool(torch.isfinite(w64).all()):
        raise ValueError("handshake_weights has non-finite values")
    if ns and float((torch.zeros(ns, dtype=torch.float64).index_add_(0, fid, w64) - 1).abs().max()) > 1e-5:
        raise ValueError("handshake_weights must sum to 1 over each shared frame")
    if ns == 0:
        return None
    return {"offsets": off.to(torch.int32), "rows": rows.to(torch.int32), "weights": w.to(torch.float32),
            "owner_rows": own.to(torch.int32), "nshared": ns}


def edit_rows_from_joints(edit_joints, mean, std, dim_pose, device=None, to_motion=None):
    """``edit_joints``, a list of N joint clips (n_i, J, 3) (or a padded (N, T, J, 3) tensor: every clip T frames), as the
    known motion of an edit: (rows (N, max n_i - 1, dim_pose), normalised with ``mean`` / ``std`` and zero past each clip,
    and the row counts n_i - 1).  One call of ``to_motion`` (default ``motion_features.joints_to_motion``, the HIP kernel;
    tests inject a CPU function) on the clips moved to ``device``, canonicalised as the training data was: on the floor,
    frame 0's root XZ at the origin and facing Z+.  Raises ValueError without mean / std or for a dim_pose that is neither
    the HumanML3D nor the KIT width."""
    if mean is None or std is None:
        raise ValueError("edit_joints needs the dataset's mean and std (feature rows are normalised, joints are not)")
    from .motion_features import joints_to_motion, skeleton_for_feats
    skeleton = skeleton_for_feats(dim_pose)
    if skeleton is None:
        raise ValueError(f"edit_joints needs dim_pose 263 (HumanML3D) or 251 (KIT), not {dim_pose}")
    if torch.is_tensor(edit_joints) or isinstance(edit_joints, np.ndarray):
        edit_joints = list(torch.as_tensor(edit_joints))
    clips = [torch.as_tensor(c) if device is None else torch.as_tensor(c).to(device) for c in edit_joints]
    rows = (to_motion or joints_to_motion)(clips, None, mean, std, skeleton=skeleton)
    return rows, [int(c.shape[0]) - 1 for c in clips]


def joint_clips_from_bvh(edit_bvh, bvh_options=None, edit_joints=None, edit_motion=None, device=None):
    """``edit_bvh``, a list of N BVH texts, paths or parsed files, as the known motion of an edit: the joint clips that
    ``motion_rig.bvh_to_joints`` reads from them at the model's frame rate, under ``bvh_options`` (its ``joint_map``,
    ``scale``, ``up``, ``basis`` and ``fps_out``).  The one place where files become clips: from here on they are
    ``edit_joints``.  Raises ValueError when the known motion is also given as joints or as rows, and for options without
    files."""
    if edit_bvh is None:
        if bvh_options is not None:
            raise ValueError("bvh_options goes with edit_bvh")
        return edit_joints
    if edit_joints is not None or edit_motion is not None:
        raise ValueError("edit_bvh, edit_joints and edit_motion are exclusive: the known motion is given as files, as joints "
                         "or as rows")
    options = dict(bvh_options or {})
    unknown = sorted(set(options) - {"joint_map", "scale", "up", "basis", "fps_out"})
    if unknown:
        raise ValueError(f"bvh_options takes joint_map, scale, up, basis and fps_out, not {unknown}")
    from .motion_rig import bvh_to_joints
    return bvh_to_joints(edit_bvh, device=device, **options)


def check_joint_edit_mask(mask, rows):
    """``mask`` (N, T, F), expanded, against the row counts of the clips an edit was given as: a clip of n joint frames has
    n - 1 feature rows, so a mask that keeps frame n - 1 or a later one asks for a row that does not exist."""
    for i, n in enumerate(rows):
        if bool((mask[i, n:] != 0).any()):
            raise ValueError(f"edit_mask keeps a frame at or past {n} of sample {i}, whose clip of {n + 1} joint frames gives "
                             f"{n} feature rows (the last frame only supplies velocities): the clip is one frame short")


def joint_edit_mask_frames(mask, rows):
    """The frames the mask of an ``edit_joints`` call covers: its frame dim, second to last as ``edit_mask`` broadcasts by
    its trailing dims ((T, 1), (N, T, 1), (N, T, F)); 0 for a mask without one ((F,), (1, F)).  Raises ValueError for a mask
    of more than 3 dims and for one that covers fewer frames than the longest clip has rows (``rows``)."""
    m = torch.as_tensor(mask)
    if m.dim() > 3:
        raise ValueError(f"edit_mask of shape {tuple(m.shape)} has more dims than (N, T, dim_pose)")
    T = int(m.shape[-2]) if m.dim() >= 2 and m.shape[-2] != 1 else 0
    if T and T < rows:
        raise ValueError(f"edit_mask covers {T} frames, the longest clip of edit_joints gives {rows} feature rows: give a "
                         "mask over the whole motion, or shorter clips")
    return T


def strength_steps(strength, num_steps) -> int:
    """The steps a motion-to-motion call runs of a sampler of ``num_steps`` steps: ``round(strength * num_steps)``, halves
    up.  All of them is the plain loop (the given motion is ignored), none returns the given motion, and n of them start
    at step n - 1.  Raises ValueError for a strength outside [0, 1] (NaN included)."""
    v = float(strength)
    if not 0.0 <= v <= 1.0:
        raise ValueError(f"strength must lie in [0, 1], not {strength}")
    return min(int(math.floor(v * int(num_steps) + 0.5)), int(num_steps))


class LatentStep(int):
    """The step of a spaced schedule at which inverted latents stand, with the step count of that schedule
    (``sample_steps``): ``DDPMTrainer.invert`` returns one, and ``generate(latents=, latent_step=)`` holds it against its
    own sampler."""

    def __new__(cls, step, sample_steps):
        self = super().__new__(cls, step)
        self.sample_steps = int(sample_steps)
        return self


def init_rows_from(init_motion, init_joints, init_bvh, bvh_options, mean, std, dim_pose, device=None, to_motion=None):
    """The motion a motion-to-motion call starts from, given as normalised rows ``init_motion`` (N, T_max, dim_pose), as N
    joint clips ``init_joints`` or as N BVH files ``init_bvh`` (the paths of the edit inputs: ``joint_clips_from_bvh``, then
    ``edit_rows_from_joints`` under ``mean`` / ``std``): (rows (N, T, dim_pose), the row count of every sample).  Raises
    ValueError for more than one of the three, joints or files without mean / std, rows of another shape, and rows that are
    not finite."""
    given = [k for k, v in (("init_motion", init_motion), ("init_joints", init_joints), ("init_bvh", init_bvh)) if v is not None]
    if len(given) != 1:
        raise ValueError("init_motion, init_joints and init_bvh are exclusive: the motion to start from is given as rows, as "
                         f"joints or as files, not as {' and '.join(given) or 'none of them'}")
    if init_motion is None:
        if mean is None or std is None:
            raise ValueError(f"{given[0]} needs the dataset's mean and std (feature rows are normalised, joints are not)")
        if init_bvh is not None:
            init_joints = joint_clips_from_bvh(init_bvh, bvh_options, device=device)
        x, have = edit_rows_from_joints(init_joints, mean, std, dim_pose, device, to_motion)
    else:
        x = torch.as_tensor(init_motion)
        if x.dim() != 3 or x.shape[2] != dim_pose or not x.is_floating_point():
            raise ValueError(f"init_motion of shape {tuple(x.shape)} must be floating point (N, T_max, {dim_pose})")
        have = [int(x.shape[1])] * int(x.shape[0])
    if not bool(torch.isfinite(x).all()):
        raise ValueError(f"{given[0]} has non-finite values")
    return x, have


def pad_frames(x, T):
    """``x`` (N, t, F) zero-padded along its frame dim to T frames (returned as it is when t >= T)."""
    if x.shape[1] >= T:
        return x
    return torch.cat([x, x.new_zeros((x.shape[0], T - x.shape[1], x.shape[2]))], dim=1)


class Conditioning:
    """The checked conditioning of one generate call over N samples, and the one description of the conditioning keywords of
    ``DDPMTrainer.generate_batch`` (N = its B) / ``generate`` / ``generate_bucketed``, which pass theirs on as
    ``**conditioning``.  Tensors cover the call, T_max frames; what does not depend on a batch is checked here, once, and
    ``kwargs`` / ``start_kwargs`` hand out a batch's rows and first T frames (views) and check that they cover its T.
    ``captions``: N strings, or with ``prompt_weights`` N sequences of K strings.
    ``edit_motion`` (N, T_max, dim_pose), normalised, and ``edit_mask`` broadcastable to it, values in [0, 1]: motion editing;
    both are kept where the mask is 1 (exactly, for a binary mask) and generated elsewhere (``edit``).
    ``prompt_weights`` (N, K, ...) broadcastable to (N, K, T_max, dim_pose): ``captions[i]`` is then a sequence of K captions,
    composed on every step under these weights; kept as (N, K, T_w, dim_pose), T_w 1 without a frame dim
    (``weights``).
    ``control_joints`` (N, T_max, J, 3) target joint positions and ``control_weights`` (N, ...) broadcastable to them, with the
    dataset's ``mean`` / ``std`` (dim_pose,), kept as float32: every step's x0 is moved ``control_iters`` times down the gradient
    of the weighted squared distance, scaled by ``control_scale`` (units in ``motion_control``; ``control``).
    ``scene``: obstacles the joints keep out of, a list of ``motion_scene`` primitives shared by all samples or
    one list per sample, with ``scene_joint_radius`` (J,) and ``scene_joint_weights`` (J,) (default 0 and 1); it needs ``mean`` /
    ``std``, acts through the same guidance as ``control_joints`` (``control_scale`` / ``control_iters``) and may come without
    targets (``scene_records`` / ``scene_joint_params``).
    ``scene_tracks``: obstacles that move, a list of ``motion_scene`` track stacks (``moving_sphere`` ...,
    ``character_tracks``) shared by all samples or one list per sample (or packed records), over T_max frames; with or without
    ``scene`` and targets, under the same ``mean`` / ``std``, joint radius and weights and guidance (``track_records``).
    ``terrain``: a height-map ground, one ``motion_scene`` terrain (``heightfield`` / ``ramp`` / ``stairs``)
    shared by all samples or a list of one per sample: every joint is kept above it, by its ``scene_joint_radius`` and under
    its ``scene_joint_weights``, through the same guidance, with or without ``scene``, ``scene_tracks`` and targets
    (``terrain_grids`` / ``terrain_records``).  ``terrain_stand``: which joints are pulled down onto the ground as well: None
    (none), ``"contacts"`` (on every step the foot joints whose foot-contact label in that step's x0, de-normalised, exceeds
    ``terrain_stand_threshold``), or stand weights (N, T_max, J) >= 0.
    ``edit_joints``: N joint clips (n_i, J, 3) in place of ``edit_motion`` (needs ``mean`` / ``std``), turned into feature rows
    once per call (``edit_rows_from_joints``: ``motion_features.joints_to_motion``) and zero-padded to the mask's
    frames; a clip of n frames gives n - 1 rows, so the mask may keep frames up to n - 2.
    ``edit_bvh``: N BVH texts, paths or parsed files in place of ``edit_joints``, read into clips first (``joint_clips_from_bvh``)
    at the model's frame rate by ``motion_rig.bvh_to_joints`` under ``bvh_options`` (a dict of its ``joint_map`` /
    ``scale`` / ``up`` / ``basis`` / ``fps_out``), from there on treated as ``edit_joints``; exclusive with it and ``edit_motion``.
    ``self_collision``: keep every joint out of the capsules of the character's own bones: None, True (the
    defaults) or a dict of ``weight`` (default 5; 0 leaves it out), ``radius_scale``, ``margin``, ``hops``, ``radii``, ``pairs``,
    ``joint_radius``, ``joint_weights`` (``motion_scene.self_body``'s) and ``offsets`` (J, 3), the skeleton's bone offsets (default
    ``motion_scene.default_offsets`` of the skeleton dim_pose names, at ``height``); it needs ``mean`` / ``std`` and acts through
    the same guidance (``control_scale`` / ``control_iters``), with or without targets, ``scene``, ``scene_tracks`` and ``terrain``.
    ``init_motion`` (N, T_max, dim_pose), normalised, with ``strength`` in [0, 1]: motion-to-motion (DESIGN.md §22;
    ``init_rows_from``, ``strength_steps``).  The motion is noised to an intermediate level of the chosen sampler's schedule and
    ``round(strength * steps)`` steps run from there under the caption: 1 is the plain call (the motion is ignored), 0 returns
    the motion, values in between stay the closer to it the smaller they are; with the call's ``seed`` the noise mixed into
    sample i is a function of (seed, i).  ``init_joints`` (N joint clips, needs ``mean`` / ``std``) or ``init_bvh`` (N files, read
    under ``bvh_options``) in place of ``init_motion``, converted as ``edit_joints`` / ``edit_bvh`` are; a clip must cover its
    sample's length.  It composes with the edit, prompt and control inputs, which act on every step that runs.
    ``latents`` (N, T, dim_pose, or a list of (T_i, dim_pose)) with ``latent_step`` in their place: x at that step of this call's
    schedule, as ``DDPMTrainer.invert`` returns them, to continue from; needs ``sampler="ddim"`` and the inversion's
    ``sample_steps``.  ``device``: where clips and files are converted; ``to_motion``: see ``edit_rows_from_joints``."""

    def __init__(self, captions, dim_pose, edit_motion=None, edit_mask=None, prompt_weights=None, control_joints=None,
                 control_weights=None, control_scale=1.0, control_iters=1, mean=None, std=None, edit_joints=None,
                 device=None, to_motion=None, edit_bvh=None, bvh_options=None, init_motion=None, init_joints=None,
                 init_bvh=None, strength=None, latents=None, latent_step=None, scene=None, scene_joint_radius=None,
                 scene_joint_weights=None, scene_tracks=None, terrain=None, terrain_stand=None, terrain_stand_threshold=0.5,
                 self_collision=None):
        self.captions, self.dim_pose = captions, dim_pose
        self.self_collision = self._self_collision(self_collision, dim_pose)
        self.init, self.strength, self.latents, self.latent_step = None, None, None, None
        if init_motion is not None or init_joints is not None or init_bvh is not None:
            if latents is not None:
                raise ValueError("latents and init_motion / init_joints / init_bvh are exclusive")
            if strength is None:
                raise ValueError("a motion to start from needs strength, the share of the sampler's steps to run")
            strength_steps(strength, 1)
            self.init = init_rows_from(init_motion, init_joints, init_bvh, bvh_options, mean, std, dim_pose, device, to_motion)
            if self.init[0].shape[0] != len(captions):
                raise ValueError(f"{self.init[0].shape[0]} motions to start from for {len(captions)} captions")
            self.strength = float(strength)
        elif strength is not None:
            raise ValueError("strength goes with init_motion, init_joints or init_bvh")
        if (latents is None) != (latent_step is None):
            raise ValueError("latents and latent_step go together: give both or neither")
        if latents is not None:
            if not torch.is_tensor(latents):
                lat = [torch.as_tensor(v) for v in latents]
                latents = torch.stack([pad_frames(v[None], max(u.shape[0] for u in lat))[0] for v in lat])
            if latents.dim() != 3 or latents.shape[0] != len(captions) or latents.shape[2] != dim_pose:
                raise ValueError(f"latents of shape {tuple(latents.shape)} must be (N = {len(captions)}, T, {dim_pose})")
            if not bool(torch.isfinite(latents).all()):
                raise ValueError("latents has non-finite values")
            self.latents, self.latent_step = latents, latent_step
        if init_bvh is not None and edit_bvh is None:
            bvh_options = None  # they were the init files'
        edit_joints = joint_clips_from_bvh(edit_bvh, bvh_options, edit_joints, edit_motion, device)
        self.weights = None if prompt_weights is None else self._compose(captions, prompt_weights, dim_pose)
        self.edit = None
        rows = None
        if edit_joints is not None:
            if edit_motion is not None:
                raise ValueError("edit_joints and edit_motion are exclusive: the known motion is given as joints or as rows")
            if edit_mask is None:
                raise ValueError("edit_joints and edit_mask go together: give both or neither")
            edit_motion, rows = edit_rows_from_joints(edit_joints, mean, std, dim_pose, device, to_motion)
            edit_motion = pad_frames(edit_motion, joint_edit_mask_frames(edit_mask, edit_motion.shape[1]))
        if edit_motion is not None or edit_mask is not None:
            if edit_motion is None or edit_mask is None:
                raise ValueError("edit_motion and edit_mask go together: give both or neither")
            k = torch.as_tensor(edit_motion)
            self.edit = (k, expand_to(edit_mask, None, k.shape, "edit_mask"))
            if rows is not None:
                check_joint_edit_mask(self.edit[1], rows)
        self.control = self._control(control_joints, control_weights, mean, std, dim_pose,
                                     scene is not None or scene_tracks is not None or terrain is not None
                                     or self.self_collision is not None)
        self.scene_records = self.scene_joint_params = self.track_records = None
        self.terrain_grids = self.terrain_records = self.terrain_stand = self.terrain_stand_threshold = None
        if scene is not None or scene_tracks is not None or terrain is not None:
            from .motion_control import joints_for_feats
            from .motion_scene import batch_scene, batch_terrain, batch_tracks, joint_params
            self.scene_records = batch_scene([] if scene is None else scene, len(captions))
            self.scene_joint_params = joint_params(joints_for_feats(dim_pose), scene_joint_radius, scene_joint_weights)
            if scene_tracks is not None:
                self.track_records = batch_tracks(scene_tracks, len(captions), self._track_frames(scene_tracks))
            if terrain is not None:
                self.terrain_grids, self.terrain_records = batch_terrain(terrain, len(captions))
                if isinstance(terrain_stand, str):
                    if terrain_stand != "contacts":
                        raise ValueError(f'terrain_stand must be None, "contacts" or stand weights, not {terrain_stand!r}')
                    self.terrain_stand, self.terrain_stand_threshold = terrain_stand, float(terrain_stand_threshold)
                elif terrain_stand is not None:
                    st = torch.as_tensor(terrain_stand, dtype=torch.float32)
                    if st.dim() != 3 or st.shape[0] != len(captions) or st.shape[2] != joints_for_feats(dim_pose):
                        raise ValueError(f"terrain_stand of shape {tuple(st.shape)} must be (N = {len(captions)}, T_max, "
                                         f"{joints_for_feats(dim_pose)})")
                    self.terrain_stand = st
        elif scene_joint_radius is not None or scene_joint_weights is not None:
            raise ValueError("scene_joint_radius / scene_joint_weights go with scene, scene_tracks or terrain")
        if terrain is None and terrain_stand is not None:
            raise ValueError("terrain_stand goes with terrain")
        self.control_scale, self.control_iters = control_scale, control_iters

    @staticmethod
    def _self_collision(opts, dim_pose):
        """``self_collision`` checked: None when it is not given or changes nothing (weight 0, no allowed pair), else the
        ``control_self`` entry of every batch's ``model_kwargs``."""
        if opts is None or opts is False:
            return None
        from .motion_features import skeleton_for_feats
        from .motion_scene import default_offsets, self_body
        opts = {} if opts is True else opts
        known = {"weight", "radius_scale", "margin", "hops", "radii", "pairs", "offsets", "height", "joint_radius", "joint_weights"}
        if not isinstance(opts, dict) or set(opts) - known:
            raise ValueError(f"self_collision must be None, True or a dict of {sorted(known)}")
        skeleton = skeleton_for_feats(dim_pose)
        if skeleton is None:
            raise ValueError(f"self_collision needs dim_pose 263 (HumanML3D) or 251 (KIT), not {dim_pose}")
        opts = dict(opts)
        weight = float(opts.pop("weight", 5.0))
        if not (math.isfinite(weight) and weight >= 0):
            raise ValueError(f"self_collision: weight must be finite and >= 0, not {weight}")
        height, offsets = opts.pop("height", None), opts.pop("offsets", None)
        if offsets is None:
            offsets = default_offsets(skeleton, **({} if height is None else {"height": height}))
        elif height is not None:
            raise ValueError("self_collision: height scales the default skeleton; with offsets= it has no meaning")
        body = self_body(offsets, skeleton, **opts)
        if weight == 0 or not bool(body.allowed.any()):
            return None
        return {"body": body, "weight": weight}

    @staticmethod
    def _track_frames(tracks):
        """T_max of ``scene_tracks``: the frames of packed records, the longest stack of lists."""
        if torch.is_tensor(tracks) or isinstance(tracks, np.ndarray):
            return int(tracks.shape[-3])
        flat = [t for v in tracks for t in ([v] if hasattr(v, "ndim") else v)]
        return max([int(t.shape[0]) for t in flat] + [1])

    @staticmethod
    def _compose(captions, prompt_weights, dim_pose):
        N = len(captions)
        for c in captions:
            if isinstance(c, str) or not all(isinstance(v, str) for v in c):
                raise ValueError("with prompt_weights every caption must be a sequence of K strings")
        ks = {len(c) for c in captions}
        if len(ks) != 1:
            raise ValueError(f"every sample must have the same number of prompts, not {sorted(ks)}")
        K = ks.pop()
        w = expand_to(torch.as_tensor(prompt_weights, dtype=torch.float32), 0, (N, K, -1, dim_pose), "prompt_weights",
                      "has more dims than (N, K, T, dim_pose)",
                      f"{{name}} of shape {{padded}} does not broadcast to (N={N}, K={K}, T, {dim_pose})")
        if not bool(torch.isfinite(w).all()):
            raise ValueError("prompt_weights has non-finite values")
        return w

    @staticmethod
    def _control(control_joints, control_weights, mean, std, dim_pose, scene=False):
        if control_joints is None and control_weights is None and not scene:
            return None
        if (control_joints is None) != (control_weights is None):
            raise ValueError("control_joints and control_weights go together: give both or neither")
        if mean is None or std is None:
            raise ValueError("joint control and scenes need the dataset's mean and std (targets and primitives are "
                             "de-normalised positions)")
        from .motion_control import joints_for_feats
        J = joints_for_feats(dim_pose)
        g = w = None
        if control_joints is not None:
            g = torch.as_tensor(control_joints, dtype=torch.float32)
            if g.dim() != 4 or tuple(g.shape[2:]) != (J, 3):
                raise ValueError(f"control_joints of shape {tuple(g.shape)} must be (N, T_max, {J}, 3)")
            w = expand_to(torch.as_tensor(control_weights, dtype=torch.float32), 1, g.shape, "control_weights",
                          f"must lead with N = {g.shape[0]}")
        ms = []
        for name, v in (("mean", mean), ("std", std)):
            v = torch.as_tensor(v if torch.is_tensor(v) else np.asarray(v), dtype=torch.float32).flatten()
            if v.numel() != dim_pose:
                raise ValueError(f"{name} must have {dim_pose} entries")
            ms.append(v)
        return {"joints": g, "weights": w, "mean": ms[0], "std": ms[1]}

    def captions_of(self, rows):
        """The captions of batch rows ``rows`` (a slice or an index tensor)."""
        return self.captions[rows] if isinstance(rows, slice) else [self.captions[i] for i in rows.tolist()]

    def edit_kwargs(self, rows, T):
        """``inpaint_motion`` / ``inpaint_mask`` of rows ``rows``, their first T frames; {} without editing."""
        if self.edit is None:
            return {}
        k, msk = self.edit
        if k.dim() != 3 or k.shape[2] != self.dim_pose or k.shape[1] < T:
            raise ValueError(f"edit_motion of shape {tuple(k.shape)} must be (N, T_max >= {T}, {self.dim_pose})")
        return {"inpaint_motion": k[rows, :T], "inpaint_mask": msk[rows, :T]}

    def text_kwargs(self, rows, T):
        """The rows' captions as ``text`` (the sampler encodes them), or the composed prompts and their weights' rows and
        first T frames."""
        caps, w = self.captions_of(rows), self.weights
        if w is None:
            return {"text": caps}
        if w.shape[2] != 1 and w.shape[2] < T:
            raise ValueError(f"prompt_weights has {w.shape[2]} frames, the batch {T}")
        w = w[rows]
        return {"compose_text": [list(c) for c in caps], "compose_weights": w[:, :, :T] if w.shape[2] != 1 else w}

    def control_kwargs(self, rows, T, device):
        """``control_*`` of rows ``rows``, their first T frames, on ``device``; {} without control."""
        if self.control is None:
            return {}
        c, out = self.control, {}
        if c["joints"] is not None:
            g = c["joints"][rows]
            if g.shape[1] < T:
                raise ValueError(f"control_joints has {g.shape[1]} frames, the batch {T}")
            out = {"control_joints": g[:, :T].to(device), "control_weights": c["weights"][rows][:, :T].to(device)}
        if self.scene_records is not None:
            rec = self.scene_records[rows]
            out.update(control_scene=rec.to(device),
                       control_joint_params=self.scene_joint_params.to(device).expand(rec.shape[0], -1, -1))
        if self.track_records is not None:
            trk = self.track_records[rows]
            if trk.shape[1] < T:  # a track ends where its stack ends: padding from there on
                trk = torch.cat([trk, trk.new_zeros((trk.shape[0], T - trk.shape[1]) + tuple(trk.shape[2:]))], dim=1)
            out.update(control_tracks=trk[:, :T].contiguous().to(device))
        if self.terrain_grids is not None:
            out.update(control_terrain=self.terrain_grids[rows].to(device), control_terrain_rec=self.terrain_records[rows].to(device))
            if isinstance(self.terrain_stand, str):
                out.update(control_stand=self.terrain_stand, control_stand_threshold=self.terrain_stand_threshold)
            elif self.terrain_stand is not None:
                st = self.terrain_stand[rows]
                if st.shape[1] < T:
                    raise ValueError(f"terrain_stand has {st.shape[1]} frames, the batch {T}")
                out.update(control_stand=st[:, :T].contiguous().to(device))
        if self.self_collision is not None:
            out.update(control_self=self.self_collision)
        n = len(self.captions_of(rows))
        return {**out, "control_mean": c["mean"].to(device).expand(n, -1), "control_std": c["std"].to(device).expand(n, -1),
                "control_scale": self.control_scale, "control_iters": self.control_iters}

    def start_kwargs(self, rows, T, lengths, num_steps, sampler, device):
        """Where the loop of the batch of rows ``rows`` at T frames starts, for a sampler of ``num_steps`` steps:
        ``(loop arguments, result)``.  ({}, None): the plain loop (nothing given, or a strength that runs every step).
        ``init_motion`` and ``start_step``: the rows' motions, their first T frames, and the step ``strength_steps`` maps the
        strength to.  ({}, the motions): a strength that runs no step.  ``noise`` and ``start_step``: the rows' latents.
        Raises ValueError for a motion with fewer rows than its sample's length, latents of fewer than T frames, latents
        with a sampler other than "ddim", and a ``latent_step`` outside the schedule or from another step count."""
        if self.latents is not None:
            ls = self.latent_step
            if sampler != "ddim":
                raise ValueError(f'latents continue a DDIM inversion: they need sampler="ddim", not {sampler!r}')
            if getattr(ls, "sample_steps", num_steps) != num_steps or not 0 <= int(ls) < num_steps:
                raise ValueError(f"latent_step {int(ls)} (of {getattr(ls, 'sample_steps', '?')} steps) does not belong to this "
                                 f"call's {num_steps}-step schedule: give the sample_steps of the inversion")
            if self.latents.shape[1] < T:
                raise ValueError(f"latents has {self.latents.shape[1]} frames, the batch {T}")
            return {"noise": self.latents[rows][:, :T].to(device), "start_step": int(ls)}, None
        if self.init is None:
            return {}, None
        n_run = strength_steps(self.strength, num_steps)
        if n_run == num_steps:
            return {}, None
        x, have = self.init
        ids = list(range(x.shape[0]))[rows] if isinstance(rows, slice) else rows.tolist()
        for i, n in zip(ids, torch.as_tensor(lengths).flatten().tolist()):
            if have[i] < min(int(n), T):
                raise ValueError(f"sample {i}: a motion of {have[i]} rows to start from is shorter than its length "
                                 f"{min(int(n), T)}")
        x = pad_frames(x[rows], T)[:, :T].to(device, torch.float32)
        if n_run == 0:
            return {}, x.clone()
        return {"init_motion": x, "start_step": n_run - 1}, None

    def kwargs(self, rows, T, device):
        """The ``model_kwargs`` entries of the batch of rows ``rows`` (a slice or an index tensor) at T frames."""
        return {**self.text_kwargs(rows, T), **self.edit_kwargs(rows, T), **self.control_kwargs(rows, T, device)}

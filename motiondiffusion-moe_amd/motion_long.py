"""Long motions from overlapping windows: host tables for the handshake kernel (csrc/handshake.hip).

A long motion is a script of segments ``(caption_i, length_i)``, each at most the model's ``num_frames``, and an overlap
``h``.  Window i covers canvas frames ``[s_i, s_i + length_i)`` with ``s_0 = 0`` and ``s_{i+1} = s_i + length_i - h``; the
canvas has ``sum(length_i) - (n - 1) h`` frames.  With ``0 <= h <= min(length_i) / 2`` no canvas frame is covered by more
than two windows.  The windows are rows of one sampler batch, padded to a common T.

Every canvas frame two windows cover is a "shared frame" of the tables: its entries are that frame's row in the left
window, then in the right one (``rows[e] = window_row * T + frame``).  On every step the sampler writes the weighted mean of
the two eps rows back into both (``weights``: a linear crossfade, the right window weighing ``(j + 1) / (h + 1)`` at overlap
frame j, or ``"uniform"`` halves), and copies x_T and the step noise from the left ("owner") window into the right one.
The overlap frames of neighbouring windows then stay bit for bit equal on every step, and the canvas is the windows' valid
frames.  ``script_plans``, ``canvas_conditioning``, ``plan_batches``, ``batch_tables`` and ``gather_canvases`` are the host
half of ``DDPMTrainer.generate_long``; ``canvas_frame_rows`` and ``batch_control_tables`` name the row that owns each canvas
frame for joint control over the whole canvas.  Host logic only: runs without a GPU.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .conditioning import check_joint_edit_mask, edit_rows_from_joints, expand_to, joint_clips_from_bvh, pad_frames

BLENDS = ("linear", "uniform")


def _int(v, name: str) -> int:
    if isinstance(v, bool) or int(v) != v:
        raise ValueError(f"{name} must be an integer, not {v!r}")
    return int(v)


def plan_windows(lengths: Sequence[int], overlap: int, max_len: Optional[int] = None) -> Tuple[List[int], int]:
    """Window starts and the canvas length of a script with these window ``lengths`` and ``overlap`` frames.
    Raises ValueError for an empty script, a length below 1 or above ``max_len``, and an overlap below 0 or above half
    the shortest window."""
    lengths = [_int(n, "a window length") for n in lengths]
    h = _int(overlap, "overlap")
    if not lengths:
        raise ValueError("a long motion needs at least one window")
    if min(lengths) < 1:
        raise ValueError(f"window lengths must be >= 1, not {min(lengths)}")
    if max_len is not None and max(lengths) > max_len:
        raise ValueError(f"window length {max(lengths)} exceeds the model's {max_len} frames")
    if h < 0:
        raise ValueError(f"overlap must be >= 0, not {h}")
    if 2 * h > min(lengths):
        raise ValueError(f"overlap {h} exceeds half the shortest window ({min(lengths)} frames): a frame would be covered "
                         "by more than two windows")
    starts = [0]
    for n in lengths[:-1]:
        starts.append(starts[-1] + n - h)
    return starts, starts[-1] + lengths[-1]


def _check_plan(starts, lengths, T, overlap):
    starts, lengths = list(starts), list(lengths)
    if len(starts) != len(lengths):
        raise ValueError(f"{len(starts)} starts for {len(lengths)} windows")
    want, _ = plan_windows(lengths, overlap)
    if [int(s) for s in starts] != want:
        raise ValueError(f"starts {starts} do not follow from lengths {lengths} and overlap {overlap}: {want}")
    if _int(T, "T") < max(lengths):
        raise ValueError(f"T = {T} is shorter than the longest window ({max(lengths)} frames)")
    return want, [int(n) for n in lengths]


def handshake_tables(starts, lengths, T: int, overlap: int, blend: str = "linear", first_row: int = 0) -> Dict:
    """The tables of one long motion whose windows are batch rows ``first_row, first_row + 1, ...`` padded to T frames:
    ``offsets`` int32 (nshared + 1), ``rows`` int32 (2 nshared; left window first), ``weights`` float32 like ``rows``
    (``blend`` "linear" or "uniform"), and the owner table ``owner_rows`` (its first entry per frame, the left window, is
    the source of the copy; its weights are None)."""
    if blend not in BLENDS:
        raise ValueError(f"blend must be one of {BLENDS}, not {blend!r}")
    starts, lengths = _check_plan(starts, lengths, T, overlap)
    h, n = int(overlap), len(lengths)
    rows, weights = [], []
    for i in range(n - 1):
        left, right = first_row + i, first_row + i + 1
        for j in range(h):
            wr = (j + 1) / (h + 1) if blend == "linear" else 0.5
            rows += [left * T + lengths[i] - h + j, right * T + j]
            weights += [1.0 - wr, wr]
    ns = (n - 1) * h
    rows = np.asarray(rows, dtype=np.int32).reshape(-1)
    return {"offsets": np.arange(0, 2 * ns + 1, 2, dtype=np.int32), "rows": rows,
            "weights": np.asarray(weights, dtype=np.float32).reshape(-1), "owner_rows": rows.copy()}


def merge_tables(tables: Sequence[Dict]) -> Dict:
    """The tables of several long motions in one batch (each built with its own ``first_row``), concatenated."""
    offsets, rows, weights, owner, base = [np.zeros(1, np.int32)], [], [], [], 0
    for t in tables:
        offsets.append(t["offsets"][1:] + base)
        base += int(t["offsets"][-1])
        rows.append(t["rows"]), weights.append(t["weights"]), owner.append(t["owner_rows"])
    cat = lambda v, dt: np.concatenate(v).astype(dt) if v else np.zeros(0, dt)  # noqa: E731
    return {"offsets": np.concatenate(offsets).astype(np.int32), "rows": cat(rows, np.int32),
            "weights": cat(weights, np.float32), "owner_rows": cat(owner, np.int32)}


def script_plans(scripts, overlap, num_frames):
    """Checked scripts: per motion (captions, lengths, window starts, canvas length)."""
    if isinstance(scripts, (str, bytes)) or len(scripts) == 0:
        raise ValueError("scripts must be a non-empty list of long motions, each a list of (caption, length)")
    plans = []
    for i, sc in enumerate(scripts):
        if isinstance(sc, (str, bytes)) or len(sc) == 0:
            raise ValueError(f"motion {i}: a script is a non-empty list of (caption, length) segments")
        caps, lens = [], []
        for seg in sc:
            if len(seg) != 2 or not isinstance(seg[0], str):
                raise ValueError(f"motion {i}: segment {seg!r} is not a (caption, length) pair")
            caps.append(seg[0])
            lens.append(seg[1])
        starts, C = plan_windows(lens, overlap, num_frames)
        plans.append((caps, [int(n) for n in lens], starts, C))
    return plans


def plan_batches(plans, batch_size: int) -> List[List[int]]:
    """The motions of ``plans`` (from ``script_plans``) dealt into batches in order: whole motions, at most ``batch_size``
    windows each.  Raises ValueError for a motion of more windows than that."""
    batches, cur = [], []
    for i, (_, lens, _, _) in enumerate(plans):
        if len(lens) > batch_size:
            raise ValueError(f"motion {i} has {len(lens)} windows, more than batch_size = {batch_size}")
        if cur and sum(len(plans[j][1]) for j in cur) + len(lens) > batch_size:
            batches.append(cur)
            cur = []
        cur.append(i)
    if cur:
        batches.append(cur)
    return batches


def batch_tables(plans, idx, T: int, overlap: int, blend: str = "linear") -> Dict[str, torch.Tensor]:
    """The ``handshake_*`` model kwargs of one batch: the tables of motions ``idx``, whose windows are consecutive batch
    rows in that order padded to T frames, merged."""
    tabs, row = [], 0
    for i in idx:
        tabs.append(handshake_tables(plans[i][2], plans[i][1], T, overlap, blend, first_row=row))
        row += len(plans[i][1])
    return {"handshake_" + k: torch.from_numpy(v) for k, v in merge_tables(tabs).items()}


def canvas_frame_rows(starts, lengths, T: int, first_row: int = 0) -> np.ndarray:
    """For every canvas frame of one long motion whose windows are batch rows ``first_row, first_row + 1, ...`` padded to T
    frames, the row (``window_row * T + frame``) of its owner: the first (left) window that covers it, as in
    ``handshake_tables``' ``owner_rows`` and ``windows_to_canvas``.  int32 (canvas_len,): every canvas frame exactly once."""
    starts, lengths, C = _span(starts, lengths)
    if _int(T, "T") < max(lengths):
        raise ValueError(f"T = {T} is shorter than the longest window ({max(lengths)} frames)")
    rows = np.empty(C, dtype=np.int32)
    for i in reversed(range(len(starts))):  # a left window overwrites its right neighbour's share of an overlap
        rows[starts[i]:starts[i] + lengths[i]] = (int(first_row) + i) * int(T) + np.arange(lengths[i], dtype=np.int32)
    return rows


def batch_control_tables(plans, idx, T: int, joints, weights) -> Dict[str, torch.Tensor]:
    """The ``canvas_control_*`` table kwargs of one batch, next to ``batch_tables``: for the motions ``idx``,
    whose windows are consecutive batch rows in that order padded to T frames, ``canvas_control_offsets`` (len(idx) + 1),
    ``canvas_control_rows`` (``canvas_frame_rows`` of each, concatenated) and the canvas-order ``canvas_control_joints`` /
    ``canvas_control_weights`` (sum of canvas lengths, J, 3) from ``joints[i]`` / ``weights[i]`` (C_i, J, 3); ``joints`` None
    (a scene without targets): the two row tables alone."""
    offsets, rows, row = [0], [], 0
    for i in idx:
        rows.append(canvas_frame_rows(plans[i][2], plans[i][1], T, first_row=row))
        offsets.append(offsets[-1] + plans[i][3])
        row += len(plans[i][1])
    out = {"canvas_control_offsets": torch.tensor(offsets, dtype=torch.int32),
           "canvas_control_rows": torch.from_numpy(np.concatenate(rows))}
    if joints is not None:
        out.update(canvas_control_joints=torch.cat([joints[i] for i in idx]).contiguous(),
                   canvas_control_weights=torch.cat([weights[i] for i in idx]).contiguous())
    return out


def canvas_control(plans, dim_pose, control_joints=None, control_weights=None, control_scale=None, control_iters=None,
                   mean=None, std=None, device=None, scene=None, scene_joint_radius=None, scene_joint_weights=None,
                   scene_tracks=None, terrain=None, terrain_stand=None, terrain_stand_threshold=0.5):
    """The joint-control inputs of ``DDPMTrainer.generate_long`` (described there), checked once for the call:
    one (C_i, J, 3) target array per motion of ``plans`` in canvas frames and weights broadcastable to it (aligned on the
    frame dim), with the dataset's ``mean`` / ``std``.  Returns ``tables(idx, T)``: the ``canvas_control_*`` model kwargs
    (``batch_control_tables``, one mean / std row per motion, ``control_scale`` / ``control_iters`` where given) of the batch
    of motions ``idx`` at T frames, on ``device``; {} without control.  Raises ValueError for targets without weights or the
    reverse, a scale or iteration count without them, missing mean / std, not one entry per motion, and canvas shapes.
    ``scene``: one list of ``motion_scene`` primitives per motion, in its canvas frame, with
    ``scene_joint_radius`` / ``scene_joint_weights`` (J,); it may come without targets, and adds ``canvas_control_scene`` /
    ``canvas_control_joint_params`` to the tables.  ``scene_tracks``: one list of ``motion_scene`` track stacks
    per motion, over its canvas frames, with or without ``scene`` and targets; it adds ``canvas_control_tracks``.
    ``terrain``: one ``motion_scene`` terrain per motion, in its canvas frame, with or without the rest;
    ``terrain_stand``: None, ``"contacts"`` (with ``terrain_stand_threshold``) or one (C_i, J) array of stand weights per
    motion; they add ``canvas_control_terrain`` / ``canvas_control_terrain_rec`` / ``canvas_control_stand``."""
    aim = control_joints is not None or control_weights is not None
    if scene is None and scene_tracks is None and terrain is None and (scene_joint_radius is not None or scene_joint_weights is not None):
        raise ValueError("scene_joint_radius / scene_joint_weights go with scene, scene_tracks or terrain")
    if terrain is None and terrain_stand is not None:
        raise ValueError("terrain_stand goes with terrain")
    if scene is None and (scene_tracks is not None or terrain is not None):
        scene = [[] for _ in plans]
    if not aim and scene is None:
        if control_scale is not None or control_iters is not None:
            raise ValueError("control_scale / control_iters given without control_joints / control_weights")
        return lambda idx, T: {}
    N = len(plans)
    if aim and (control_joints is None or control_weights is None):
        raise ValueError("control_joints and control_weights go together: give both or neither")
    if mean is None or std is None:
        raise ValueError("joint control and scenes need the dataset's mean and std (targets and primitives are "
                         "de-normalised positions)")
    for name, v in (("control_joints", control_joints), ("control_weights", control_weights)) if aim else ():
        if torch.is_tensor(v) or isinstance(v, np.ndarray) or len(v) != N or any(x is None for x in v):
            raise ValueError(f"{name} must hold one entry per motion ({N}), each over its canvas: for every motion or for none")
    from .motion_control import joints_for_feats
    J = joints_for_feats(dim_pose)
    records = params = None
    if scene is not None:
        from .motion_scene import Primitive, batch_scene, joint_params
        if torch.is_tensor(scene) or isinstance(scene, np.ndarray) or len(scene) != N or any(
                s is None or isinstance(s, Primitive) for s in scene):
            raise ValueError(f"scene must hold one list of primitives per motion ({N}), in its canvas frame")
        records = batch_scene(scene, N)
        params = joint_params(J, scene_joint_radius, scene_joint_weights)
    tracks = None
    if scene_tracks is not None:
        from .motion_scene import _is_stack, pack_tracks
        if torch.is_tensor(scene_tracks) or isinstance(scene_tracks, np.ndarray) or len(scene_tracks) != N or any(
                t is None or _is_stack(t) for t in scene_tracks):
            raise ValueError(f"scene_tracks must hold one list of track stacks per motion ({N}), over its canvas frames")
        tracks = [pack_tracks(t, plans[i][3]) for i, t in enumerate(scene_tracks)]
    grounds = stands = None
    if terrain is not None:
        from .motion_scene import Terrain, batch_terrain, check_stand
        if isinstance(terrain, Terrain) or len(terrain) != N:
            raise ValueError(f"terrain must hold one terrain per motion ({N}), in its canvas frame")
        grounds = batch_terrain(list(terrain), N)
        if isinstance(terrain_stand, str):
            if terrain_stand != "contacts":
                raise ValueError(f'terrain_stand must be None, "contacts" or one array of stand weights per motion, not {terrain_stand!r}')
        elif terrain_stand is not None:
            if torch.is_tensor(terrain_stand) or isinstance(terrain_stand, np.ndarray) or len(terrain_stand) != N:
                raise ValueError(f"terrain_stand must hold one (canvas_len, J) array of stand weights per motion ({N})")
            stands = [check_stand(s, (plans[i][3], J), f"terrain_stand of motion {i}") for i, s in enumerate(terrain_stand)]
    joints, weights = [], []
    for i, (g, w) in enumerate(zip(control_joints, control_weights) if aim else ()):
        C = plans[i][3]
        g = torch.as_tensor(g).detach().to("cpu", torch.float32)
        if tuple(g.shape) != (C, J, 3):
            raise ValueError(f"control_joints of motion {i} has shape {tuple(g.shape)}, its canvas {(C, J, 3)}")
        w = expand_to(torch.as_tensor(w).detach().to("cpu", torch.float32), 0, (C, J, 3), "control_weights",
                      "has more dims than (canvas_len, J, 3)",
                      f"{{name}} of motion {i} has shape {{shape}}, not broadcastable to its canvas {{target}} (aligned on the "
                      "frame dim: (C,), (C, J) or (C, J, 3))")
        joints.append(g)
        weights.append(w)
    ms = []
    for name, v in (("mean", mean), ("std", std)):
        v = torch.as_tensor(v if torch.is_tensor(v) else np.asarray(v)).detach().to("cpu", torch.float32).flatten()
        if v.numel() != dim_pose:
            raise ValueError(f"{name} must have {dim_pose} entries")
        ms.append(v)

    def tables(idx, T):
        kw = batch_control_tables(plans, idx, T, joints if aim else None, weights)
        if records is not None:
            kw.update(canvas_control_scene=records[list(idx)], canvas_control_joint_params=params.expand(len(idx), -1, -1))
        if tracks is not None:
            Km = max(tracks[i].shape[1] for i in idx)
            kw.update(canvas_control_tracks=torch.cat([torch.nn.functional.pad(tracks[i], (0, 0, 0, Km - tracks[i].shape[1]))
                                                       for i in idx]).contiguous())
        if grounds is not None:
            kw.update(canvas_control_terrain=grounds[0][list(idx)], canvas_control_terrain_rec=grounds[1][list(idx)])
            if stands is not None:
                kw.update(canvas_control_stand=torch.cat([stands[i] for i in idx]).contiguous())
        kw.update(canvas_control_mean=ms[0].expand(len(idx), -1), canvas_control_std=ms[1].expand(len(idx), -1))
        kw = {k: v.to(device) for k, v in kw.items()}
        if grounds is not None and isinstance(terrain_stand, str):
            kw.update(canvas_control_stand=terrain_stand, canvas_control_stand_threshold=float(terrain_stand_threshold))
        kw.update({k: v for k, v in (("control_scale", control_scale), ("control_iters", control_iters)) if v is not None})
        return kw

    return tables


def gather_canvases(values, plans, idx, T: int, dim_pose: int, what: str) -> torch.Tensor:
    """``values[i]``, broadcast to motion i's canvas (C_i, dim_pose), for the motions ``idx`` of a batch, gathered into
    their window rows (sum of windows, T, dim_pose) as float32."""
    parts = []
    for i in idx:
        _, lens, starts, C = plans[i]
        x = expand_to(torch.as_tensor(values[i], dtype=torch.float32), None, (C, dim_pose), what,
                      fail_msg=f"{{name}} of motion {i} has shape {{shape}}, not broadcastable to its canvas {{target}}")
        parts.append(canvas_to_windows(x, starts, lens, T))
    return torch.cat(parts)


def canvas_conditioning(plans, dim_pose, *, edit_motion=None, edit_mask=None, noise=None, init_motion=None, strength=None,
                        edit_joints=None, mean=None, std=None, edit_bvh=None, bvh_options=None, device=None, to_motion=None):
    """The per-motion inputs of ``DDPMTrainer.generate_long`` (described there), one entry per motion of ``plans`` each, checked
    once for the call; joint clips and files become rows that start their canvas (``to_motion``: as in
    ``conditioning.edit_rows_from_joints``).  Returns ``window_rows(idx, T)``: for the batch of motions ``idx`` at T frames a
    dict of the inputs given, gathered into the batch's window rows on ``device``; it raises ValueError for a canvas of
    another shape.  Raises ValueError for inputs that exclude each other, lack their partner, have not one entry per motion or
    are given for some motions only, and for a clip longer than its canvas or cut short by its mask."""
    N = len(plans)
    if edit_bvh is not None or bvh_options is not None:
        edit_joints = joint_clips_from_bvh(edit_bvh, bvh_options, edit_joints, edit_motion, device)
    if edit_joints is not None:
        if edit_motion is not None:
            raise ValueError("edit_joints and edit_motion are exclusive: the known motion is given as joints or as rows")
        if edit_mask is None or len(edit_joints) != N or len(edit_mask) != N or any(mk is None for mk in edit_mask):
            raise ValueError(f"edit_joints needs one clip and one edit_mask per motion ({N})")
        rows, nrows = edit_rows_from_joints(edit_joints, mean, std, dim_pose, device, to_motion)
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

    def window_rows(idx, T):
        rows = {}
        for name, values in per.items():
            if values[idx[0]] is None:
                continue
            for i in idx:
                if name != "edit_mask" and tuple(torch.as_tensor(values[i]).shape) != (plans[i][3], dim_pose):
                    raise ValueError(f"{name} of motion {i} must be {(plans[i][3], dim_pose)}")
            rows[name] = gather_canvases(values, plans, idx, T, dim_pose, name).to(device)
        return rows

    return window_rows


def split_long(caption: str, total_frames: int, window: int, overlap: int) -> List[Tuple[str, int]]:
    """A script for one caption over ``total_frames`` canvas frames: the fewest windows of at most ``window`` frames that
    cover it with ``overlap`` shared frames between neighbours, lengths as even as possible (the longer ones first)."""
    total, window, h = _int(total_frames, "total_frames"), _int(window, "window"), _int(overlap, "overlap")
    if total < 1:
        raise ValueError(f"total_frames must be >= 1, not {total}")
    if window < 1 or h < 0 or 2 * h > window:
        raise ValueError(f"need window >= 1 and 0 <= overlap <= window / 2, not window {window}, overlap {h}")
    n = 1 if total <= window else math.ceil((total - h) / (window - h))
    size, extra = divmod(total + (n - 1) * h, n)
    lengths = [size + (1 if i < extra else 0) for i in range(n)]
    plan_windows(lengths, h, window)  # the shortest window must still hold two overlaps
    return [(caption, n_) for n_ in lengths]


def _span(starts, lengths):
    """Checked windows (starts, lengths) that tile a canvas from frame 0 without gaps, and its length."""
    starts, lengths = [int(s) for s in starts], [int(n) for n in lengths]
    if len(starts) != len(lengths) or not starts:
        raise ValueError(f"{len(starts)} starts for {len(lengths)} windows")
    if starts[0] != 0 or min(lengths) < 1 or any(not starts[i] < starts[i + 1] <= starts[i] + lengths[i]
                                                 for i in range(len(starts) - 1)):
        raise ValueError(f"windows at {starts} of {lengths} frames do not tile a canvas from frame 0")
    return starts, lengths, starts[-1] + lengths[-1]


def canvas_to_windows(canvas: torch.Tensor, starts, lengths, T: int) -> torch.Tensor:
    """Gather a canvas (C, ...) into the window layout (n, T, ...); frames past each window's length are zero."""
    starts, lengths, C = _span(starts, lengths)
    canvas = torch.as_tensor(canvas)
    if canvas.dim() < 1 or canvas.shape[0] != C:
        raise ValueError(f"the canvas has {canvas.shape[0] if canvas.dim() else 0} frames, the windows cover {C}")
    if max(lengths) > T:
        raise ValueError(f"T = {T} is shorter than the longest window ({max(lengths)} frames)")
    out = canvas.new_zeros((len(starts), T) + tuple(canvas.shape[1:]))
    for i, (s, n) in enumerate(zip(starts, lengths)):
        out[i, :n] = canvas[s:s + n]
    return out


def windows_to_canvas(windows: torch.Tensor, starts, lengths) -> torch.Tensor:
    """Scatter windows (n, T, ...) onto their canvas (C, ...): each canvas frame taken from the first window covering it
    (the owner; after a handshake sampler its right neighbour holds the same bits there)."""
    starts, lengths, C = _span(starts, lengths)
    if windows.dim() < 2 or windows.shape[0] != len(starts) or windows.shape[1] < max(lengths):
        raise ValueError(f"windows of shape {tuple(windows.shape)} do not hold {len(starts)} windows of up to "
                         f"{max(lengths)} frames")
    out = windows.new_empty((C,) + tuple(windows.shape[2:]))
    for i in reversed(range(len(starts))):
        out[starts[i]:starts[i] + lengths[i]] = windows[i, :lengths[i]]
    return out

"""Joint-position control (``DDPMTrainer.generate(..., control_joints=, control_weights=)``).

Units: targets are joint positions in the units and frame of ``recover_from_ric`` applied to DE-normalised features
(``x * std + mean``), without the temporal filter: metres in HumanML3D, Y up, the motion starting at the origin of the
XZ plane with heading 0.  A target array is (T, J, 3) per sample, (x, y, z) per joint, joints in the skeleton's order
(``motion_edit.SMPL_JOINTS`` for the 22-joint skeleton; joint 0 is the pelvis).  Weights have the same shape, are >= 0,
and select what is steered: 0 ignores the entry (its target is then never read into the loss).

For sample b the guidance minimises L_b = sum_{t < len_b, j, c} W (P - G)^2 with P = recover_from_ric(x0 * std + mean),
moving the clean-motion estimate x0 of every sampler step down its gradient.  Only the root columns (0-3) and the ric
columns (4 .. 3J) enter recover_from_ric, so only they are steered; rot6d, velocity and contact columns are left to the
denoiser.  J follows from the feature width F = 12J - 1 (263 -> 22, 251 -> 21).

``root_path_targets`` and ``keyframe_targets`` are host helpers returning float32 CPU tensors; ``joint_loss_grad`` runs
the loss and its gradient on the device (``mdm_joint_loss_grad``).

Over a long motion (``DDPMTrainer.generate_long(..., control_joints=, control_weights=)``) the same loss
runs over the whole canvas: targets are (canvas_len, J, 3) per motion, frame 0 of the canvas at the origin, and
``canvas_loss_grad`` evaluates it on rows a table names (``mdm_canvas_joint_loss_grad``)."""
from __future__ import annotations

from typing import Iterable, Sequence

import numpy as np
import torch

from . import _lib as L

LDS_BYTES = 64 * 1024  # what csrc/motion_control.hip keeps per sample: see max_frames


def joints_for_feats(F: int) -> int:
    """J for a feature width F = 12 J - 1; ValueError for any other F."""
    F = int(F)
    if F < 11 or (F + 1) % 12:
        raise ValueError(f"feature width {F} is not of the form 12 J - 1 (263 for 22 joints, 251 for 21)")
    return (F + 1) // 12


def steerable_columns(F: int) -> int:
    """Number of leading feature columns joint control can move: root 4 + ric 3 (J - 1) = 3 J + 1."""
    return 3 * joints_for_feats(F) + 1


def max_frames(F: int) -> int:
    """Longest T the control kernels take at feature width F: the steerable columns of one sample, two rows of std /
    mean and 48 bytes of per-frame state fit 64 KiB of LDS (205 frames at F = 263, 211 at 251).  Equals
    ``mdm_joint_control_max_frames``."""
    ds = steerable_columns(F) | 1
    return (LDS_BYTES - 2 * ds * 4) // (ds * 4 + 48)


def root_path_targets(T: int, waypoints, frames: Sequence[int], joints_num: int = 22):
    """A pelvis path on the ground plane: ``waypoints`` (K, 2) XZ positions reached at ``frames`` (K increasing ints in
    [0, T)), linearly interpolated in between.  Returns (targets, weights), each (T, joints_num, 3) float32: weight 1 on
    joint 0's X and Z at frames[0] .. frames[-1], 0 everywhere else (height, the other joints and the frames outside the
    path are left free).  T is any frame count: a window's, or the canvas length of a long motion."""
    wp = torch.as_tensor(np.asarray(waypoints, dtype=np.float32))
    fr = [int(f) for f in frames]
    if wp.dim() != 2 or wp.shape[1] != 2 or wp.shape[0] != len(fr) or not fr:
        raise ValueError(f"waypoints of shape {tuple(wp.shape)} must be (K, 2) with one frame each ({len(fr)} frames)")
    if not bool(torch.isfinite(wp).all()):
        raise ValueError("waypoints has non-finite values")
    if fr[0] < 0 or fr[-1] >= T or any(b <= a for a, b in zip(fr, fr[1:])):
        raise ValueError(f"frames must be strictly increasing in [0, {T})")
    tg = torch.zeros(T, joints_num, 3)
    w = torch.zeros(T, joints_num, 3)
    t = torch.arange(fr[0], fr[-1] + 1, dtype=torch.float64)
    f64 = torch.tensor(fr, dtype=torch.float64)
    for k, c in ((0, 0), (1, 2)):
        v = torch.from_numpy(np.interp(t.numpy(), f64.numpy(), wp[:, k].double().numpy())).float()
        tg[fr[0]:fr[-1] + 1, 0, c] = v
        w[fr[0]:fr[-1] + 1, 0, c] = 1.0
    return tg, w


def keyframe_targets(joints_xyz, frames: Iterable[int], joints: Iterable[int]):
    """Positions of ``joints`` at ``frames`` taken from ``joints_xyz`` (T, J, 3), e.g. ``recover_from_ric`` of another
    motion or hand-placed points.  Returns (targets, weights), each (T, J, 3) float32: the targets are ``joints_xyz``
    itself and the weights are 1 on every coordinate of the chosen (frame, joint) pairs, 0 elsewhere.  T is any frame
    count: a window's, or the canvas length of a long motion."""
    g = torch.as_tensor(joints_xyz).detach().to("cpu", torch.float32)
    if g.dim() != 3 or g.shape[2] != 3:
        raise ValueError(f"joints_xyz of shape {tuple(g.shape)} must be (T, J, 3)")
    T, J = g.shape[0], g.shape[1]
    fr, js = [int(f) for f in frames], [int(j) for j in joints]
    if not fr or not js:
        raise ValueError("give at least one frame and one joint")
    if any(not 0 <= f < T for f in fr) or any(not 0 <= j < J for j in js):
        raise ValueError(f"frames must lie in [0, {T}) and joints in [0, {J})")
    w = torch.zeros(T, J, 3)
    w[torch.tensor(fr)[:, None], torch.tensor(js)[None, :]] = 1.0
    sel = w > 0
    if not bool(torch.isfinite(g[sel]).all()):
        raise ValueError("joints_xyz has non-finite values at the chosen frames and joints")
    return g.clone().contiguous(), w


def _rows(v, B: int, F: int, name: str) -> torch.Tensor:
    t = torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v).to(torch.float32)
    if t.dim() == 1:
        t = t[None].expand(B, -1)
    if tuple(t.shape) != (B, F):
        raise ValueError(f"{name} must be ({F},) or ({B}, {F}), not {tuple(t.shape)}")
    return t


@torch.no_grad()
def joint_loss_grad(x0: torch.Tensor, lengths, mean, std, targets, weights):
    """Loss (B,) and gradient (B, T, F) of the weighted squared joint-position distance (module docstring) with respect
    to the normalised features ``x0`` (B, T, F) on a GPU, through ``mdm_joint_loss_grad``.  ``mean`` / ``std``: (F,) or
    (B, F); ``targets`` (B, T, J, 3); ``weights`` broadcastable to it.  The gradient is exactly 0 in every column past
    3 J and in every frame at or past ``lengths[b]``."""
    L.require_cuda(x0)
    dev = x0.device
    x = x0.detach().to(torch.float32).contiguous()
    if x.dim() != 3:
        raise ValueError(f"x0 of shape {tuple(x.shape)} must be (B, T, F)")
    B, T, F = x.shape
    J = joints_for_feats(F)
    if not 1 <= T <= max_frames(F):
        raise ValueError(f"T = {T}: the control kernels take 1 to {max_frames(F)} frames at F = {F}")
    tg = torch.as_tensor(targets).to(dev, torch.float32)
    if tuple(tg.shape) != (B, T, J, 3):
        raise ValueError(f"targets of shape {tuple(tg.shape)} must be {(B, T, J, 3)}")
    w = torch.broadcast_to(torch.as_tensor(weights).to(dev, torch.float32), (B, T, J, 3)).contiguous()
    tg = tg.contiguous()
    mean_t = _rows(mean, B, F, "mean").to(dev).contiguous()
    std_t = _rows(std, B, F, "std").to(dev).contiguous()
    ln = torch.as_tensor(lengths).to(dev, torch.int32).contiguous()
    if tuple(ln.shape) != (B,):
        raise ValueError(f"lengths must hold {B} entries")
    loss = torch.empty(B, device=dev)
    grad = torch.empty_like(x)
    with torch.cuda.device(dev):
        L.check(L.lib().mdm_joint_loss_grad(
            x.data_ptr(), ln.data_ptr(), mean_t.data_ptr(), std_t.data_ptr(), tg.data_ptr(), w.data_ptr(), B, T, F, loss.data_ptr(),
            grad.data_ptr(), L.stream_ptr()), "mdm_joint_loss_grad")
    return loss, grad


@torch.no_grad()
def canvas_loss_grad(rows: torch.Tensor, motion_offsets, frame_rows, mean, std, targets, weights):
    """Loss (M,) and gradient (total, F), dense in canvas order, of the weighted squared joint-position distance over the
    canvases of M long motions on a GPU, through ``mdm_canvas_joint_loss_grad``.  ``rows`` (R, F), or any
    (..., F) tensor flattened to it: normalised feature rows; canvas frame c of motion m, c in ``[motion_offsets[m],
    motion_offsets[m + 1])``, is row ``frame_rows[c]``.  ``mean`` / ``std``: (F,) or (M, F); ``targets`` (total, J, 3) in
    canvas order; ``weights`` broadcastable to it.  Any canvas length.  The gradient is exactly 0 in every column past 3 J.
    Raises ValueError for offsets that do not rise from 0 to total and for rows out of range or repeated."""
    L.require_cuda(rows)
    dev = rows.device
    x = rows.detach().to(torch.float32).contiguous()
    F = x.shape[-1]
    x = x.reshape(-1, F)
    J = joints_for_feats(F)
    off = torch.as_tensor(motion_offsets).flatten().to(torch.int64).cpu()
    fr = torch.as_tensor(frame_rows).flatten().to(torch.int64).cpu()
    M, total = off.numel() - 1, fr.numel()
    if M < 0 or int(off[0]) != 0 or int(off[-1]) != total or bool((off[1:] < off[:-1]).any()):
        raise ValueError(f"motion_offsets must rise from 0 to the number of frame rows {total}")
    if total and (int(fr.min()) < 0 or int(fr.max()) >= x.shape[0] or torch.unique(fr).numel() != total):
        raise ValueError(f"frame_rows must be distinct rows in [0, {x.shape[0]})")
    tg = torch.as_tensor(targets).to(dev, torch.float32)
    if tuple(tg.shape) != (total, J, 3):
        raise ValueError(f"targets of shape {tuple(tg.shape)} must be {(total, J, 3)}")
    w = torch.broadcast_to(torch.as_tensor(weights).to(dev, torch.float32), (total, J, 3)).contiguous()
    tg = tg.contiguous()
    mean_t = _rows(mean, M, F, "mean").to(dev).contiguous()
    std_t = _rows(std, M, F, "std").to(dev).contiguous()
    off_d, fr_d = off.to(dev, torch.int32), fr.to(dev, torch.int32)
    loss = torch.zeros(M, device=dev)
    grad = torch.zeros((total, F), device=dev)
    ws = torch.empty(max(int(L.lib().mdm_canvas_control_workspace_floats(total, F)), 1), device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().mdm_canvas_joint_loss_grad(
            x.data_ptr(), off_d.data_ptr(), fr_d.data_ptr(), mean_t.data_ptr(), std_t.data_ptr(), tg.data_ptr(), w.data_ptr(), M, F,
            loss.data_ptr(), grad.data_ptr(), ws.data_ptr(), L.stream_ptr()), "mdm_canvas_joint_loss_grad")
    return loss, grad

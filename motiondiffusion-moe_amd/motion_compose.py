"""Weight maps for composed multi-prompt guidance (``DDPMTrainer.generate(..., prompt_weights=)``).

Pure host helpers: each returns a float32 CPU tensor whose leading dim is the prompt index k, to be given per sample as
``prompt_weights`` of shape (N, K, T, F) or anything broadcastable to it (``w[None]`` applies one map to every sample).
On every step the guided x0 is ``x0_u + s * sum_k w_k (x0_k - x0_u)``: weights that sum to 1 over k split the guidance
between prompts, and a negative weight is a negative prompt.

Maps combine by products: with ``tl = timeline_weights(T, [100])`` and ``bp = body_part_weights([UPPER_BODY,
LOWER_BODY])``, ``torch.stack([tl[0] * bp[0], tl[1] * bp[0], bp[1].expand(T, -1)])`` has the upper body follow prompt 0
for frames 0-99 and prompt 1 afterwards, and the lower body follow prompt 2 throughout (again a partition of unity).
"""
from __future__ import annotations

from typing import Iterable, Sequence

import torch

from .motion_edit import feature_dim, joint_columns


def timeline_weights(T: int, bounds: Sequence[int], blend: int = 0) -> torch.Tensor:
    """(K, T, 1) time-varied weights of K = len(bounds) + 1 prompts: prompt k owns frames [bounds[k-1], bounds[k]).
    ``blend`` > 0 replaces each hard switch by a linear crossfade over ``blend`` frames centred on the boundary (between
    frames b - 1 and b): the next prompt's share at frame f is clamp((f - b + 1/2) / blend + 1/2, 0, 1).  The weights are
    non-negative and sum to 1 at every frame."""
    T, blend = int(T), int(blend)
    b = [int(v) for v in bounds]
    if T < 1:
        raise ValueError(f"T = {T} frames")
    if blend < 0:
        raise ValueError(f"blend of {blend} frames")
    if any(not 0 < v < T for v in b) or any(v1 <= v0 for v0, v1 in zip(b, b[1:])):
        raise ValueError(f"bounds {b} must be strictly increasing frame indices in [1, {T - 1}]")
    f = torch.arange(T, dtype=torch.float64)
    ramps = [(f >= v).double() if blend == 0 else ((f - v + 0.5) / blend + 0.5).clamp(0.0, 1.0) for v in b]
    ones = torch.ones(T, dtype=torch.float64)
    edges = [ones] + ramps + [torch.zeros(T, dtype=torch.float64)]  # share of prompts >= k, non-increasing in k
    w = torch.stack([edges[k] - edges[k + 1] for k in range(len(b) + 1)])
    return w.to(torch.float32)[:, :, None]


def body_part_weights(parts: Sequence[Iterable[int]], joints_num: int = 22) -> torch.Tensor:
    """(K, F) body-part weights of K prompts: prompt k owns the feature columns of the joints in ``parts[k]``
    (``motion_edit.joint_columns``), so every column has weight 1 for exactly one prompt.  Every joint must be in
    exactly one part."""
    parts = [[int(j) for j in p] for p in parts]
    if not parts:
        raise ValueError("no parts")
    owner = {}
    for k, p in enumerate(parts):
        for j in p:
            if not 0 <= j < joints_num:
                raise ValueError(f"joint {j} outside [0, {joints_num})")
            if j in owner:
                raise ValueError(f"joint {j} is in parts {owner[j]} and {k}")
            owner[j] = k
    missing = [j for j in range(joints_num) if j not in owner]
    if missing:
        raise ValueError(f"joints {missing} are in no part")
    w = torch.zeros((len(parts), feature_dim(joints_num)), dtype=torch.float32)
    for j, k in owner.items():
        w[k, joint_columns(j, joints_num)] = 1.0
    return w

"""CPU: joint-position control host logic.

* the target helpers (root path, keyframes): shapes, values, weights;
* every ValueError of check_control_kwargs and of the trainer's control arguments; dist.shard_kwargs of control kwargs;
* the fp64 autograd restatement of the loss through oracle/motion_ref.recover_from_ric, checked against central finite
  differences: the reference tests/test_motion_control_gpu.py holds the kernels against.
"""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, pkg

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import motion_ref  # noqa: E402


@contextlib.contextmanager
def _f64():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)  # motion_ref allocates its quaternions and root positions at the default dtype
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def ref_positions(x, mean, std):
    """P = recover_from_ric(x * std + mean) in fp64 (differentiable), x (T, F) normalised, mean / std (F,)."""
    F = x.shape[-1]
    J = (F + 1) // 12
    with _f64():
        return motion_ref.recover_from_ric(x.double() * std.double() + mean.double(), J)


def ref_loss_grad(x0, lengths, mean, std, targets, weights):
    """fp64 loss (B,) and gradient (B, T, F) of sum_{t < len, j, c} W (P - G)^2 with respect to the normalised x0.
    mean / std (F,) or (B, F); weights broadcastable to targets (B, T, J, 3)."""
    x0 = torch.as_tensor(x0).detach().double().cpu()
    B, T, F = x0.shape
    mean = torch.as_tensor(mean).double().cpu().reshape(-1, F).expand(B, F)
    std = torch.as_tensor(std).double().cpu().reshape(-1, F).expand(B, F)
    G = torch.as_tensor(targets).double().cpu()
    W = torch.broadcast_to(torch.as_tensor(weights).double().cpu(), G.shape)
    losses, grads = [], []
    for b in range(B):
        n = max(0, min(int(lengths[b]), T))
        x = x0[b].clone().requires_grad_(True)
        if n == 0:
            losses.append(torch.zeros((), dtype=torch.float64))
            grads.append(torch.zeros(T, F, dtype=torch.float64))
            continue
        P = ref_positions(x[:n], mean[b], std[b])
        w = W[b, :n]
        d = torch.where(w != 0, P - G[b, :n], torch.zeros_like(P))
        loss = (w * d * d).sum()
        loss.backward()
        losses.append(loss.detach())
        grads.append(x.grad.detach().clone())
    return torch.stack(losses), torch.stack(grads)


def _case(T=6, F=263, seed=0):
    g = torch.Generator().manual_seed(seed)
    J = (F + 1) // 12
    x = torch.randn(1, T, F, generator=g, dtype=torch.float64) * 0.5
    mean = torch.randn(F, generator=g, dtype=torch.float64) * 0.1
    std = torch.rand(F, generator=g, dtype=torch.float64) + 0.5
    G = torch.randn(1, T, J, 3, generator=g, dtype=torch.float64)
    W = torch.rand(1, T, J, 3, generator=g, dtype=torch.float64)
    return x, mean, std, G, W


# ---- the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [263, 251])
def test_reference_gradient_matches_finite_differences(F):
    T = 6
    x, mean, std, G, W = _case(T, F, seed=F)
    _, grad = ref_loss_grad(x, [T - 1], mean, std, G, W)
    D = 3 * ((F + 1) // 12) + 1
    assert torch.equal(grad[0, :, D:], torch.zeros(T, F - D, dtype=torch.float64))
    assert torch.equal(grad[0, T - 1], torch.zeros(F, dtype=torch.float64))  # past the length
    h = 1e-6
    rng = np.random.RandomState(1)
    picks = [(t, c) for t in range(T - 1) for c in (0, 1, 2, 3)] + [(int(rng.randint(T - 1)), int(rng.randint(4, D)))
                                                                     for _ in range(12)]
    for t, c in picks:
        xp, xm = x.clone(), x.clone()
        xp[0, t, c] += h
        xm[0, t, c] -= h
        lp, _ = ref_loss_grad(xp, [T - 1], mean, std, G, W)
        lm, _ = ref_loss_grad(xm, [T - 1], mean, std, G, W)
        fd = float((lp - lm) / (2 * h))
        assert abs(fd - float(grad[0, t, c])) <= 1e-6 * max(1.0, abs(fd)), (t, c, fd, float(grad[0, t, c]))


def test_reference_positions_equal_the_oracle_in_f32_layout():
    x, mean, std, _, _ = _case(8)
    P = ref_positions(x[0], mean, std)
    want = motion_ref.recover_from_ric((x[0] * std + mean).float(), 22).double()
    assert (P - want).abs().max() < 1e-4


# ---- helpers ------------------------------------------------------------------------------------------------------------
def test_root_path_targets():
    M = pkg("motion_control")
    tg, w = M.root_path_targets(20, [[0.0, 0.0], [2.0, 1.0], [2.0, 3.0]], [2, 10, 18])
    assert tg.shape == (20, 22, 3) and w.shape == (20, 22, 3) and tg.dtype == torch.float32
    assert torch.equal(w[2:19, 0, 0], torch.ones(17)) and torch.equal(w[2:19, 0, 2], torch.ones(17))
    assert float(w.sum()) == 34.0  # joint 0's X and Z on frames 2..18 only
    assert float(w[:, 0, 1].sum()) == 0.0 and float(w[:2].sum()) == 0.0 and float(w[19:].sum()) == 0.0
    assert torch.allclose(tg[[2, 6, 10, 14, 18], 0, 0], torch.tensor([0.0, 1.0, 2.0, 2.0, 2.0]))
    assert torch.allclose(tg[[2, 6, 10, 14, 18], 0, 2], torch.tensor([0.0, 0.5, 1.0, 2.0, 3.0]))
    assert float(tg[:, 1:].abs().sum()) == 0.0
    tg21, _ = M.root_path_targets(8, [[0, 0], [1, 1]], [0, 7], joints_num=21)
    assert tg21.shape == (8, 21, 3)
    for bad in (dict(waypoints=[[0, 0]], frames=[0, 1]), dict(waypoints=[[0, 0], [1, 1]], frames=[3, 3]),
                dict(waypoints=[[0, 0], [1, 1]], frames=[0, 20]), dict(waypoints=[[0, 0, 0]], frames=[0]),
                dict(waypoints=[[0, float("nan")]], frames=[0])):
        with pytest.raises(ValueError):
            M.root_path_targets(20, **bad)


def test_keyframe_targets():
    M = pkg("motion_control")
    g = torch.randn(30, 22, 3)
    tg, w = M.keyframe_targets(g, [0, 29], [20, 21])
    assert torch.equal(tg, g) and tg is not g
    assert float(w.sum()) == 2 * 2 * 3
    assert torch.equal(w[29, 21], torch.ones(3)) and torch.equal(w[0, 20], torch.ones(3)) and float(w[5].sum()) == 0
    for bad in (([30], [0]), ([0], [22]), ([], [0]), ([0], [])):
        with pytest.raises(ValueError):
            M.keyframe_targets(g, *bad)
    with pytest.raises(ValueError):
        M.keyframe_targets(torch.zeros(4, 22), [0], [0])


def test_feature_layout_and_frame_limit():
    M = pkg("motion_control")
    assert M.joints_for_feats(263) == 22 and M.joints_for_feats(251) == 21
    assert M.steerable_columns(263) == 67 and M.steerable_columns(251) == 64
    assert M.max_frames(263) == 205 and M.max_frames(251) == 211
    for F in (262, 264, 0, 10):
        with pytest.raises(ValueError):
            M.joints_for_feats(F)


# ---- check_control_kwargs -----------------------------------------------------------------------------------------------
def _kw(B=2, T=8, F=263):
    J = (F + 1) // 12
    return {"control_joints": torch.zeros(B, T, J, 3), "control_weights": torch.ones(B, T),
            "control_mean": torch.zeros(B, F), "control_std": torch.ones(B, F), "control_scale": 0.5, "control_iters": 3}


def test_check_control_kwargs_accepts_and_broadcasts():
    D = pkg("diffusion")
    assert D.check_control_kwargs({}, (2, 8, 263)) is None
    c = D.check_control_kwargs(_kw(), (2, 8, 263))
    assert c["weights"].shape == (2, 8, 22, 3) and c["scale"] == 0.5 and c["iters"] == 3
    kw = _kw()
    del kw["control_scale"], kw["control_iters"]
    c = D.check_control_kwargs(kw, (2, 8, 263))
    assert c["scale"] == 1.0 and c["iters"] == 1
    for w in (torch.ones(2), torch.ones(2, 8, 22), torch.ones(2, 1, 22, 3), torch.ones(2, 8, 22, 3)):
        assert D.check_control_kwargs(dict(_kw(), control_weights=w), (2, 8, 263))["weights"].shape == (2, 8, 22, 3)
    assert D.check_control_kwargs(_kw(F=251), (2, 8, 251))["targets"].shape == (2, 8, 21, 3)


@pytest.mark.parametrize("change", [
    dict(control_joints=None), dict(control_weights=None), dict(control_mean=None), dict(control_std=None),
    dict(control_joints=torch.zeros(2, 8, 21, 3)), dict(control_joints=torch.zeros(2, 7, 22, 3)),
    dict(control_joints=torch.zeros(2, 8, 22, 3, dtype=torch.int64)),
    dict(control_weights=torch.ones(8)), dict(control_weights=torch.ones(2, 8, 5)), dict(control_weights=-torch.ones(2)),
    dict(control_weights=torch.full((2,), float("nan"))), dict(control_weights=torch.full((2,), float("inf"))),
    dict(control_joints=torch.full((2, 8, 22, 3), float("nan"))),
    dict(control_mean=torch.zeros(263)), dict(control_std=torch.ones(263)), dict(control_std=torch.zeros(2, 263)),
    dict(control_mean=torch.full((2, 263), float("inf"))),
    dict(control_scale=float("nan")), dict(control_scale=float("inf")),
    dict(control_iters=0), dict(control_iters=33), dict(control_iters=1.5), dict(control_iters=True),
])
def test_check_control_kwargs_errors(change):
    D = pkg("diffusion")
    kw = {k: v for k, v in dict(_kw(), **change).items() if v is not None}
    with pytest.raises(ValueError):
        D.check_control_kwargs(kw, (2, 8, 263))


def test_check_control_kwargs_shape_errors():
    D = pkg("diffusion")
    with pytest.raises(ValueError):  # scale / iters alone
        D.check_control_kwargs({"control_scale": 1.0}, (2, 8, 263))
    with pytest.raises(ValueError):  # F not 12 J - 1
        D.check_control_kwargs(dict(_kw(F=263), control_mean=torch.zeros(2, 262), control_std=torch.ones(2, 262)),
                               (2, 8, 262))
    with pytest.raises(ValueError):  # T over the LDS limit
        D.check_control_kwargs(dict(_kw(T=206)), (2, 206, 263))
    assert D.check_control_kwargs(_kw(T=205), (2, 205, 263)) is not None


def test_shard_kwargs_gives_each_rank_its_rows():
    Dist = pkg("dist")
    kw = _kw(B=5)
    kw["control_joints"] = torch.arange(5 * 8 * 22 * 3, dtype=torch.float32).reshape(5, 8, 22, 3)
    kw["control_mean"] = torch.arange(5 * 263, dtype=torch.float32).reshape(5, 263)
    kw["control_weights"] = torch.arange(5, dtype=torch.float32)
    for lo, hi in ((0, 3), (3, 5)):
        s = Dist.shard_kwargs(kw, lo, hi)
        for k in ("control_joints", "control_weights", "control_mean", "control_std"):
            assert torch.equal(s[k], kw[k][lo:hi]), k
        assert s["control_scale"] == 0.5 and s["control_iters"] == 3
        assert pkg("diffusion").check_control_kwargs(s, (hi - lo, 8, 263))["targets"].shape[0] == hi - lo


# ---- trainer arguments --------------------------------------------------------------------------------------------------
def test_trainer_control_arguments():
    Cond = pkg("conditioning").Conditioning
    caps = ["a", "b", "c"]
    g = torch.zeros(3, 10, 22, 3)
    mean, std = np.zeros(263, np.float32), np.ones(263, np.float32)

    def ctl(g, w, mean, std, dim_pose=263, **kw):
        return Cond(caps, dim_pose, control_joints=g, control_weights=w, mean=mean, std=std, **kw)

    assert ctl(None, None, None, None).control is None
    assert ctl(None, None, mean, std).control is None and ctl(None, None, mean, std).control_kwargs(slice(0, 3), 6, "cpu") == {}
    c = ctl(g, torch.ones(3, 10), mean, std).control
    assert c["weights"].shape == (3, 10, 22, 3) and c["mean"].shape == (263,)
    kw = ctl(g, torch.ones(3, 10), mean, std, control_scale=2.0, control_iters=4).control_kwargs(slice(1, 3), 6, "cpu")
    assert kw["control_joints"].shape == (2, 6, 22, 3) and kw["control_weights"].shape == (2, 6, 22, 3)
    assert kw["control_mean"].shape == (2, 263) and kw["control_scale"] == 2.0 and kw["control_iters"] == 4
    kw = ctl(g, torch.ones(3, 10), mean, std).kwargs(torch.tensor([2, 0]), 10, "cpu")
    assert kw["control_joints"].shape == (2, 10, 22, 3) and kw["control_scale"] == 1.0 and kw["control_iters"] == 1
    with pytest.raises(ValueError):
        ctl(g, torch.ones(3, 10), mean, std).control_kwargs(slice(0, 3), 11, "cpu")
    for args in ((g, None, mean, std), (None, torch.ones(3), mean, std), (g, torch.ones(3), None, std),
                 (g, torch.ones(3), mean, None), (torch.zeros(3, 10, 21, 3), torch.ones(3), mean, std),
                 (g, torch.ones(2), mean, std), (g, torch.ones(3, 10, 7), mean, std), (g, torch.ones(3), mean[:5], std)):
        with pytest.raises(ValueError):
            ctl(*args)
    with pytest.raises(ValueError):
        ctl(torch.zeros(3, 10, 22, 3), torch.ones(3), np.zeros(262), np.ones(262), 262)

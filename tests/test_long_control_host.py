"""CPU: joint-position control over a long motion's canvas, host logic.

* canvas_frame_rows: every canvas frame once, in its owner (left) window's row, in agreement with handshake_tables' owner
  entries and windows_to_canvas; batch_control_tables / canvas_control over a batch of motions;
* every ValueError of check_canvas_control_kwargs, the NotImplementedError kept for per-window control with handshakes;
* dist.shard_kwargs refuses the canvas tensors; generate_long's argument checks on a trainer built without a device.
"""
import types

import numpy as np
import pytest
import torch

from conftest import pkg


def _ml():
    return pkg("motion_long")


@pytest.mark.parametrize("lens,h,T,first", [([16, 12, 16], 4, 16, 0), ([16, 12, 16], 4, 18, 5), ([10], 3, 12, 2),
                                            ([6, 6, 6, 6], 3, 6, 1), ([8, 8], 0, 8, 0)])
def test_canvas_frame_rows_name_each_frames_owner(lens, h, T, first):
    ML = _ml()
    starts, C = ML.plan_windows(lens, h)
    rows = ML.canvas_frame_rows(starts, lens, T, first)
    assert rows.dtype == np.int32 and rows.shape == (C,) and len(set(rows.tolist())) == C
    # by definition: the first window that covers the frame
    for c in range(C):
        i = min(k for k in range(len(lens)) if starts[k] <= c < starts[k] + lens[k])
        assert rows[c] == (first + i) * T + c - starts[i], c
    # the owner entries of the handshake tables are among them; the copies are not
    tab = ML.handshake_tables(starts, lens, T, h, first_row=first)
    own = tab["owner_rows"].reshape(-1, 2)
    assert set(own[:, 0].tolist()) <= set(rows.tolist()) and not set(own[:, 1].tolist()) & set(rows.tolist())
    # and gathering those rows of the window layout is windows_to_canvas
    win = torch.randn(first + len(lens), T, 5)
    assert torch.equal(win.reshape(-1, 5)[torch.from_numpy(rows).long()], ML.windows_to_canvas(win[first:], starts, lens))
    with pytest.raises(ValueError):
        ML.canvas_frame_rows(starts, lens, max(lens) - 1, first)
    with pytest.raises(ValueError):
        ML.canvas_frame_rows(starts[:-1] if len(starts) > 1 else [], lens, T, first)


def _plans():
    return _ml().script_plans([[("a", 16), ("b", 12), ("c", 16)], [("d", 10)], [("e", 14), ("f", 16)]], 4, 16)


def _targets(plans, J=22):
    g = torch.Generator().manual_seed(0)
    return [torch.randn(p[3], J, 3, generator=g) for p in plans], [torch.rand(p[3], J, 3, generator=g) for p in plans]


def test_batch_control_tables_and_canvas_control():
    ML, D = _ml(), pkg("diffusion")
    plans = _plans()
    tg, w = _targets(plans)
    kw = ML.batch_control_tables(plans, [0, 2], 16, tg, w)
    assert kw["canvas_control_offsets"].tolist() == [0, 36, 62] and kw["canvas_control_offsets"].dtype == torch.int32
    rows = kw["canvas_control_rows"]
    assert rows.dtype == torch.int32 and rows[:36].tolist() == ML.canvas_frame_rows(plans[0][2], plans[0][1], 16).tolist()
    assert rows[36:].tolist() == ML.canvas_frame_rows(plans[2][2], plans[2][1], 16, first_row=3).tolist()
    assert torch.equal(kw["canvas_control_joints"], torch.cat([tg[0], tg[2]]))
    assert torch.equal(kw["canvas_control_weights"], torch.cat([w[0], w[2]]))
    mean, std = np.zeros(263, np.float32), np.ones(263, np.float32)
    tables = ML.canvas_control(plans, 263, tg, [w[0][:, :, 0], w[1][:, 0, 0], w[2]], 0.1, 3, mean, std)
    ckw = tables([0, 2], 16)
    assert ckw["control_scale"] == 0.1 and ckw["control_iters"] == 3 and tuple(ckw["canvas_control_mean"].shape) == (2, 263)
    assert torch.equal(ckw["canvas_control_weights"][:36], w[0][:, :, :1].expand(36, 22, 3))
    got = D.check_canvas_control_kwargs({**ckw, **ML.batch_tables(plans, [0, 2], 16, 4), "length": torch.tensor([16, 12, 16, 14, 16])},
                                        (5, 16, 263))
    assert got["M"] == 2 and got["total"] == 62 and got["iters"] == 3 and got["rows"].dtype == torch.int32
    assert "control_scale" not in ML.canvas_control(plans, 263, tg, w, None, None, mean, std)([1], 10)
    assert ML.canvas_control(plans, 263)([0], 16) == {}
    for args, msg in (((tg, None), "go together"), ((None, w), "go together"), ((tg[:2], w), "one entry per motion"),
                      ((tg, [w[0], None, w[2]]), "one entry per motion"), ((torch.zeros(3, 36, 22, 3), w), "one entry per motion"),
                      (([tg[0][:35], tg[1], tg[2]], w), r"control_joints of motion 0 has shape \(35, 22, 3\), its canvas \(36, 22, 3\)"),
                      (([t[:, :21] for t in tg], w), "control_joints of motion 0"),
                      ((tg, [w[0][:35], w[1], w[2]]), "control_weights of motion 0 has shape"),
                      ((tg, [w[0][None], w[1], w[2]]), "has more dims")):
        with pytest.raises(ValueError, match=msg):
            ML.canvas_control(plans, 263, *args, mean=mean, std=std)
    with pytest.raises(ValueError, match="mean and std"):
        ML.canvas_control(plans, 263, tg, w)
    with pytest.raises(ValueError, match="mean must have 263 entries"):
        ML.canvas_control(plans, 263, tg, w, mean=mean[:10], std=std)
    with pytest.raises(ValueError, match="without control_joints"):
        ML.canvas_control(plans, 263, control_scale=0.1)
    with pytest.raises(ValueError, match="12 J - 1"):
        ML.canvas_control(plans, 100, tg, w, mean=mean, std=std)


def _kw(single=False):
    """The model kwargs of one batch: motions 0 and 2 of _plans() (five windows), or a single-window motion without tables."""
    ML = _ml()
    plans = _plans()
    tg, w = _targets(plans)
    mean, std = np.zeros(263, np.float32), np.ones(263, np.float32)
    control = ML.canvas_control(plans, 263, tg, w, None, None, mean, std)
    if single:
        return {**control([1], 10), "length": torch.tensor([10])}, (1, 10, 263)
    return {**control([0, 2], 16), **ML.batch_tables(plans, [0, 2], 16, 4), "length": torch.tensor([16, 12, 16, 14, 16])}, (5, 16, 263)


def test_check_canvas_control_kwargs_errors():
    D = pkg("diffusion")
    kw, shape = _kw()
    assert D.check_canvas_control_kwargs({"length": kw["length"]}, shape) is None
    ok = D.check_canvas_control_kwargs(kw, shape)
    assert ok["scale"] == 1.0 and ok["iters"] == 1 and tuple(ok["weights"].shape) == (62, 22, 3)
    assert D.check_control_kwargs(dict(kw, control_scale=0.5, control_iters=2), shape) is None  # the scalars are the canvas form's
    one, shape1 = _kw(single=True)
    assert D.check_canvas_control_kwargs(one, shape1)["M"] == 1  # a single window needs no handshake tables

    def bad(msg, shape_=shape, **upd):
        with pytest.raises(ValueError, match=msg):
            D.check_canvas_control_kwargs(dict(kw, **upd), shape_)

    for k in ("canvas_control_offsets", "canvas_control_rows", "canvas_control_joints", "canvas_control_weights",
              "canvas_control_mean", "canvas_control_std"):
        bad(f"needs all of .*missing {k}", **{k: None})
    hs = {k: None for k in kw if k.startswith("handshake_")}
    bad("motion 0 spans several windows", **hs)
    off, rows = kw["canvas_control_offsets"], kw["canvas_control_rows"]
    bad("rise from 0", canvas_control_offsets=off + 1)
    bad("rise from 0", canvas_control_offsets=torch.tensor([0, 40, 36, 62]))
    bad("rise from 0", canvas_control_offsets=off[:-1])
    bad("1-D integer", canvas_control_offsets=off.float())
    bad("1-D integer", canvas_control_rows=rows[None])
    r = rows.clone()
    r[5] = 5 * 16
    bad(r"must lie in \[0, B \* T\)", canvas_control_rows=r)
    r = rows.clone()
    r[5] = -1
    bad(r"must lie in \[0, B \* T\)", canvas_control_rows=r)
    r = rows.clone()
    r[5] = r[4]
    bad("repeats a row", canvas_control_rows=r)
    r = rows.clone()
    r[35] = 16 + 13  # window 1 has 12 frames
    bad("at or past its window's length", canvas_control_rows=r)
    r = rows.clone()
    r[12] = 16  # the copy of canvas frame 12 in window 1, not its owner in window 0
    bad("names a copy of a shared frame", canvas_control_rows=r)
    bad("length must have 5 entries", length=torch.tensor([16, 12]))
    bad(r"canvas_control_joints has shape \(61, 22, 3\)", canvas_control_joints=kw["canvas_control_joints"][:61])
    bad(r"expected \(62, 22, 3\)", canvas_control_joints=kw["canvas_control_joints"][:, :21])
    bad("must lead with the row count 62", canvas_control_weights=torch.ones(61))
    bad("does not broadcast", canvas_control_weights=torch.ones(62, 5))
    bad("must be floating point", canvas_control_weights=torch.ones(62, dtype=torch.int64))
    bad(r"canvas_control_mean has shape \(1, 263\)", canvas_control_mean=kw["canvas_control_mean"][:1])
    bad(r"canvas_control_std has shape \(2, 262\)", canvas_control_std=kw["canvas_control_std"][:, :262])
    for name in ("canvas_control_joints", "canvas_control_weights", "canvas_control_mean", "canvas_control_std"):
        for v in (float("nan"), float("inf")):
            t = kw[name].clone()
            t.view(-1)[3] = v
            bad("non-finite", **{name: t})
    w = kw["canvas_control_weights"].clone()
    w[3, 2, 1] = -0.5
    bad("must be >= 0", canvas_control_weights=w)
    s = kw["canvas_control_std"].clone()
    s[1, 7] = 0
    bad("zero entries", canvas_control_std=s)
    bad("control_scale must be finite", control_scale=float("nan"))
    for it in (0, 33, 1.5, True):
        bad("control_iters must be an integer", control_iters=it)
    bad("exclusive", control_joints=torch.zeros(5, 16, 22, 3))
    bad("exclusive", control_std=torch.ones(5, 263))
    bad("composed prompts", compose_weights=torch.ones(5, 2))
    bad("composed prompts", compose_text=[["a", "b"]] * 5)
    bad("12 J - 1", shape_=(5, 16, 100))
    assert D.check_canvas_control_kwargs(dict(kw, canvas_control_weights=torch.ones(62)), shape) is not None  # per frame


def test_per_window_control_with_handshakes_is_still_not_implemented():
    D = pkg("diffusion")
    kw, shape = _kw()
    hs = {k: v for k, v in kw.items() if k.startswith("handshake_")}
    for extra in ({"control_joints": torch.zeros(5, 16, 22, 3)}, {"control_weights": torch.ones(5)},
                  {"control_mean": torch.zeros(5, 263)}, {"control_std": torch.ones(5, 263)}):
        with pytest.raises(NotImplementedError, match="canvas_control"):
            D.check_handshake_kwargs(dict(hs, **extra), shape)
    assert D.check_handshake_kwargs(kw, shape)["nshared"] == 12  # the canvas form passes


def test_shard_kwargs_refuses_the_canvas_tensors():
    dist = pkg("dist")
    kw, _ = _kw()
    for k in kw:
        if k.startswith("canvas_control_"):
            with pytest.raises(ValueError, match=f"{k} describes whole long motions"):
                dist.shard_kwargs({"length": kw["length"], k: kw[k]}, 0, 2)
    out = dist.shard_kwargs({"length": kw["length"], "canvas_control_rows": None, "control_scale": 0.5}, 1, 3)
    assert out["length"].tolist() == [12, 16] and out["control_scale"] == 0.5


def test_generate_long_control_argument_checks():
    Tr = pkg("trainer")
    tr = Tr.DDPMTrainer.__new__(Tr.DDPMTrainer)
    tr.encoder = types.SimpleNamespace(num_frames=16, eval=lambda: None)
    scripts = [[("a", 16), ("b", 12), ("c", 16)], [("d", 10)]]
    tg, w = [torch.zeros(36, 22, 3), torch.zeros(10, 22, 3)], [torch.ones(36), torch.ones(10)]
    mean, std = np.zeros(263, np.float32), np.ones(263, np.float32)

    def bad(msg, front=None, **kw):
        with pytest.raises(ValueError, match=msg):
            if front is None:
                tr.generate_long(scripts, 263, overlap=4, **kw)
            else:
                getattr(tr, front)(scripts, 263, mean, std, overlap=4, **kw)

    bad("go together", control_joints=tg, mean=mean, std=std)
    bad("go together", control_weights=w, mean=mean, std=std)
    bad("mean and std", control_joints=tg, control_weights=w)
    bad("one entry per motion", control_joints=tg[:1], control_weights=w, mean=mean, std=std)
    bad("one entry per motion", control_joints=[tg[0], None], control_weights=w, mean=mean, std=std)
    bad(r"control_joints of motion 1 has shape \(16, 22, 3\), its canvas \(10, 22, 3\)",
        control_joints=[tg[0], torch.zeros(16, 22, 3)], control_weights=w, mean=mean, std=std)
    bad("control_weights of motion 0 has shape", control_joints=tg, control_weights=[torch.ones(16), w[1]], mean=mean, std=std)
    bad("without control_joints", control_scale=0.1)
    bad("without control_joints", control_iters=2)
    # the front ends bring their own mean / std: what is left to fail is the canvas shape
    for front in ("generate_long_joints", "generate_long_bvh", "generate_long_gif"):
        bad("control_joints of motion 1 has shape", front, control_joints=[tg[0], torch.zeros(16, 22, 3)], control_weights=w)
        bad("go together", front, control_joints=tg)

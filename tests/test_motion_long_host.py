"""CPU: the host side of long-motion generation (motion_long, check_handshake_kwargs, the trainer's script checks).

Window starts and canvas lengths, coverage (every canvas frame once or twice), the blend weights (linear ramp values, sum 1
per shared frame) and owner tables, the canvas <-> windows round trip, every ValueError of bad scripts and tables, and the
NotImplementedError for composed prompts and joint control."""
import types

import numpy as np
import pytest
import torch

from conftest import pkg


def _ml():
    return pkg("motion_long")


def test_plan_windows_starts_and_canvas_length():
    ML = _ml()
    assert ML.plan_windows([16, 12, 16], 4) == ([0, 12, 20], 36)
    assert ML.plan_windows([196, 196, 196, 196], 20) == ([0, 176, 352, 528], 724)
    assert ML.plan_windows([10], 5) == ([0], 10)
    assert ML.plan_windows([8, 8], 0) == ([0, 8], 16)
    for lens, h in (([16, 12, 16], 4), ([40, 33, 50, 41], 16), ([9, 9, 9], 0), ([7, 6], 3)):
        starts, C = ML.plan_windows(lens, h)
        assert C == sum(lens) - (len(lens) - 1) * h
        cover = np.zeros(C, int)
        for s, n in zip(starts, lens):
            cover[s:s + n] += 1
        assert cover.min() == 1 and cover.max() <= 2, cover
        assert int((cover == 2).sum()) == (len(lens) - 1) * h


@pytest.mark.parametrize("blend", ["linear", "uniform"])
def test_tables_weights_and_owner(blend):
    ML = _ml()
    lens, h, T = [16, 12, 16], 4, 16
    starts, C = ML.plan_windows(lens, h)
    t = ML.handshake_tables(starts, lens, T, h, blend)
    assert t["offsets"].dtype == np.int32 and t["rows"].dtype == np.int32 and t["weights"].dtype == np.float32
    assert t["offsets"].tolist() == list(range(0, 2 * 8 + 1, 2))
    # shared frame c: (window i, frame len_i - h + j) then (window i + 1, frame j)
    want = []
    for i in range(2):
        for j in range(h):
            want += [i * T + lens[i] - h + j, (i + 1) * T + j]
    assert t["rows"].tolist() == want
    assert t["owner_rows"].tolist() == want  # the left window owns each overlap and comes first
    w = t["weights"].reshape(-1, 2).astype(np.float64)
    assert np.abs(w.sum(1) - 1).max() < 1e-7
    if blend == "linear":
        for c in range(8):
            j = c % h
            assert w[c, 1] == np.float32((j + 1) / (h + 1)) and w[c, 0] == np.float32(1 - (j + 1) / (h + 1)), c
    else:
        assert (w == 0.5).all()
    # the rows of every shared frame map to the same canvas frame
    for c in range(8):
        r = t["rows"][2 * c:2 * c + 2]
        assert len({starts[k // T] + k % T for k in r.tolist()}) == 1
    # several motions in one batch: rows shifted by each motion's first row, offsets continued
    t2 = ML.handshake_tables([0, 6], [8, 8], T, 2, blend, first_row=3)
    mt = ML.merge_tables([t, t2])
    assert mt["offsets"].tolist() == list(range(0, 2 * 10 + 1, 2))
    assert mt["rows"][16:].tolist() == [3 * T + 6, 4 * T + 0, 3 * T + 7, 4 * T + 1]
    empty = ML.handshake_tables([0], [10], 10, 0, blend)
    assert empty["offsets"].tolist() == [0] and empty["rows"].size == 0


def test_canvas_windows_round_trip():
    ML = _ml()
    lens, h, T = [16, 12, 16], 4, 16
    starts, C = ML.plan_windows(lens, h)
    canvas = torch.randn(C, 7, generator=torch.Generator().manual_seed(0))
    win = ML.canvas_to_windows(canvas, starts, lens, T)
    assert win.shape == (3, T, 7)
    assert torch.equal(win[1, 12:], torch.zeros(4, 7))  # padding past window 1's length
    for i, (s, n) in enumerate(zip(starts, lens)):
        assert torch.equal(win[i, :n], canvas[s:s + n])
    assert torch.equal(ML.windows_to_canvas(win, starts, lens), canvas)
    # the owner (left) window's values stand in an overlap
    win2 = win.clone()
    win2[1, :h] += 1
    assert torch.equal(ML.windows_to_canvas(win2, starts, lens), canvas)
    with pytest.raises(ValueError):
        ML.canvas_to_windows(canvas[:-1], starts, lens, T)
    with pytest.raises(ValueError):
        ML.canvas_to_windows(canvas, starts, lens, 15)
    with pytest.raises(ValueError):
        ML.windows_to_canvas(win[:2], starts, lens)
    with pytest.raises(ValueError):
        ML.windows_to_canvas(win, [0, 20, 30], lens)  # a gap between windows 0 and 1


def test_split_long():
    ML = _ml()
    assert ML.split_long("walk", 100, 196, 20) == [("walk", 100)]
    for total, window, h in ((600, 196, 20), (1000, 196, 20), (197, 196, 20), (36, 16, 4), (500, 120, 30)):
        sc = ML.split_long("walk", total, window, h)
        lens = [n for _, n in sc]
        assert all(c == "walk" for c, _ in sc)
        assert max(lens) <= window and max(lens) - min(lens) <= 1
        _, C = ML.plan_windows(lens, h, window)
        assert C == total, (total, lens)
        if len(lens) > 1:  # the fewest windows
            assert (len(lens) - 1) * window - (len(lens) - 2) * h < total
    for bad in ((0, 196, 20), (100, 0, 0), (100, 40, 21), (100, 40, -1)):
        with pytest.raises(ValueError):
            ML.split_long("walk", *bad)


def test_plan_and_table_errors():
    ML = _ml()
    with pytest.raises(ValueError):
        ML.plan_windows([], 0)
    with pytest.raises(ValueError):
        ML.plan_windows([16, 17], 2, max_len=16)  # a window longer than the model's num_frames
    with pytest.raises(ValueError):
        ML.plan_windows([16, 12], 7)  # above half the shortest window
    with pytest.raises(ValueError):
        ML.plan_windows([16, 12], -1)
    with pytest.raises(ValueError):
        ML.plan_windows([16, 0], 0)
    with pytest.raises(ValueError):
        ML.plan_windows([16, 2.5], 0)
    with pytest.raises(ValueError):
        ML.handshake_tables([0, 12], [16, 12], 16, 4, "cosine")
    with pytest.raises(ValueError):
        ML.handshake_tables([0, 11], [16, 12], 16, 4)  # starts that do not follow from the lengths
    with pytest.raises(ValueError):
        ML.handshake_tables([0, 12], [16, 12], 14, 4)  # T shorter than a window


def _kw(lens=(16, 12, 16), h=4, T=16):
    ML = _ml()
    starts, _ = ML.plan_windows(list(lens), h)
    t = ML.handshake_tables(starts, list(lens), T, h)
    return {"handshake_offsets": torch.from_numpy(t["offsets"]), "handshake_rows": torch.from_numpy(t["rows"]),
            "handshake_weights": torch.from_numpy(t["weights"]), "handshake_owner_rows": torch.from_numpy(t["owner_rows"])}


def test_check_handshake_kwargs():
    D = pkg("diffusion")
    shape = (3, 16, 263)
    assert D.check_handshake_kwargs({}, shape) is None
    kw = _kw()
    hs = D.check_handshake_kwargs(kw, shape)
    assert hs["nshared"] == 8 and hs["rows"].dtype == torch.int32 and hs["weights"].dtype == torch.float32
    assert D.check_handshake_kwargs(_kw(h=0), shape) is None  # no shared frame: nothing to run
    # owner rows may list a frame's rows in another order (another owner)
    own = kw["handshake_owner_rows"].clone().view(-1, 2).flip(1).reshape(-1)
    assert D.check_handshake_kwargs(dict(kw, handshake_owner_rows=own), shape) is not None

    def bad(**upd):
        with pytest.raises(ValueError):
            D.check_handshake_kwargs(dict(kw, **upd), shape)

    bad(handshake_weights=None)
    bad(handshake_offsets=kw["handshake_offsets"][None])                    # not 1-D
    bad(handshake_rows=kw["handshake_rows"].float())                         # not integer
    bad(handshake_weights=kw["handshake_weights"].int())                     # not floating point
    bad(handshake_offsets=kw["handshake_offsets"][:-1])                      # does not end at the entry count
    bad(handshake_offsets=kw["handshake_offsets"] + 1)                       # does not start at 0
    bad(handshake_weights=kw["handshake_weights"][:-1])                      # one weight short
    bad(handshake_owner_rows=kw["handshake_owner_rows"][:-1])
    bad(handshake_offsets=torch.tensor([0, 1, 16], dtype=torch.int32))       # a frame of one entry
    r = kw["handshake_rows"].clone()
    r[3] = 3 * 16
    bad(handshake_rows=r)                                                    # outside [0, B T)
    r = kw["handshake_rows"].clone()
    r[3] = r[0]
    bad(handshake_rows=r)                                                    # repeated
    own = kw["handshake_owner_rows"].clone()
    own[0], own[2] = own[2].clone(), own[0].clone()
    bad(handshake_owner_rows=own)                                            # rows moved between frames
    w = kw["handshake_weights"].clone()
    w[0] = float("nan")
    bad(handshake_weights=w)
    bad(handshake_weights=kw["handshake_weights"] * 2)                       # not a weighted mean
    with pytest.raises(ValueError):
        D.check_handshake_kwargs(_kw(), (2, 16, 263))                        # rows of a third window in a batch of two


def test_plan_batches_keeps_motions_whole_and_in_order():
    ML = _ml()
    plans = ML.script_plans([[("a", 16)] * 2, [("b", 16)] * 3, [("c", 16)], [("d", 16)] * 2, [("e", 12)] * 4], 4, 16)
    assert [len(p[1]) for p in plans] == [2, 3, 1, 2, 4] and plans[1][0] == ["b"] * 3 and plans[4][2:] == ([0, 8, 16, 24], 36)
    assert ML.plan_batches(plans, 4) == [[0], [1, 2], [3], [4]]      # a motion that does not fit starts the next batch
    assert ML.plan_batches(plans, 5) == [[0, 1], [2, 3], [4]]
    assert ML.plan_batches(plans, 6) == [[0, 1, 2], [3, 4]]
    assert ML.plan_batches(plans, 100) == [[0, 1, 2, 3, 4]]
    assert ML.plan_batches(plans[:1], 2) == [[0]]
    for bs in (4, 5, 6, 7, 12):  # every motion once, in order, never more windows than batch_size
        got = ML.plan_batches(plans, bs)
        assert [i for b in got for i in b] == [0, 1, 2, 3, 4]
        assert all(sum(len(plans[i][1]) for i in b) <= bs for b in got)
    with pytest.raises(ValueError, match="motion 4 has 4 windows, more than batch_size = 3"):
        ML.plan_batches(plans, 3)


def test_gather_canvases_against_canvas_to_windows():
    ML = _ml()
    plans = ML.script_plans([[("a", 6), ("b", 4)], [("c", 5)], [("d", 4), ("e", 4), ("f", 6)]], 2, 8)
    assert [p[3] for p in plans] == [8, 5, 10]
    canv = [torch.arange(8 * 3, dtype=torch.float64).view(8, 3), None, 100 + torch.arange(10 * 3, dtype=torch.float32).view(10, 3)]
    got = ML.gather_canvases(canv, plans, [2, 0], 6, 3, "noise")
    assert got.shape == (5, 6, 3) and got.dtype == torch.float32
    want = torch.cat([ML.canvas_to_windows(canv[2], [0, 2, 4], [4, 4, 6], 6), ML.canvas_to_windows(canv[0].float(), [0, 4], [6, 4], 6)])
    assert torch.equal(got, want)
    # by hand: window 1 of motion 2 is canvas frames 2..5, then padding; window 1 of motion 0 is canvas frames 4..7
    assert torch.equal(got[1, :4], canv[2][2:6]) and torch.equal(got[1, 4:], torch.zeros(2, 3))
    assert torch.equal(got[4, :4], canv[0][4:8].float()) and torch.equal(got[4, 4:], torch.zeros(2, 3))
    # values broadcast to the canvas: a (C, 1) frame mask, a (dim_pose,) feature mask
    fm = torch.tensor([1.0, 1.0, 0.0, 0.0, 0.0])[:, None]
    got = ML.gather_canvases([None, fm, None], plans, [1], 6, 3, "edit_mask")
    assert got.shape == (1, 6, 3) and got[0, :, 1].tolist() == [1.0, 1.0, 0.0, 0.0, 0.0, 0.0]
    assert torch.equal(ML.gather_canvases([None, torch.tensor([1.0, 0.0, 1.0]), None], plans, [1], 6, 3, "edit_mask")[0, :5],
                       torch.tensor([1.0, 0.0, 1.0]).expand(5, 3))
    with pytest.raises(ValueError, match=r"edit_mask of motion 1 has shape \(4, 1\), not broadcastable to its canvas \(5, 3\)"):
        ML.gather_canvases([None, fm[:4], None], plans, [1], 6, 3, "edit_mask")


@pytest.mark.parametrize("blend", ["linear", "uniform"])
def test_batch_tables_of_two_motions_pass_the_sampler_check(blend):
    ML = _ml()
    D = pkg("diffusion")
    plans = ML.script_plans([[("a", 16), ("b", 12), ("c", 16)], [("d", 10)], [("e", 14), ("f", 16)]], 4, 16)
    kw = ML.batch_tables(plans, [0, 2], 16, 4, blend)
    assert sorted(kw) == ["handshake_offsets", "handshake_owner_rows", "handshake_rows", "handshake_weights"]
    hs = D.check_handshake_kwargs(kw, (5, 16, 263))
    assert hs["nshared"] == 12 and hs["offsets"].tolist() == list(range(0, 25, 2))
    # the second motion's windows are batch rows 3 and 4: frames 10..13 of row 3 meet frames 0..3 of row 4
    assert hs["rows"][16:].tolist() == [3 * 16 + 10, 4 * 16, 3 * 16 + 11, 4 * 16 + 1, 3 * 16 + 12, 4 * 16 + 2, 3 * 16 + 13, 4 * 16 + 3]
    one = ML.handshake_tables(plans[0][2], plans[0][1], 16, 4, blend)
    assert hs["rows"][:16].tolist() == one["rows"].tolist() and hs["weights"][:16].tolist() == one["weights"].tolist()
    with pytest.raises(ValueError):  # the same tables over a batch that lacks the last window's row
        D.check_handshake_kwargs(kw, (4, 16, 263))
    assert D.check_handshake_kwargs(ML.batch_tables(plans, [1], 10, 4, blend), (1, 10, 263)) is None  # one window: no overlap


def test_compose_and_control_with_handshakes_are_not_implemented():
    D = pkg("diffusion")
    shape = (3, 16, 263)
    for extra in ({"compose_weights": torch.ones(3, 2)}, {"compose_text": [["a", "b"]] * 3},
                  {"control_joints": torch.zeros(3, 16, 22, 3)}, {"control_weights": torch.ones(3)}):
        with pytest.raises(NotImplementedError):
            D.check_handshake_kwargs(dict(_kw(), **extra), shape)


def test_trainer_script_errors():
    Tr = pkg("trainer")
    tr = Tr.DDPMTrainer.__new__(Tr.DDPMTrainer)
    tr.encoder = types.SimpleNamespace(num_frames=16, eval=lambda: None)
    for scripts, h in (([], 4),                                   # no motion
                       ([[]], 4),                                 # an empty script
                       ([[("a", 17)]], 4),                        # a window above num_frames
                       ([[("a", 16), ("b", 12)]], 7),             # overlap above half the shortest window
                       ([[("a", 16), ("b", 12)]], -1),
                       ([[("a", 16, 3)]], 4),
                       ([[(3, 16)]], 4)):
        with pytest.raises(ValueError):
            tr.generate_long(scripts, 263, overlap=h)
    with pytest.raises(ValueError):  # a motion of three windows in batches of two
        tr.generate_long([[("a", 16), ("b", 12), ("c", 16)]], 263, overlap=4, batch_size=2)
    with pytest.raises(ValueError):  # noise for one of two motions
        tr.generate_long([[("a", 16)], [("b", 16)]], 263, overlap=4, noise=[torch.zeros(16, 263)])
    with pytest.raises(ValueError):  # a canvas longer than the joint recovery holds
        tr.generate_long_joints([[("a", 16)] * 500], 263, np.zeros(263), np.ones(263), overlap=4, batch_size=500)

"""CPU: composed multi-prompt guidance -- the weight builders of motion_compose, validation of the compose kwargs, the
trainer's prompt_weights checks and argument checks of mdm_composed_update."""
import ctypes as C
import os
import types

import pytest
import torch

from conftest import pkg


def test_timeline_weights_partition_unity_and_crossfade():
    MC = pkg("motion_compose")
    w = MC.timeline_weights(10, [4])
    assert w.shape == (2, 10, 1) and w.dtype == torch.float32
    assert w[0, :, 0].tolist() == [1.0] * 4 + [0.0] * 6 and w[1, :, 0].tolist() == [0.0] * 4 + [1.0] * 6
    assert torch.equal(MC.timeline_weights(7, []), torch.ones(1, 7, 1))
    for T, bounds, blend in ((20, [5, 12], 4), (196, [60, 120], 10), (30, [10, 11, 20], 3), (12, [1, 11], 5)):
        w = MC.timeline_weights(T, bounds, blend)
        assert w.shape == (len(bounds) + 1, T, 1)
        assert (w >= 0).all() and (w <= 1).all()
        assert (w.sum(0) - 1).abs().max() < 1e-6, (T, bounds, blend)
    # a crossfade of `blend` frames centred between frames b - 1 and b: symmetric, linear, exact 0 / 1 outside it
    w = MC.timeline_weights(20, [10], blend=4)[1, :, 0]
    assert w[:8].eq(0).all() and w[12:].eq(1).all()
    assert torch.allclose(w[8:12], torch.tensor([0.125, 0.375, 0.625, 0.875]))
    assert torch.allclose(w[8:12] + w[8:12].flip(0), torch.ones(4))
    w = MC.timeline_weights(20, [10], blend=3)[1, :, 0]
    assert w[:8].eq(0).all() and w[11:].eq(1).all() and torch.allclose(w[9] + w[10], torch.tensor(1.0))
    assert (w[1:] >= w[:-1]).all()
    for bad in ((10, [0]), (10, [10]), (10, [5, 5]), (10, [6, 3]), (10, [3], -1), (0, [])):
        with pytest.raises(ValueError):
            MC.timeline_weights(*bad)


def test_body_part_weights_own_every_column_once():
    MC = pkg("motion_compose")
    E = pkg("motion_edit")
    w = MC.body_part_weights([E.UPPER_BODY, E.LOWER_BODY])
    assert w.shape == (2, 263) and w.dtype == torch.float32
    assert torch.equal(w.sum(0), torch.ones(263)) and set(w.unique().tolist()) == {0.0, 1.0}
    assert torch.equal(w[0], E.joint_feature_mask(E.UPPER_BODY)) and torch.equal(w[1], E.joint_feature_mask(E.LOWER_BODY))
    parts = [[j] for j in range(22)]
    w = MC.body_part_weights(parts)
    assert w.shape == (22, 263) and torch.equal(w.sum(0), torch.ones(263))
    for j in range(22):
        assert w[j].nonzero().flatten().tolist() == sorted(E.joint_columns(j))
    for bad in ([E.UPPER_BODY], [E.UPPER_BODY, E.LOWER_BODY, [3]], [E.UPPER_BODY, list(E.LOWER_BODY) + [22]], [],
                [list(range(22)), [-1]]):
        with pytest.raises(ValueError):
            MC.body_part_weights(bad)
    # products with a timeline stay a partition of unity: upper body A then B, lower body C throughout
    T = 30
    tl = MC.timeline_weights(T, [12], blend=4)
    bp = MC.body_part_weights([E.UPPER_BODY, E.LOWER_BODY])
    w = torch.stack([tl[0] * bp[0], tl[1] * bp[0], bp[1].expand(T, -1)])
    assert w.shape == (3, T, 263) and (w.sum(0) - 1).abs().max() < 1e-6


def _ok(B=2, K=3, T=5, F=7, N=4, Dt=6):
    return {"compose_weights": torch.rand(B, K, T, F), "compose_xf_proj": torch.zeros(B, K, Dt),
            "compose_xf_out": torch.zeros(B, K, N, Dt)}


def test_compose_kwargs_validation():
    D = pkg("diffusion")
    shape = (2, 5, 7)
    assert D.check_compose_kwargs({}, shape) is None and D.check_compose_kwargs({"xf_proj": 1, "length": 3}, shape) is None
    got = D.check_compose_kwargs(_ok(), shape, "cfg_ddim")
    assert got["K"] == 3 and got["weights"].shape == (2, 3, 5, 7) and got["text"] is None
    for w in (torch.ones(2, 3), torch.ones(2, 3, 5), torch.ones(2, 3, 1, 7), torch.ones(2, 3, 5, 1)):
        assert D.check_compose_kwargs(dict(_ok(), compose_weights=w), shape)["weights"].shape == (2, 3, 5, 7)
    w = torch.tensor([[1.0, 2.0, -1.0], [0.5, 0.25, 0.0]])
    got = D.check_compose_kwargs(dict(_ok(), compose_weights=w), shape)["weights"]
    assert torch.equal(got[:, :, 3, 4], w)  # (B, K) is per sample and prompt
    txt = {"compose_weights": torch.ones(2, 2), "compose_text": [("a", "b"), ["c", "d"]]}
    got = D.check_compose_kwargs(txt, shape, "cfg")
    assert got["K"] == 2 and got["text"] == [["a", "b"], ["c", "d"]] and got["xf_proj"] is None
    assert D.check_compose_kwargs({"compose_weights": torch.ones(2, 8), "compose_text": [["a"] * 8] * 2}, shape)["K"] == 8
    bad = [
        ({"compose_weights": torch.ones(2, 3)}, None),                                        # weights without prompts
        ({k: v for k, v in _ok().items() if k != "compose_weights"}, None),                   # prompts without weights
        ({k: v for k, v in _ok().items() if k != "compose_xf_out"}, None),                    # one embedding only
        (dict(_ok(), compose_text=[["a"] * 3] * 2), None),                                    # embeddings and captions
        (dict(_ok(), xf_proj=torch.zeros(2, 6)), None),                                       # plain prompt as well
        (dict(_ok(), xf_out=torch.zeros(2, 4, 6)), None),
        (dict(_ok(), compose_weights=torch.ones(2, 3, 4, 7)), None),                          # does not broadcast
        (dict(_ok(), compose_weights=torch.ones(2, 3, 5, 7, 1)), None),
        (dict(_ok(), compose_weights=torch.ones(1, 3, 5, 7)), None),                          # leading dims not (B, K)
        (dict(_ok(), compose_weights=torch.ones(2, 2, 5, 7)), None),
        (dict(_ok(), compose_weights=torch.ones(2)), None),
        (dict(_ok(), compose_weights=torch.tensor(1.0)), None),
        (dict(_ok(), compose_weights=torch.ones(2, 3, dtype=torch.int32)), None),
        (dict(_ok(), compose_weights=torch.full((2, 3), float("nan"))), None),                # non-finite
        (dict(_ok(), compose_weights=torch.full((2, 3), float("inf"))), None),
        (dict(_ok(), compose_xf_proj=torch.zeros(3, 3, 6)), None),                            # embedding shapes
        (dict(_ok(), compose_xf_out=torch.zeros(2, 2, 4, 6)), None),
        (dict(_ok(), compose_xf_out=torch.zeros(2, 3, 6)), None),
        ({"compose_weights": torch.ones(2, 2), "compose_text": [["a", "b"], ["c"]]}, None),   # K differs between samples
        ({"compose_weights": torch.ones(2, 2), "compose_text": [["a", "b"]]}, None),          # not one entry per sample
        ({"compose_weights": torch.ones(2, 1), "compose_text": ["a", "b"]}, None),            # captions, not sequences
        ({"compose_weights": torch.ones(2, 1), "compose_text": [[1], [2]]}, None),
        ({"compose_weights": torch.ones(2, 9), "compose_text": [["a"] * 9] * 2}, None),       # K above the maximum
        (_ok(K=9), None),
        ({"compose_weights": torch.ones(2, 0), "compose_text": [[], []]}, None),              # K = 0
        (_ok(), "ddim"),                                                                      # no guidance
        (_ok(), "ddpm"),
    ]
    for kw, mode in bad:
        with pytest.raises(ValueError):
            D.check_compose_kwargs(kw, shape, mode)
    pkg("_lib")
    assert pkg("_lib").COMPOSE_MAX_K == 8


def _cpu_trainer():
    Tr = pkg("trainer")
    m = torch.nn.Linear(1, 1)
    m.num_frames = 16
    m.encode_text = lambda text, device: pytest.fail("argument checks must fail before any text is encoded")
    return Tr.DDPMTrainer(types.SimpleNamespace(device=torch.device("cpu"), diffusion_steps=100, is_train=False), m)


def test_trainer_prompt_weight_checks():
    Cond = pkg("conditioning").Conditioning
    cw = lambda caps, w, dim_pose: Cond(caps, dim_pose, prompt_weights=w).weights  # noqa: E731
    caps = [("a", "b"), ("c", "d"), ("e", "f")]
    assert cw(caps, 1, 263).shape == (3, 2, 1, 263)
    assert cw(caps, torch.ones(3, 2), 263).shape == (3, 2, 1, 263)
    cond = Cond(caps, 263, prompt_weights=torch.rand(1, 2, 16, 1))
    w = cond.weights
    assert w.shape == (3, 2, 16, 263)
    assert cw(caps, torch.rand(1, 2, 1, 263), 263).shape == (3, 2, 1, 263)
    kw = cond.text_kwargs(slice(1, 3), 10)
    assert kw["compose_text"] == [["c", "d"], ["e", "f"]] and torch.equal(kw["compose_weights"], w[1:3, :, :10])
    kw = Cond(caps, 263, prompt_weights=1).text_kwargs(torch.tensor([2, 0]), 10)
    assert kw["compose_weights"].shape == (2, 2, 1, 263) and "xf_proj" not in kw
    assert kw["compose_text"] == [["e", "f"], ["a", "b"]]
    assert sorted(Cond(caps, 263, prompt_weights=1).kwargs(torch.tensor([2, 0]), 10, "cpu")) == sorted(kw)
    with pytest.raises(ValueError):  # the weights cover fewer frames than the batch
        cond.text_kwargs(slice(0, 3), 17)
    with pytest.raises(ValueError):
        cond.kwargs(slice(0, 3), 17, "cpu")
    for bad_caps, bad_w in ((["a", "b", "c"], 1), ([("a", "b"), ("c",), ("d", "e")], 1), ([("a", 1)] * 3, 1),
                            (caps, torch.ones(3, 3)), (caps, torch.ones(2, 2)), (caps, torch.ones(3, 2, 16, 262)),
                            (caps, torch.ones(3, 2, 16, 263, 1)), (caps, torch.rand(2, 1, 263)), (caps, torch.full((3, 2), float("nan")))):
        with pytest.raises(ValueError):
            cw(bad_caps, bad_w, 263)
    tr = _cpu_trainer()
    lens = torch.tensor([8, 8, 8])
    for kw in (dict(prompt_weights=1, caption=["a", "b", "c"]), dict(prompt_weights=torch.ones(3, 3), caption=caps),
               dict(prompt_weights=torch.full((3, 2), float("nan")), caption=caps)):
        cap = kw.pop("caption")
        for gen in (tr.generate, tr.generate_bucketed):
            with pytest.raises(ValueError):
                gen(cap, lens, 263, **kw)
    with pytest.raises(ValueError):  # every sampler of the trainer is guided; anything else is refused
        tr.generate(caps, lens, 263, sampler="plain", prompt_weights=1)


def test_composed_entry_rejects_bad_arguments_without_a_gpu():
    L = pkg("_lib")
    if not os.path.exists(L.LIB_PATH):
        pkg("build").build(verbose=False)
    lib = L.lib()
    p = C.c_void_p(16)  # never dereferenced: every call below must fail its argument check before any launch
    n, z = C.c_int64(8), C.c_void_p(0)

    def upd(x=p, eps=p, K=2, w=p, known=p, mask=p, tab=p, coef=p, steps=10, t_dev=p, t_imm=0, x_out=p, n=n):
        return lib.mdm_composed_update(x, eps, C.c_int32(K), w, p, p, known, mask, n, tab, coef, C.c_int32(steps), t_dev,
                                       C.c_int32(t_imm), C.c_float(2.5), C.c_int32(0), x_out, p, z)

    for bad in (dict(K=0), dict(K=-1), dict(K=9), dict(known=z), dict(mask=z), dict(x=z), dict(eps=z), dict(w=z),
                dict(tab=z), dict(coef=z), dict(x_out=z), dict(steps=0), dict(n=C.c_int64(-1)), dict(t_dev=z, t_imm=10),
                dict(t_dev=z, t_imm=-1)):
        assert upd(**bad) == 1, bad
    assert upd(n=C.c_int64(0)) == 0 and upd(known=z, mask=z, n=C.c_int64(0)) == 0 and upd(K=8, n=C.c_int64(0)) == 0
    assert upd(known=z, n=C.c_int64(0)) == 1 and upd(K=9, n=C.c_int64(0)) == 1

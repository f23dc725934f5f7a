"""CPU: the conditioning module -- the one align-and-expand helper and the row selection ``generate`` and
``generate_bucketed`` rest on: a batch's share of a call's conditioning is the full batch's, sliced to its rows."""
import numpy as np
import pytest
import torch

from conftest import pkg


def test_expand_to_alignment_and_messages():
    ex = pkg("conditioning").expand_to
    w = torch.arange(6.0).view(2, 3)
    got = ex(w, 1, (2, 3, 4), "w", "must lead with 2")
    assert got.shape == (2, 3, 4) and torch.equal(got[:, :, 2], w) and got.data_ptr() == w.data_ptr()  # (B, T): per frame
    assert torch.equal(ex(torch.tensor([1.0, 2.0]), 1, (2, 3, 4), "w")[:, 1, 1], torch.tensor([1.0, 2.0]))
    assert ex(torch.ones(3, 4), None, (2, 3, 4), "w").shape == (2, 3, 4)  # lead=None: trailing-aligned
    assert ex(2.0, 0, (2, 3, -1, 5), "w").shape == (2, 3, 1, 5) and ex(torch.ones(1, 3, 7, 1), 0, (2, 3, -1, 5), "w").shape[2] == 7
    with pytest.raises(ValueError, match=r"w of shape \(3, 3\) must lead with 2"):
        ex(torch.ones(3, 3), 1, (2, 3, 4), "w", "must lead with 2")
    with pytest.raises(ValueError, match=r"w of shape \(\) must lead with 2"):
        ex(torch.tensor(1.0), 1, (2, 3, 4), "w", "must lead with 2")
    with pytest.raises(ValueError, match="must lead"):
        ex(torch.ones(2, 3, 4, 1), 1, (2, 3, 4), "w", "must lead with 2")
    with pytest.raises(ValueError, match=r"w of shape \(2, 2\) does not broadcast to \(2, 3, 4\)"):
        ex(torch.ones(2, 2), 1, (2, 3, 4), "w")
    with pytest.raises(ValueError, match=r"w of shape \(3, 4\) does not broadcast to \(2, 3, 5\)"):
        ex(torch.ones(3, 4), None, (2, 3, 5), "w")
    with pytest.raises(ValueError, match=r"w: \(2, 2\) padded to \(2, 2, 1\)"):
        ex(torch.ones(2, 2), 1, (2, 3, 4), "w", fail_msg="{name}: {shape} padded to {padded}")


def _call(N=5, T=12, F=263):
    g = torch.Generator().manual_seed(0)
    caps = [(f"a{i}", f"b{i}") for i in range(N)]
    return caps, dict(edit_motion=torch.randn(N, T, F, generator=g), edit_mask=torch.rand(N, T, 1, generator=g),
                      prompt_weights=torch.randn(N, 2, T, 1, generator=g), control_joints=torch.randn(N, T, 22, 3, generator=g),
                      control_weights=torch.rand(N, T, generator=g), control_scale=0.5, control_iters=3,
                      mean=np.arange(F, dtype=np.float32), std=np.ones(F, np.float32))


@pytest.mark.parametrize("rows", [slice(1, 4), slice(0, 5), torch.tensor([3, 0, 4, 1])], ids=["slice", "all", "permuted"])
@pytest.mark.parametrize("T", [12, 8])
def test_rows_of_the_full_batch_equal_the_rows_asked_for(rows, T):
    Cond = pkg("conditioning").Conditioning
    caps, kw = _call()
    for cond in (Cond(caps, 263, **kw), Cond([c[0] for c in caps], 263, **{k: v for k, v in kw.items() if k != "prompt_weights"}),
                 Cond([c[0] for c in caps], 263)):
        full, part = cond.kwargs(slice(None), T, "cpu"), cond.kwargs(rows, T, "cpu")
        assert sorted(full) == sorted(part)
        pick = (lambda seq: seq[rows]) if isinstance(rows, slice) else (lambda seq: [seq[i] for i in rows.tolist()])
        for k, v in full.items():
            if torch.is_tensor(v):
                assert v.shape[0] == 5 and v.shape[1] in (2, 263, T) and torch.equal(part[k], v[rows]), k
            elif isinstance(v, list):
                assert part[k] == pick(v), k
            else:
                assert part[k] == v, k
    full = Cond(caps, 263, **kw).kwargs(slice(None), T, "cpu")
    assert sorted(full) == sorted(["compose_text", "compose_weights", "inpaint_motion", "inpaint_mask", "control_joints",
                                   "control_weights", "control_mean", "control_std", "control_scale", "control_iters"])
    assert full["compose_weights"].shape == (5, 2, T, 263) and full["control_weights"].shape == (5, T, 22, 3)
    assert full["inpaint_mask"].shape == (5, T, 263) and torch.equal(full["control_mean"][3], torch.arange(263.0))


def test_conditioning_checks_the_shapes_the_sampler_checks():
    """What ``Conditioning.kwargs`` hands out passes the sampler's own validation of a batch."""
    C = pkg("conditioning")
    caps, kw = _call()
    kw["control_weights"] = kw["control_weights"].abs()
    got = C.Conditioning(caps, 263, **kw).kwargs(torch.tensor([4, 2]), 8, "cpu")
    shape = (2, 8, 263)
    assert C.check_inpaint_kwargs(got, shape)[1].shape == shape
    assert C.check_compose_kwargs(got, shape, "cfg")["K"] == 2
    assert C.check_control_kwargs(got, shape)["iters"] == 3

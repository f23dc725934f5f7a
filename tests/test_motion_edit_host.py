"""CPU: motion editing -- the mask helpers of motion_edit, the feature layout they assume, the "ddpm" coefficient table,
validation of the editing kwargs and argument checks of mdm_guided_update_inpaint."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden, pkg


def _kw(steps, var="FIXED_SMALL"):
    D = pkg("diffusion")
    return dict(betas=D.get_named_beta_schedule("linear", steps), model_mean_type=D.ModelMeanType.EPSILON,
                model_var_type=getattr(D.ModelVarType, var), loss_type=D.LossType.MSE)


def test_frame_masks():
    E = pkg("motion_edit")
    p = E.prefix_mask(10, 3)
    assert p.shape == (10, 1) and p.dtype == torch.float32
    assert p[:, 0].tolist() == [1.0] * 3 + [0.0] * 7
    assert E.prefix_mask(5, 0).sum() == 0 and E.prefix_mask(5, 5).sum() == 5
    b = E.inbetween_mask(10, 2, 3)
    assert b.shape == (10, 1) and b[:, 0].tolist() == [1, 1, 0, 0, 0, 0, 0, 1, 1, 1]
    assert E.inbetween_mask(6, 0, 0).sum() == 0 and E.inbetween_mask(6, 2, 0)[:, 0].tolist() == [1, 1, 0, 0, 0, 0]
    assert E.inbetween_mask(6, 3, 3).sum() == 6
    for bad in ((10, -1), (10, 11)):
        with pytest.raises(ValueError):
            E.prefix_mask(*bad)
    for bad in ((10, 6, 5), (10, -1, 2), (10, 2, -1)):
        with pytest.raises(ValueError):
            E.inbetween_mask(*bad)
    # masks broadcast against (N, T, F) and combine
    both = torch.maximum(E.prefix_mask(10, 3), E.joint_feature_mask(E.UPPER_BODY))
    assert torch.broadcast_to(both, (2, 10, 263)).shape == (2, 10, 263)


def test_joint_columns_are_disjoint_and_cover_the_layout():
    E = pkg("motion_edit")
    J = 22
    assert E.feature_dim(J) == 263
    owner = {}
    for j in range(J):
        for c in E.joint_columns(j):
            assert c not in owner, (c, owner.get(c), j)
            owner[c] = j
    assert sorted(owner) == list(range(263))
    # the layout written out: root 4 | ric 21*3 | rot6d 21*6 | local velocity 22*3 | foot contacts 4
    assert [owner[c] for c in range(4)] == [0] * 4
    assert [owner[c] for c in range(4, 67)] == [j for j in range(1, 22) for _ in range(3)]
    assert [owner[c] for c in range(67, 193)] == [j for j in range(1, 22) for _ in range(6)]
    assert [owner[c] for c in range(193, 259)] == [j for j in range(22) for _ in range(3)]
    assert [owner[c] for c in range(259, 263)] == [7, 10, 8, 11]
    # named sets: disjoint, cover the skeleton, and their masks partition the features
    assert not set(E.UPPER_BODY) & set(E.LOWER_BODY) and sorted(E.UPPER_BODY + E.LOWER_BODY) == list(range(J))
    up, low = E.joint_feature_mask(E.UPPER_BODY), E.joint_feature_mask(E.LOWER_BODY)
    assert up.shape == (263,) and torch.equal(up + low, torch.ones(263))
    assert E.SMPL_JOINTS[7] == "left_ankle" and E.SMPL_JOINTS[11] == "right_foot" and len(E.SMPL_JOINTS) == J
    assert torch.equal(E.joint_feature_mask([]), torch.zeros(263))
    with pytest.raises(ValueError):
        E.joint_feature_mask([22])
    with pytest.raises(ValueError):
        E.joint_feature_mask([1], joints_num=21)


def test_joint_mask_perturbation_moves_only_those_joints_in_the_oracle():
    """recover_from_ric (oracle restatement) of a motion perturbed on joint_feature_mask(S) only: joints outside S stay."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import motion_ref as MR
    E = pkg("motion_edit")
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(2, 12, 263, generator=gen) * 0.3
    for S in (E.UPPER_BODY, (4, 7, 10), (21,)):
        m = E.joint_feature_mask(S)
        y = x + m * torch.randn(x.shape, generator=gen)
        a, b = MR.recover_from_ric(x), MR.recover_from_ric(y)
        moved = ((a - b).abs().amax(dim=(0, 1, 3)) > 0).nonzero().flatten().tolist()
        assert set(moved) <= set(S) and moved, (S, moved)


@pytest.mark.parametrize("steps,spaced", [(25, None), (1000, None), (1000, "ddim10"), (1000, [4, 3, 3])])
def test_ddpm_coefficient_table(steps, spaced):
    D = pkg("diffusion")
    d = D.GaussianDiffusion(**_kw(steps)) if spaced is None else D.SpacedDiffusion(D.space_timesteps(steps, spaced),
                                                                                   **_kw(steps))
    got = d.solver_coefficients("ddpm")
    assert got.dtype == np.float64 and got.shape == (d.num_timesteps, 4)
    assert np.array_equal(got[:, 0], d.posterior_mean_coef2) and np.array_equal(got[:, 1], d.posterior_mean_coef1)
    assert (got[:, 2] == 0).all()
    np.testing.assert_allclose(got[1:, 3], np.sqrt(d.posterior_variance[1:]), rtol=1e-12)
    assert np.array_equal(got[1:, 3], np.exp(0.5 * d.posterior_log_variance_clipped[1:])) and got[0, 3] == 0.0
    # rounded to f32, the last step is exactly {0, 1, 0, 0}: a binary mask's kept entries come out bit for bit
    assert tuple(got[0].astype(np.float32)) == (0.0, 1.0, 0.0, 0.0)
    for kind in ("ddim", "dpmpp"):
        assert tuple(d.solver_coefficients(kind).astype(np.float32)[0]) == (0.0, 1.0, 0.0, 0.0)
    # the rows the DDPM kernel reads from schedule_table, in the same f32 rounding
    tab = d.schedule_table()
    assert np.array_equal(got[:, 1].astype(np.float32), tab[2]) and np.array_equal(got[:, 0].astype(np.float32), tab[3])
    np.testing.assert_allclose(got[1:, 3].astype(np.float32), np.exp(0.5 * tab[4, 1:].astype(np.float64)), rtol=1e-6)


def test_ddpm_table_against_the_golden_schedule_and_fixed_large():
    g, meta = load_golden("loops_tiny")
    D = pkg("diffusion")
    for n, pre in ((25, "tables/"), (1000, "tables1000/")):
        got = D.GaussianDiffusion(**_kw(n)).solver_coefficients("ddpm")
        np.testing.assert_allclose(got[:, 0], g[pre + "posterior_mean_coef2"].numpy(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(got[:, 1], g[pre + "posterior_mean_coef1"].numpy(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(got[1:, 3], np.exp(0.5 * g[pre + "posterior_log_variance_clipped"].numpy()[1:]),
                                   rtol=1e-12)
    dl = D.GaussianDiffusion(**_kw(50, "FIXED_LARGE"))
    np.testing.assert_allclose(dl.solver_coefficients("ddpm")[1:, 3], np.sqrt(dl.betas[1:]), rtol=1e-12)


def test_inpaint_kwargs_validation():
    D = pkg("diffusion")
    shape = (2, 5, 7)
    k = torch.zeros(shape)
    assert D.check_inpaint_kwargs({}, shape) is None and D.check_inpaint_kwargs({"length": 3}, shape) is None
    for mask in (torch.ones(2, 5, 7), torch.ones(2, 5, 1), torch.ones(2, 1, 7), torch.ones(2, 5), torch.ones(2)):
        kn, m = D.check_inpaint_kwargs({"inpaint_motion": k, "inpaint_mask": mask}, shape)
        assert kn is k and m.shape == shape
    _, m = D.check_inpaint_kwargs({"inpaint_motion": k, "inpaint_mask": torch.tensor([[1.0] * 5, [0.0] * 5])}, shape)
    assert m[0].eq(1).all() and m[1].eq(0).all()  # a (B, T) mask is per sample and frame
    bad = [
        {"inpaint_motion": k},                                                   # one without the other
        {"inpaint_mask": torch.ones(shape)},
        {"inpaint_motion": torch.zeros(2, 5, 8), "inpaint_mask": torch.ones(shape)},   # motion shape
        {"inpaint_motion": torch.zeros(1, 5, 7), "inpaint_mask": torch.ones(1, 5, 7)},
        {"inpaint_motion": k, "inpaint_mask": torch.ones(5, 7)},                # leading dim is not B
        {"inpaint_motion": k, "inpaint_mask": torch.ones(1, 5, 7)},
        {"inpaint_motion": k, "inpaint_mask": torch.tensor(1.0)},
        {"inpaint_motion": k, "inpaint_mask": torch.ones(2, 4, 7)},             # does not broadcast
        {"inpaint_motion": k, "inpaint_mask": torch.ones(2, 5, 7, 1)},
        {"inpaint_motion": k, "inpaint_mask": torch.full(shape, 1.5)},          # range
        {"inpaint_motion": k, "inpaint_mask": torch.full(shape, -0.25)},
        {"inpaint_motion": k, "inpaint_mask": torch.full(shape, float("nan"))},  # finiteness
        {"inpaint_motion": torch.full(shape, float("inf")), "inpaint_mask": torch.ones(shape)},
        {"inpaint_motion": torch.full(shape, float("nan")), "inpaint_mask": torch.ones(shape)},
        {"inpaint_motion": torch.zeros(shape, dtype=torch.int32), "inpaint_mask": torch.ones(shape)},
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            D.check_inpaint_kwargs(kw, shape)


def test_trainer_edit_kwargs_slice_rows_and_frames():
    Cond = pkg("conditioning").Conditioning
    E = pkg("motion_edit")
    caps = ["a", "b", "c"]
    k = torch.arange(3 * 8 * 263, dtype=torch.float32).view(3, 8, 263)
    assert Cond(caps, 263).edit_kwargs(slice(0, 3), 8) == {}
    assert Cond(caps, 263).kwargs(slice(0, 3), 8, "cpu") == {"text": caps}
    kw = Cond(caps, 263, edit_motion=k, edit_mask=E.prefix_mask(8, 2)).edit_kwargs(torch.tensor([2, 0]), 5)
    assert torch.equal(kw["inpaint_motion"], k[[2, 0], :5])
    assert kw["inpaint_mask"].shape == (2, 5, 263) and kw["inpaint_mask"][:, :2].eq(1).all()
    assert kw["inpaint_mask"][:, 2:].eq(0).all()
    kw = Cond(caps, 263, edit_motion=k, edit_mask=E.joint_feature_mask(E.LOWER_BODY)).kwargs(slice(1, 3), 8, "cpu")
    assert torch.equal(kw["inpaint_mask"][1, 7], E.joint_feature_mask(E.LOWER_BODY)) and kw["text"] == ["b", "c"]
    for bad in ((k, None), (None, torch.ones(8, 1)), (k[:, :4], torch.ones(4, 1)), (k[..., :262], torch.ones(1)),
                (k, torch.ones(7, 1))):
        with pytest.raises(ValueError):
            Cond(caps, 263, edit_motion=bad[0], edit_mask=bad[1]).edit_kwargs(slice(0, 3), 5)


def test_inpaint_entry_rejects_bad_arguments_without_a_gpu():
    L = pkg("_lib")
    if not os.path.exists(L.LIB_PATH):
        pkg("build").build(verbose=False)
    lib = L.lib()
    p = C.c_void_p(16)  # never dereferenced: every call below must fail its argument check before any launch
    n, z = C.c_int64(8), C.c_void_p(0)

    def upd(x=p, ec=p, known=p, mask=p, tab=p, coef=p, steps=10, t_dev=p, t_imm=0, x_out=p, n=n):
        return lib.mdm_guided_update_inpaint(x, ec, p, p, p, known, mask, n, tab, coef, C.c_int32(steps), t_dev,
                                             C.c_int32(t_imm), C.c_float(2.5), C.c_int32(0), x_out, p, z)

    for bad in (dict(known=z), dict(mask=z), dict(known=z, mask=z), dict(x=z), dict(ec=z), dict(tab=z), dict(coef=z),
                dict(x_out=z), dict(steps=0), dict(n=C.c_int64(-1)), dict(n=C.c_int64(-4)), dict(t_dev=z, t_imm=10),
                dict(t_dev=z, t_imm=-1)):
        assert upd(**bad) == 1, bad
    assert upd(n=C.c_int64(0)) == 0  # nothing to do: no launch
    assert upd(known=z, n=C.c_int64(0)) == 1  # a null known is an error even with nothing to do

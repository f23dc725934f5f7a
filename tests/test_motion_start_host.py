"""CPU: motion-to-motion generation without a device.

* the "ddim_inverse" coefficient table against a restatement from abar in f64, and the identity that makes it right: row t
  of it followed by row t + 1 of the "ddim" table at eta = 0 gives any (x, eps) back;
* the DPM-Solver++ table with a start row: first order there, unchanged below, and the plain table for None / the last row;
* the strength -> steps mapping at N = 1, 20, 1000, both ends included;
* every ValueError of the new inputs (exclusive inputs, missing mean / std, short clips, non-finite values, latents with
  the wrong sampler or step count), the conversion of joints injected so that no HIP library is needed;
* the argument checks of mdm_diffuse_start, which return before the device is touched.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import pkg


def _kw(steps):
    D = pkg("diffusion")
    return dict(betas=D.get_named_beta_schedule("linear", steps), model_mean_type=D.ModelMeanType.EPSILON,
                model_var_type=D.ModelVarType.FIXED_SMALL, loss_type=D.LossType.MSE)


def _schedules():
    D = pkg("diffusion")
    return {"plain25": D.GaussianDiffusion(**_kw(25)),
            "ddim10": D.SpacedDiffusion(D.space_timesteps(1000, "ddim10"), **_kw(1000)),
            "plain1000": D.GaussianDiffusion(**_kw(1000))}


@pytest.mark.parametrize("name", ["plain25", "ddim10", "plain1000"])
def test_inversion_table(name):
    d = _schedules()[name]
    N, acp = d.num_timesteps, d.alphas_cumprod
    inv = d.solver_coefficients("ddim_inverse")
    assert inv.shape == (N, 4) and inv.dtype == np.float64
    assert np.array_equal(inv[N - 1], [1.0, 0.0, 0.0, 0.0]) and not inv[:, 2:].any()
    # restated from abar, element by element
    for t in range(N - 1):
        al, si = np.sqrt(acp[t]), np.sqrt(1.0 - acp[t])
        al1, si1 = np.sqrt(acp[t + 1]), np.sqrt(1.0 - acp[t + 1])
        assert abs(inv[t, 0] - si1 / si) <= 1e-12 * (si1 / si), t
        c0 = al1 - si1 / si * al
        # c0 is a difference of two terms of the size of alpha_{t+1}: the bound is relative to the terms
        assert abs(inv[t, 1] - c0) <= 1e-12 * max(abs(c0), al1), t
    # row t, then the DDIM eta = 0 row t + 1, is the identity on (x0, eps): the step the kernel does under a table is
    # x0 = (x - sigma eps) / alpha, out = cx x + c0 x0, and eps of the result is re-derived from x0 at the new level
    ddim = d.solver_coefficients("ddim", 0.0)
    rng = np.random.RandomState(0)
    x, eps = rng.randn(64), rng.randn(64)
    for t in range(N - 1):
        al, si = np.sqrt(acp[t]), np.sqrt(1.0 - acp[t])
        x0 = (x - si * eps) / al
        up = inv[t, 0] * x + inv[t, 1] * x0  # level t + 1, the same (x0, eps)
        back = ddim[t + 1, 0] * up + ddim[t + 1, 1] * x0
        scale = np.abs(x).max() + np.abs(x0).max()
        assert np.abs(back - x).max() <= 1e-12 * scale, (t, np.abs(back - x).max())
        al1, si1 = np.sqrt(acp[t + 1]), np.sqrt(1.0 - acp[t + 1])
        assert np.abs((up - al1 * x0) / si1 - eps).max() <= 1e-12 * scale / si1, t  # eps is carried unchanged


@pytest.mark.parametrize("name", ["plain25", "ddim10"])
def test_dpmpp_table_with_a_start_row(name):
    d = _schedules()[name]
    N = d.num_timesteps
    plain, ddim = d.solver_coefficients("dpmpp", 0.0, 2), d.solver_coefficients("ddim", 0.0)
    assert np.array_equal(d.solver_coefficients("dpmpp", 0.0, 2, start=None), plain)
    assert np.array_equal(d.solver_coefficients("dpmpp", 0.0, 2, start=N - 1), plain)
    for start in range(N):
        tab = d.solver_coefficients("dpmpp", 0.0, 2, start=start)
        assert tab[start, 2] == 0.0 and tab[start, 3] == 0.0
        # the same two numbers evaluated along two routes in f64; c0 is a difference of terms of the size of alpha_{t-1}
        a_prev = np.sqrt(d.alphas_cumprod_prev[start])
        assert abs(tab[start, 0] - ddim[start, 0]) <= 1e-12 * abs(ddim[start, 0]), start
        assert abs(tab[start, 1] - ddim[start, 1]) <= 1e-12 * a_prev, start
        keep = np.arange(N) != start
        assert np.array_equal(tab[keep], plain[keep]), start
        if 0 < start < N - 1:
            assert plain[start, 2] != 0.0  # the row that was second order
    assert np.array_equal(d.solver_coefficients("dpmpp", 0.0, 1, start=3), d.solver_coefficients("dpmpp", 0.0, 1))
    with pytest.raises(ValueError):
        d.solver_coefficients("ddim", 0.0, 2, start=3)
    with pytest.raises(ValueError):
        d.solver_coefficients("dpmpp", 0.0, 2, start=N)
    with pytest.raises(ValueError):
        d.solver_coefficients("dpmpp", 0.0, 2, start=-1)


def test_strength_mapping():
    Cd = pkg("conditioning")
    f = Cd.strength_steps
    assert [f(s, 1) for s in (0.0, 0.49, 0.5, 1.0)] == [0, 0, 1, 1]
    assert [f(s, 20) for s in (0.0, 0.02, 0.025, 0.5, 0.52, 0.53, 0.974, 0.975, 1.0)] == [0, 0, 1, 10, 10, 11, 19, 20, 20]
    assert [f(s, 1000) for s in (0.0, 0.0004, 0.0005, 0.3, 0.9994, 0.9996, 1.0)] == [0, 0, 1, 300, 999, 1000, 1000]
    for n in (1, 20, 1000):
        assert f(0.0, n) == 0 and f(1.0, n) == n
        assert all(f(k / n, n) == k for k in range(n + 1))
    for bad in (-0.01, 1.01, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            f(bad, 20)


def test_start_row_checks():
    d = _schedules()["ddim10"]
    assert d._start_row(None) is None and d._start_row(4) == 4 and d._start_row(torch.tensor([4, 4])) == 4
    with pytest.raises(NotImplementedError):
        d._start_row(torch.tensor([4, 3]))
    for bad in (10, -1, 2.0):
        with pytest.raises(ValueError):
            d._start_row(bad)
    x = torch.zeros(2, 4, 5)
    assert d._partial(None, None, None, x.shape) == (None, None)
    assert d._partial(None, 3, x, x.shape) == (3, None)  # noise is x at that level
    start, got = d._partial(x, 3, None, x.shape)
    assert start == 3 and got is x
    with pytest.raises(ValueError):
        d._partial(x, None, None, x.shape)  # init_motion without start_step
    with pytest.raises(ValueError):
        d._partial(None, 3, None, x.shape)  # start_step with nothing to start from
    with pytest.raises(ValueError):
        d._partial(x[:, :3], 3, None, x.shape)
    with pytest.raises(ValueError):
        d._partial(torch.full_like(x, float("nan")), 3, None, x.shape)
    with pytest.raises(ValueError):
        d.ddim_invert_loop(None, x, {"inpaint_mask": x})


def _to_motion(clips, lengths, mean, std, *, skeleton="t2m", **kw):
    """joints_to_motion's signature on a stand-in: a clip of n frames gives n - 1 rows (its joints' x, tiled)."""
    assert lengths is None
    n = max(c.shape[0] for c in clips) - 1
    rows = torch.zeros(len(clips), n, 263)
    for i, c in enumerate(clips):
        rows[i, :c.shape[0] - 1] = c[:-1, :, 0].mean(1, keepdim=True)
    return rows


def test_validation():
    Cd = pkg("conditioning")
    caps, mean, std = ["a", "b", "c"], np.zeros(263, np.float32), np.ones(263, np.float32)
    rows = torch.randn(3, 16, 263, generator=torch.Generator().manual_seed(0))
    clips = [torch.randn(n, 22, 3, generator=torch.Generator().manual_seed(n)) for n in (17, 13, 17)]

    def cond(**kw):
        return Cd.Conditioning(caps, 263, to_motion=_to_motion, **kw)

    # exclusive inputs
    for extra in (dict(init_joints=clips, mean=mean, std=std), dict(init_bvh=["x.bvh"] * 3, mean=mean, std=std)):
        with pytest.raises(ValueError, match="exclusive"):
            cond(init_motion=rows, strength=0.5, **extra)
    with pytest.raises(ValueError, match="exclusive"):
        cond(init_joints=clips, init_bvh=["x.bvh"] * 3, strength=0.5, mean=mean, std=std)
    with pytest.raises(ValueError, match="exclusive"):
        cond(init_motion=rows, strength=0.5, latents=rows, latent_step=3)
    # strength and the motion go together; the strength's range
    with pytest.raises(ValueError, match="strength"):
        cond(init_motion=rows)
    with pytest.raises(ValueError, match="strength"):
        cond(strength=0.5)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="strength"):
            cond(init_motion=rows, strength=bad)
    # joints and files need mean / std
    for extra in (dict(), dict(mean=mean), dict(std=std)):
        with pytest.raises(ValueError, match="mean and std"):
            cond(init_joints=clips, strength=0.5, **extra)
        with pytest.raises(ValueError, match="mean and std"):
            cond(init_bvh=["x.bvh"] * 3, strength=0.5, **extra)
    # shapes and values
    with pytest.raises(ValueError):
        cond(init_motion=rows[:2], strength=0.5)
    with pytest.raises(ValueError):
        cond(init_motion=rows[:, :, :100], strength=0.5)
    for bad in (float("nan"), float("inf")):
        x = rows.clone()
        x[1, 2, 3] = bad
        with pytest.raises(ValueError, match="non-finite"):
            cond(init_motion=x, strength=0.5)
        with pytest.raises(ValueError, match="non-finite"):
            cond(latents=x, latent_step=3)
        cl = [c.clone() for c in clips]
        cl[2][4, 5, 0] = bad
        with pytest.raises(ValueError, match="non-finite"):
            cond(init_joints=cl, strength=0.5, mean=mean, std=std)
    # a clip shorter than its sample's length: rows against m_lens, per sample
    c = cond(init_joints=clips, strength=0.5, mean=mean, std=std)
    assert c.init[1] == [16, 12, 16]
    kw, done = c.start_kwargs(slice(0, 3), 16, torch.tensor([16, 12, 16]), 20, "dpmpp2m", "cpu")
    assert done is None and kw["start_step"] == 9 and tuple(kw["init_motion"].shape) == (3, 16, 263)
    assert torch.equal(kw["init_motion"][1, 12:], torch.zeros(4, 263))
    with pytest.raises(ValueError, match="shorter"):
        c.start_kwargs(slice(0, 3), 16, torch.tensor([16, 13, 16]), 20, "dpmpp2m", "cpu")
    with pytest.raises(ValueError, match="shorter"):
        c.start_kwargs(torch.tensor([1]), 14, torch.tensor([14]), 20, "dpmpp2m", "cpu")
    with pytest.raises(ValueError, match="shorter"):
        cond(init_motion=rows, strength=0.5).start_kwargs(slice(0, 3), 18, torch.tensor([18, 4, 4]), 20, "ddim", "cpu")
    # the ends of the strength, and each batch's rows and frames
    c = cond(init_motion=rows, strength=1.0)
    assert c.start_kwargs(slice(1, 3), 16, torch.tensor([16, 16]), 20, "ddim", "cpu") == ({}, None)
    kw, done = cond(init_motion=rows, strength=0.0).start_kwargs(slice(1, 3), 12, torch.tensor([12, 12]), 20, "ddim", "cpu")
    assert kw == {} and torch.equal(done, rows[1:3, :12])
    kw, done = cond(init_motion=rows, strength=0.25).start_kwargs(torch.tensor([2, 0]), 8, torch.tensor([8, 8]), 20, "ddpm", "cpu")
    assert kw["start_step"] == 4 and torch.equal(kw["init_motion"], rows[[2, 0], :8])
    assert cond().start_kwargs(slice(0, 3), 16, torch.tensor([16] * 3), 20, "ddim", "cpu") == ({}, None)
    # latents: both or neither, the sampler and the step count of the inversion
    with pytest.raises(ValueError, match="go together"):
        cond(latents=rows)
    with pytest.raises(ValueError, match="go together"):
        cond(latent_step=3)
    with pytest.raises(ValueError):
        cond(latents=rows[:2], latent_step=3)
    c = cond(latents=rows, latent_step=Cd.LatentStep(49, 50))
    lens = torch.tensor([16, 16, 16])
    kw, done = c.start_kwargs(slice(0, 3), 16, lens, 50, "ddim", "cpu")
    assert done is None and kw["start_step"] == 49 and torch.equal(kw["noise"], rows)
    for sampler in ("ddpm", "dpmpp2m"):
        with pytest.raises(ValueError, match="ddim"):
            c.start_kwargs(slice(0, 3), 16, lens, 50, sampler, "cpu")
    with pytest.raises(ValueError, match="sample_steps"):
        c.start_kwargs(slice(0, 3), 16, lens, 100, "ddim", "cpu")  # another step count, the step inside it
    with pytest.raises(ValueError, match="sample_steps"):
        c.start_kwargs(slice(0, 3), 16, lens, 20, "ddim", "cpu")
    with pytest.raises(ValueError, match="sample_steps"):
        cond(latents=rows, latent_step=20).start_kwargs(slice(0, 3), 16, lens, 20, "ddim", "cpu")  # a plain int: its range
    with pytest.raises(ValueError, match="frames"):
        c.start_kwargs(slice(0, 3), 18, torch.tensor([18] * 3), 50, "ddim", "cpu")
    lat = cond(latents=[rows[0], rows[1, :12], rows[2]], latent_step=3)  # a list, padded
    assert tuple(lat.latents.shape) == (3, 16, 263)


def test_argument_checks_of_the_start_kernel_without_gpu():
    """mdm_diffuse_start refuses bad arguments before it touches the device (MDM_ERR_ARG = 1) and accepts empty work."""
    L = pkg("_lib")
    lib = L.lib()
    buf = (C.c_float * 8)()
    p = C.addressof(buf)

    def call(x=p, noise=None, out=p, per=4, n=2, s0=0, ids=None, seed=1, a=0.5, s=0.5):
        return lib.mdm_diffuse_start(x, noise, out, per, n, s0, ids, seed, a, s, None)

    assert call(x=None) == 1 and call(out=None) == 1
    assert call(per=-1) == 1 and call(n=-1) == 1 and call(s0=-1) == 1
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert call(a=bad) == 1 and call(s=bad) == 1
    assert call(per=0) == 0 and call(n=0) == 0  # nothing to do: no launch
    assert "mdm_diffuse_start" in L.PROTOTYPES and L.PROTOTYPES["mdm_diffuse_start"][1][-3:-1] == [C.c_float, C.c_float]

"""CPU: terrain host logic.

* the constructors: heightfield, ramp and stairs heights worked out by hand, batch_terrain's padding, terrain_to_local;
* every ValueError of the helpers;
* the fp64 autograd restatement of tests/terrain_ref.py against central finite differences: the keep-above term only, with
  stand weights, with a yaw and cell_x != cell_z, and with a scene, tracks and targets; terrain_height against it;
* penetration(terrain=) on hand-placed joints;
* the argument errors of the five new entries on the loaded library, without a GPU;
* model kwargs: check_control_kwargs with control_terrain / control_terrain_rec / control_stand and every ValueError, the
  refusal next to long-motion handshakes, dist.shard_kwargs; Conditioning and the trainer's terrain= / terrain_stand=;
* long motions: check_canvas_control_kwargs with the canvas_control_terrain* keys and every ValueError, canvas_control and
  generate_long with one terrain per motion.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from conftest import pkg

import scene_ref as R
import scene_tracks_ref as TR
import terrain_ref as G
from test_motion_control_host import ref_positions

T = 12


# ---- constructors -------------------------------------------------------------------------------------------------------
def test_heightfield_record_and_heights():
    MS = pkg("motion_scene")
    t = MS.heightfield([[0.0, 1.0, 2.0], [3.0, 4.0, 5.0]], (0.5, 2.0), origin=(1.0, -1.0), yaw=0.3, margin=0.02, weight=1.5)
    assert tuple(t.heights.shape) == (2, 3) and t.heights.dtype == torch.float32
    assert t.record.tolist() == pytest.approx([1.0, -1.0, math.cos(0.3), math.sin(0.3), 2.0, 0.5, 1.5, 0.02])
    assert MS.heightfield(np.zeros((2, 2)), 0.25).record.tolist() == [0.0, 0.0, 1.0, 0.0, 4.0, 4.0, 1.0, 0.0]
    # samples stand at local (i cell_x, k cell_z), local = R_y(-yaw) (p - origin): p = origin + R_y(yaw) local
    c, s = math.cos(0.3), math.sin(0.3)
    for k in range(2):
        for i in range(3):
            lx, lz = 0.5 * i, 2.0 * k
            p = torch.tensor([[1.0 + c * lx + s * lz, -1.0 - s * lx + c * lz]], dtype=torch.float64)
            assert float(MS.terrain_height(t, p)) == pytest.approx(3.0 * k + i, abs=1e-12)
    # bilinear inside a cell, the edge's height outside (zero slope in the clamped direction)
    flat = MS.heightfield([[0.0, 1.0, 2.0], [3.0, 4.0, 5.0]], (0.5, 2.0))
    q = torch.tensor([[0.25, 1.0], [0.75, 0.5], [-3.0, 1.0], [9.0, 0.0], [0.5, -2.0], [0.5, 7.0], [9.0, 9.0]], dtype=torch.float64)
    assert MS.terrain_height(flat, q).tolist() == pytest.approx([2.0, 2.25, 1.5, 2.0, 1.0, 4.0, 5.0])
    assert MS.terrain_height(flat, q.float()).dtype == torch.float32


def test_ramp_and_stairs_by_hand():
    MS = pkg("motion_scene")
    xz = lambda *v: torch.tensor(v, dtype=torch.float64).reshape(-1, 2)  # noqa: E731
    r = MS.ramp((1.0, 2.0), 0.0, 4.0, 0.5, 2.0)
    assert tuple(r.heights.shape) == (2, 2) and r.record[:2].tolist() == [1.0, 1.0]  # the corner: half a width to the side
    assert MS.terrain_height(r, xz(0.0, 2.0, 1.0, 2.0, 2.0, 2.5, 3.0, 1.2, 5.0, 2.0, 9.0, 2.0, 3.0, 50.0)).tolist() == pytest.approx(
        [0.0, 0.0, 0.125, 0.25, 0.5, 0.5, 0.25])
    # turned: the climb runs along R_y(yaw) (1, 0, 0) = (cos yaw, -sin yaw)
    yaw = 0.7
    r = MS.ramp((1.0, 2.0), yaw, 4.0, -0.8, 2.0)
    along = [(1.0 + d * math.cos(yaw), 2.0 - d * math.sin(yaw)) for d in (-1.0, 0.0, 1.0, 4.0, 6.0)]
    assert MS.terrain_height(r, xz(*[v for p in along for v in p])).tolist() == pytest.approx([0.0, 0.0, -0.2, -0.8, -0.8])
    s = MS.stairs((0.0, 0.0), 0.0, 3, 0.2, 0.3, 1.0, cell=0.1)
    assert tuple(s.heights.shape) == (2, 10)
    assert s.heights[0].tolist() == pytest.approx([0.0, 0.2, 0.2, 0.2, 0.4, 0.4, 0.4, 0.6, 0.6, 0.6])
    assert torch.equal(s.heights[0], s.heights[1]) and s.record[:2].tolist() == [0.0, -0.5]
    # every riser spans one cell: the first from the start on; treads are flat; the top tread's height behind
    got = MS.terrain_height(s, xz(-1.0, 0.0, 0.0, 0.0, 0.05, 0.0, 0.1, 0.2, 0.25, 0.0, 0.35, 0.0, 0.45, 0.0, 0.65, -0.3, 0.95, 0.0, 5.0, 0.0))
    assert got.tolist() == pytest.approx([0.0, 0.0, 0.1, 0.2, 0.2, 0.3, 0.4, 0.5, 0.6, 0.6])
    down = MS.stairs((0.0, 0.0), 0.0, 2, -0.15, 0.26, 1.0)  # the run rounded to whole cells of 0.05
    assert tuple(down.heights.shape) == (2, 11) and float(down.heights.min()) == pytest.approx(-0.3)


def test_batch_terrain_pads_by_edge_replication():
    MS = pkg("motion_scene")
    a = MS.heightfield(torch.arange(6.0).reshape(2, 3), 0.5, (0.3, 0.1), 0.2)
    b = MS.stairs((0.0, 0.0), 0.0, 2, 0.2, 0.2, 1.0, cell=0.1)  # (2, 5)
    c = MS.heightfield(torch.arange(12.0).reshape(4, 3), (1.0, 2.0))
    hs, rec = MS.batch_terrain(a, 3)
    assert tuple(hs.shape) == (3, 2, 3) and tuple(rec.shape) == (3, 8) and hs.dtype == rec.dtype == torch.float32
    assert torch.equal(hs[2], a.heights) and torch.equal(rec[1], a.record.float())
    hs, rec = MS.batch_terrain([a, b, c], 3)
    assert tuple(hs.shape) == (3, 4, 5)
    assert hs[0].tolist() == [[0, 1, 2, 2, 2], [3, 4, 5, 5, 5], [3, 4, 5, 5, 5], [3, 4, 5, 5, 5]]
    # padding changes no height: past its edge a terrain continues flat
    g = torch.Generator().manual_seed(0)
    q = (torch.rand(200, 2, generator=g, dtype=torch.float64) - 0.3) * 6
    for k, t in enumerate((a, b, c)):
        padded = MS.Terrain(hs[k], rec[k].double())
        assert float((MS.terrain_height(padded, q) - MS.terrain_height(t, q)).abs().max()) <= 1e-6
    assert tuple(MS.batch_terrain([], 0)[0].shape) == (0, 2, 2)


def test_terrain_to_local_changes_only_the_record():
    MS = pkg("motion_scene")
    g = torch.Generator().manual_seed(1)
    t = MS.heightfield(torch.randn(4, 5, generator=g), (0.4, 0.7), (1.0, -2.0), 0.3, margin=0.01, weight=2.0)
    loc = MS.terrain_to_local(t, (0.5, 1.5), 0.8)
    assert loc.heights is t.heights and loc.record[4:].tolist() == t.record[4:].tolist()
    p = torch.randn(50, 3, generator=g, dtype=torch.float64) * 2
    world = MS.to_world(p, (0.5, 1.5), 0.8)
    assert float((MS.terrain_height(loc, p[:, [0, 2]]) - MS.terrain_height(t, world[:, [0, 2]])).abs().max()) <= 1e-12
    assert MS.terrain_to_local(t, (0.0, 0.0), 0.0).record.tolist() == pytest.approx(t.record.tolist())


def test_constructor_and_packing_errors():
    MS = pkg("motion_scene")
    ok = np.zeros((3, 3))
    for bad in (np.array([[0.0, np.nan], [0.0, 0.0]]), np.array([[0.0, np.inf], [0.0, 0.0]])):
        with pytest.raises(ValueError, match="non-finite"):
            MS.heightfield(bad, 0.1)
    for cell in (0.0, -1.0, (0.1, 0.0), float("nan"), float("inf")):
        with pytest.raises(ValueError, match="cell"):
            MS.heightfield(ok, cell)
    with pytest.raises(ValueError, match="cell"):
        MS.heightfield(ok, (0.1, 0.1, 0.1))
    for w in (-0.1, float("nan")):
        with pytest.raises(ValueError, match="weight"):
            MS.heightfield(ok, 0.1, weight=w)
    with pytest.raises(ValueError, match="margin"):
        MS.heightfield(ok, 0.1, margin=float("inf"))
    for shape in ((1, 3), (3, 1), (513, 2), (2, 513)):
        with pytest.raises(ValueError, match="2 to 512"):
            MS.heightfield(np.zeros(shape), 0.1)
    assert tuple(MS.heightfield(np.zeros((512, 2)), 0.1).heights.shape) == (512, 2)
    with pytest.raises(ValueError, match=r"\(Gz, Gx\)"):
        MS.heightfield(np.zeros(4), 0.1)
    with pytest.raises(ValueError, match="origin"):
        MS.heightfield(ok, 0.1, origin=(0.0, 0.0, 0.0))
    with pytest.raises(ValueError, match="2 to 512"):
        MS.stairs((0, 0), 0.0, 200, 0.2, 0.3, 1.0)  # 200 treads of 6 cells
    with pytest.raises(ValueError, match="steps"):
        MS.stairs((0, 0), 0.0, 0, 0.2, 0.3, 1.0)
    for kw in (dict(run=0.0), dict(width=-1.0), dict(cell=0.0), dict(rise=float("nan"))):
        a = dict(dict(start=(0, 0), yaw=0.0, steps=2, rise=0.2, run=0.3, width=1.0), **kw)
        with pytest.raises(ValueError):
            MS.stairs(**a)
    for kw in (dict(length=0.0), dict(width=0.0), dict(rise=float("inf"))):
        a = dict(dict(start=(0, 0), yaw=0.0, length=2.0, rise=0.5, width=1.0), **kw)
        with pytest.raises(ValueError):
            MS.ramp(**a)
    t = MS.heightfield(ok, 0.1)
    for bad, n in ((t, 0), ([t], 2), ([t, "x"], 2), (ok, 1)):
        with pytest.raises(ValueError, match="one terrain"):
            MS.batch_terrain(bad if n else [t], n if n else 2)
    rec = t.record.clone()
    rec[6] = -1.0
    with pytest.raises(ValueError, match="weight"):
        MS.check_terrain(t.heights, rec)
    with pytest.raises(ValueError, match="record"):
        MS.check_terrain(t.heights, t.record[:7])
    with pytest.raises(ValueError, match=r"\(2, 22\)"):
        MS.check_stand(torch.zeros(2, 21), (2, 22))
    for v in (-0.1, float("nan")):
        with pytest.raises(ValueError, match="finite and >= 0"):
            MS.check_stand(torch.full((2, 22), v), (2, 22))
    with pytest.raises(ValueError, match=r"\(\.\.\., 2\)"):
        MS.terrain_height(t, torch.zeros(3, 3))


# ---- the restatement ----------------------------------------------------------------------------------------------------
def _case(n=T, F=263, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(1, n, F, generator=g, dtype=torch.float64) * 0.5
    mean = torch.randn(F, generator=g, dtype=torch.float64) * 0.1
    std = torch.rand(F, generator=g, dtype=torch.float64) + 0.5
    return x, mean, std


@pytest.mark.parametrize("kind", ["above", "stand", "yaw", "all"])
def test_reference_gradient_matches_finite_differences(kind):
    """A grid placed from the positions, clear of its lines, so that both terms penalise joints: autograd against central
    differences of the fp64 loss.  "above": S = None; "stand": with S; "yaw": a 3 x 5 grid turned by 0.4 with cell_x != cell_z;
    "all": with a static scene, tracks, radii, joint weights and targets."""
    MS = pkg("motion_scene")
    F, J = 263, 22
    x, mean, std = _case(T, F, seed=3)
    P = ref_positions(x[0, :T - 1], mean, std).detach()
    g = torch.Generator().manual_seed(5)
    jp = torch.zeros(J, 2, dtype=torch.float64)
    jp[:, 1] = 1.0
    S = None if kind == "above" else torch.rand(T, J, generator=g, dtype=torch.float64) * 1.5
    tg = w = scene = tracks = None
    if kind == "all":
        jp[:, 0] = torch.rand(J, generator=g, dtype=torch.float64) * 0.1
        jp[:, 1] = torch.rand(J, generator=g, dtype=torch.float64) * 2
        jp[3, 1] = 0.0
        tg = torch.randn(1, T, J, 3, generator=g, dtype=torch.float64)
        w = torch.rand(1, T, J, 3, generator=g, dtype=torch.float64)
        scene = R.place_scene(P, jp, 5)[None]
        tracks = TR.place_tracks(P, jp, 5, seed=2, T=T)[None]
    Gx, Gz, yaw = (5, 3, 0.4) if kind in ("yaw", "all") else (4, 4, 0.0)
    grid, rec, shifts = G.place_terrain(P, jp, S, Gx, Gz, None, yaw, seed=1)
    dx, dz, below, above = G.line_distance(P, grid, rec, jp, S)
    assert shifts <= G.SHIFTS and min(dx, dz) >= 1e-4 and below > 0.05 and (S is None or above > 0.05), (dx, dz, below, above)
    assert all(v > 0 for v in G.outside_sides(P, grid, rec))  # joints beside the grid on every side
    if kind in ("yaw", "all"):
        assert float(rec[4]) != float(rec[5]) and float(rec[3]) != 0
    args = (grid[None], rec[None], jp[None], None if S is None else S[None], scene, tracks, tg, w)
    loss, grad = G.ref_terrain_loss_grad(x, [T - 1], mean, std, *args)
    assert float(loss[0]) > 0 and float(grad.abs().max()) > 0
    if kind != "all":  # the term by hand, and terrain_height against the restatement
        e = P[..., 1] - MS.terrain_height(MS.Terrain(grid.float(), rec), P[..., [0, 2]])
        d = rec[7] - e
        want = rec[6] * (d.clamp(min=0) ** 2 + (0 if S is None else S[:T - 1]) * (-d).clamp(min=0) ** 2).sum()
        assert float(loss[0]) == pytest.approx(float(want), rel=1e-12)
    D = 3 * J + 1
    assert torch.equal(grad[0, :, D:], torch.zeros(T, F - D, dtype=torch.float64))
    assert torch.equal(grad[0, T - 1], torch.zeros(F, dtype=torch.float64))  # past the length
    h = 1e-6
    rng = np.random.RandomState(1)
    picks = [(t, c) for t in range(T - 1) for c in (0, 1, 2, 3)] + [(int(rng.randint(T - 1)), int(rng.randint(4, D)))
                                                                     for _ in range(16)]
    for t, c in picks:
        xp, xm = x.clone(), x.clone()
        xp[0, t, c] += h
        xm[0, t, c] -= h
        lp, _ = G.ref_terrain_loss_grad(xp, [T - 1], mean, std, *args)
        lm, _ = G.ref_terrain_loss_grad(xm, [T - 1], mean, std, *args)
        fd = float((lp - lm) / (2 * h))
        assert abs(fd - float(grad[0, t, c])) <= 1e-6 * max(1.0, abs(fd)), (kind, t, c, fd, float(grad[0, t, c]))


def test_stand_weight_one_makes_the_two_terms_a_square():
    x, mean, std = _case(T, 263, seed=4)
    P = ref_positions(x[0], mean, std).detach()
    jp = torch.zeros(22, 2, dtype=torch.float64)
    jp[:, 0], jp[:, 1] = 0.05, 1.0
    grid, rec, _ = G.place_terrain(P, jp, torch.ones(T, 22, dtype=torch.float64), 4, 4, None, 0.2, seed=2)
    e = G.clearance(P, grid, rec)
    want = float((rec[6] * (e - 0.05 - rec[7]) ** 2).sum())
    assert float(G.terrain_loss(P, grid, rec, jp, torch.ones(T, 22, dtype=torch.float64))) == pytest.approx(want, rel=1e-12)
    assert float(G.terrain_loss(P, grid, rec, jp)) < want


# ---- penetration --------------------------------------------------------------------------------------------------------
def test_penetration_with_a_terrain_on_hand_placed_joints():
    MS = pkg("motion_scene")
    J = 22
    joints = torch.zeros(2, 4, J, 3)
    joints[..., 1] = 1.0                    # every joint at height 1 ...
    joints[:, :, :, 0] = torch.tensor([-1.0, 0.5, 1.5, 3.0])[None, :, None]  # ... walking up a ramp that rises 2 m over 2 m
    ground = MS.ramp((0.0, 0.0), 0.0, 2.0, 2.0, 4.0, margin=0.1)  # heights under the four frames: 0, 0.5, 1.5, 2
    depth, share = MS.penetration(joints, [3, 4], None, terrain=ground)
    assert depth.tolist() == pytest.approx([0.5, 1.0]) and share.tolist() == pytest.approx([1 / 3, 2 / 4])
    depth, share = MS.penetration(joints, [3, 4], None, [0.1] * J, terrain=ground)
    assert depth.tolist() == pytest.approx([0.6, 1.1])
    # a margin counts for the share, not for the depth
    near = MS.ramp((0.0, 0.0), 0.0, 2.0, 2.0, 4.0, margin=0.6)
    depth, share = MS.penetration(joints, [3, 4], None, terrain=near)
    assert depth.tolist() == pytest.approx([0.5, 1.0]) and share.tolist() == pytest.approx([2 / 3, 3 / 4])
    # next to a static scene and tracks: the deepest of them, a frame counts once; one terrain per sample
    flat = MS.heightfield(np.zeros((2, 2)), 1.0)
    depth, share = MS.penetration(joints, [3, 4], [MS.floor(1.2)], terrain=[flat, ground])
    assert depth.tolist() == pytest.approx([0.2, 1.0]) and share.tolist() == [1.0, 1.0]
    quiet = MS.ramp((0.0, 0.0), 0.0, 2.0, 2.0, 4.0, weight=0.0)
    assert MS.penetration(joints, [3, 4], None, terrain=quiet)[0].tolist() == [0.0, 0.0]
    assert MS.penetration(joints, [3, 4], [MS.floor(0.0)])[0].tolist() == [0.0, 0.0]  # without a terrain: as before


# ---- the library, without a GPU -----------------------------------------------------------------------------------------
def test_argument_validation_without_gpu():
    """The five new entries reject bad arguments before touching the device (1 = MDM_ERR_ARG): fake non-null pointers stand
    in for device memory, as nothing is launched."""
    L = pkg("_lib")
    lib = L.lib()
    assert L.TERRAIN_MAX_GRID == 512 and L.TERRAIN_REC == 8
    p, odd = C.c_void_p(0x1000), C.c_void_p(0x1004)
    i, f = C.c_int32, C.c_float

    def lg(terrain=p, rec=p, Gx=4, Gz=4, stand=None, tracks=None, Km=0, K=0, jp=p, T=8, F=263, x0=p):
        return lib.mdm_joint_terrain_loss_grad(x0, p, p, p, None, None, None, i(K), jp, tracks, i(Km), None, terrain, rec, i(Gx),
                                               i(Gz), stand, i(0), i(T), i(F), p, p, None)

    def gd(terrain=p, rec=p, Gx=4, Gz=4, stand=None, iters=1, coef=p, steps=10, t=0, T=8):
        return lib.mdm_joint_terrain_guidance(p, p, None, p, p, p, None, None, None, i(0), p, None, i(0), None, terrain, rec, i(Gx),
                                              i(Gz), stand, i(0), i(T), i(263), f(0.1), i(iters), coef, i(steps), None, i(t), None)

    def clg(terrain=p, rec=p, Gx=4, Gz=4, stand=None, ws=p, F=263):
        return lib.mdm_canvas_terrain_loss_grad(p, p, p, p, p, None, None, None, i(0), p, None, i(0), None, terrain, rec, i(Gx),
                                                i(Gz), stand, i(0), i(F), p, p, ws, None)

    def cgd(terrain=p, rec=p, Gx=4, Gz=4, stand=None, iters=1, ws=p):
        return lib.mdm_canvas_terrain_guidance(p, p, None, p, p, p, p, None, None, None, i(0), p, None, i(0), None, terrain, rec,
                                               i(Gx), i(Gz), stand, i(0), i(263), f(0.1), i(iters), p, i(10), None, i(0), ws, None)

    for call in (lg, gd, clg, cgd):
        assert call() == 0  # B / M == 0: accepted, nothing launched
        for kw in (dict(Gx=1), dict(Gz=1), dict(Gx=513), dict(Gz=513), dict(Gx=0, Gz=0), dict(rec=None), dict(rec=odd),
                   dict(rec=C.c_void_p(0x1008)), dict(terrain=C.c_void_p(0x1002)), dict(stand=C.c_void_p(0x1001))):
            assert call(**kw) == 1, (call.__name__, kw)
        assert call(Gx=2, Gz=512, stand=odd) == 0
    # what the tracks calls refuse stays refused; a NULL terrain is the tracks call, the other terrain arguments not looked at
    assert lg(tracks=odd, Km=1) == 1 and lg(Km=25, tracks=p) == 1 and lg(K=17) == 1 and lg(jp=None) == 1 and lg(x0=None) == 1
    assert lg(T=0) == 1 and lg(F=262) == 1 and lg(T=lib.mdm_joint_scene_max_frames(263, 0) + 1) == 1
    assert gd(iters=0) == 1 and gd(iters=L.CONTROL_MAX_ITERS + 1) == 1 and gd(coef=None) == 1 and gd(t=10) == 1 and gd(steps=0) == 1
    assert clg(ws=None) == 1 and clg(F=100) == 1 and cgd(ws=None) == 1 and cgd(iters=0) == 1
    for call in (lg, gd, clg, cgd):
        assert call(terrain=None, rec=None, Gx=0, Gz=0) == 0
    assert lg(terrain=None, jp=None) == 1 and lg(terrain=None, tracks=odd, Km=1) == 1

    feet = (C.c_int32 * 4)(7, 10, 8, 11)

    def sw(x0=p, n=0, mean=p, std=p, F=263, ft=feet, thr=0.5, out=p, group=0):
        return lib.mdm_terrain_stand_weights(x0, None, i(n), mean, std, i(F), i(group), ft, f(thr), out, None)

    assert sw() == 0
    for kw in (dict(x0=None), dict(mean=None), dict(std=None), dict(ft=None), dict(out=None), dict(n=-1), dict(F=262), dict(F=10),
               dict(thr=float("nan")), dict(thr=float("inf")), dict(ft=(C.c_int32 * 4)(7, 10, 8, 22)),
               dict(ft=(C.c_int32 * 4)(-1, 10, 8, 11)), dict(group=-1), dict(F=251, ft=(C.c_int32 * 4)(19, 20, 14, 21))):
        assert sw(**kw) == 1, kw  # the last: the 21-joint skeleton has no joint 21
    assert sw(F=251) == 0 and sw(group=196) == 0  # joints 7, 10, 8, 11 exist at 21 joints as well


# ---- model kwargs -------------------------------------------------------------------------------------------------------
def _kw(B=2, n=8, F=263, targets=False, scene=False, stand=None):
    MS = pkg("motion_scene")
    J = (F + 1) // 12
    hs, rec = MS.batch_terrain([MS.stairs((0, 0), 0.1 * b, 2 + b, 0.2, 0.3, 1.0, cell=0.1) for b in range(B)], B)
    kw = {"control_mean": torch.zeros(B, F), "control_std": torch.ones(B, F), "control_scale": 0.5, "control_iters": 3,
          "control_terrain": hs, "control_terrain_rec": rec}
    if stand is not None:
        kw["control_stand"] = stand
    if scene:
        kw.update(control_scene=MS.batch_scene([MS.floor(), MS.sphere((0, 1, 0), 0.3)], B),
                  control_joint_params=MS.joint_params(J, 0.05)[None].expand(B, -1, -1))
    if targets:
        kw.update(control_joints=torch.zeros(B, n, J, 3), control_weights=torch.ones(B, n))
    return kw


def test_check_control_kwargs_accepts_a_terrain():
    D, MF = pkg("diffusion"), pkg("motion_features")
    c = D.check_control_kwargs(_kw(), (2, 8, 263))  # a terrain alone: no scene, no tracks, no targets, still mean and std
    assert c["targets"] is None and c["terrain"].shape == (2, 2, 10) and c["terrain_rec"].shape == (2, 8)
    assert c["scene"].shape == (2, 0, 12) and c["joint_params"][0, 0].tolist() == [0.0, 1.0] and c["iters"] == 3
    assert "stand" not in c and "stand_feet" not in c and "tracks" not in c
    c = D.check_control_kwargs(_kw(targets=True, scene=True, stand=torch.rand(2, 8, 22)), (2, 8, 263))
    assert c["targets"].shape == (2, 8, 22, 3) and c["scene"].shape == (2, 2, 12) and c["stand"].shape == (2, 8, 22)
    c = D.check_control_kwargs(dict(_kw(stand="contacts"), control_stand_threshold=0.4), (2, 8, 263))
    assert c["stand_feet"] == tuple(MF.SKELETONS["t2m"].feet) and c["stand_threshold"] == 0.4 and "stand" not in c
    c = D.check_control_kwargs(_kw(F=251, stand="contacts"), (2, 8, 251))
    assert c["stand_feet"] == tuple(MF.SKELETONS["kit"].feet) and c["stand_threshold"] == 0.5
    plain = {k: v for k, v in _kw(targets=True).items() if not k.startswith("control_terrain")}
    assert "terrain" not in D.check_control_kwargs(plain, (2, 8, 263))
    assert D.check_control_kwargs(_kw(n=202), (2, 202, 263)) is not None  # the T limit is the scene's


def _bad_rec(col, v):
    r = _kw()["control_terrain_rec"].clone()
    r[1, col] = v
    return r


@pytest.mark.parametrize("change", [
    dict(control_mean=None), dict(control_std=None), dict(control_terrain_rec=None), dict(control_terrain=None),
    dict(control_terrain=None, control_terrain_rec=None, control_stand=torch.zeros(2, 8, 22)),
    dict(control_terrain=torch.zeros(2, 1, 10)), dict(control_terrain=torch.zeros(2, 2, 513)), dict(control_terrain=torch.zeros(3, 2, 10)),
    dict(control_terrain=torch.zeros(2, 10)), dict(control_terrain=torch.full((2, 2, 10), float("nan"))),
    dict(control_terrain=torch.zeros(2, 2, 10, dtype=torch.int64)), dict(control_terrain_rec=torch.zeros(2, 7)),
    dict(control_terrain_rec=_bad_rec(4, 0.0)), dict(control_terrain_rec=_bad_rec(5, -1.0)), dict(control_terrain_rec=_bad_rec(6, -0.5)),
    dict(control_terrain_rec=_bad_rec(0, float("inf"))), dict(control_stand=torch.zeros(2, 8, 21)), dict(control_stand=torch.zeros(2, 7, 22)),
    dict(control_stand=torch.full((2, 8, 22), -1.0)), dict(control_stand=torch.full((2, 8, 22), float("nan"))),
    dict(control_stand="feet"), dict(control_stand="contacts", control_stand_threshold=float("nan")),
    dict(control_stand_threshold=0.5), dict(control_stand=torch.zeros(2, 8, 22), control_stand_threshold=0.5),
    dict(control_weights=torch.ones(2, 8)), dict(control_scale=float("nan")), dict(control_iters=0),
])
def test_check_control_kwargs_terrain_errors(change):
    D = pkg("diffusion")
    kw = {k: v for k, v in dict(_kw(), **change).items() if v is not None}
    with pytest.raises(ValueError):
        D.check_control_kwargs(kw, (2, 8, 263))


def test_terrain_frame_limit_and_the_long_motion_refusals():
    D, MS = pkg("diffusion"), pkg("motion_scene")
    with pytest.raises(ValueError, match="at most"):
        D.check_control_kwargs(_kw(n=225), (2, 225, 263))
    with pytest.raises(ValueError, match="contacts"):
        D.check_control_kwargs(dict(_kw(F=23, stand="contacts")), (2, 8, 23))  # no skeleton of two joints
    hs = {"handshake_offsets": torch.tensor([0, 2]), "handshake_rows": torch.tensor([0, 8]), "handshake_weights": torch.ones(2),
          "handshake_owner_rows": torch.tensor([0, 8])}
    with pytest.raises(NotImplementedError, match="per-window joint control"):
        D.check_handshake_kwargs(dict(_kw(), **hs), (2, 8, 263))


def test_shard_kwargs_gives_each_rank_its_rows():
    Dist = pkg("dist")
    kw = _kw(B=5, scene=True, stand=torch.rand(5, 8, 22))
    for lo, hi in ((0, 3), (3, 5)):
        s = Dist.shard_kwargs(kw, lo, hi)
        for k in ("control_terrain", "control_terrain_rec", "control_stand", "control_scene", "control_mean"):
            assert torch.equal(s[k], kw[k][lo:hi]), k
        c = pkg("diffusion").check_control_kwargs(s, (hi - lo, 8, 263))
        assert c["terrain"].shape == (hi - lo, 2, 19) and torch.equal(c["stand"], kw["control_stand"][lo:hi])
    s = Dist.shard_kwargs(dict(_kw(B=5), control_stand="contacts"), 1, 4)
    assert s["control_stand"] == "contacts" and s["control_terrain"].shape == (3, 2, 19)


# ---- trainer arguments --------------------------------------------------------------------------------------------------
def test_trainer_terrain_arguments():
    import types
    Cond, MS = pkg("conditioning").Conditioning, pkg("motion_scene")
    caps = ["a", "b", "c"]
    mean, std = np.zeros(263, np.float32), np.ones(263, np.float32)
    up = MS.stairs((0.5, 0.0), 0.0, 4, 0.18, 0.28, 1.2, margin=0.02)
    c = Cond(caps, 263, terrain=up, mean=mean, std=std, control_scale=0.3)
    kw = c.control_kwargs(slice(1, 3), 6, "cpu")  # a batch takes its rows
    assert "control_joints" not in kw and "control_stand" not in kw and "control_tracks" not in kw
    assert kw["control_terrain"].shape == (2,) + tuple(up.heights.shape) and kw["control_scene"].shape == (2, 0, 12)
    assert torch.equal(kw["control_terrain"][1], up.heights) and kw["control_terrain_rec"][0].tolist() == up.record.float().tolist()
    assert pkg("diffusion").check_control_kwargs(kw, (2, 6, 263))["terrain"].shape[0] == 2 and kw["control_scale"] == 0.3
    per = [up, MS.ramp((0, 0), 0.3, 2.0, 0.5, 1.0), MS.heightfield(np.zeros((3, 3)), 0.5)]
    c = Cond(caps, 263, terrain=per, terrain_stand="contacts", terrain_stand_threshold=0.4, scene=[MS.floor()],
             scene_joint_radius=[0.1] * 22, mean=mean, std=std, control_joints=torch.zeros(3, 10, 22, 3), control_weights=torch.ones(3))
    kw = c.kwargs(torch.tensor([2, 0]), 10, "cpu")
    assert kw["control_terrain"].shape == (2, 3, up.heights.shape[1]) and kw["control_scene"].shape == (2, 1, 12)
    assert kw["control_stand"] == "contacts" and kw["control_stand_threshold"] == 0.4
    assert float(kw["control_joint_params"][1, 21, 0]) == pytest.approx(0.1)
    assert pkg("diffusion").check_control_kwargs(kw, (2, 10, 263))["stand_threshold"] == 0.4
    st = torch.rand(3, 10, 22)
    c = Cond(caps, 263, terrain=up, terrain_stand=st, mean=mean, std=std)
    kw = c.control_kwargs(slice(0, 2), 6, "cpu")
    assert torch.equal(kw["control_stand"], st[:2, :6])
    with pytest.raises(ValueError, match="terrain_stand has 10 frames"):
        c.control_kwargs(slice(0, 2), 12, "cpu")
    # without a terrain the kwargs are what they were
    assert not any("terrain" in k or "stand" in k for k in Cond(caps, 263, scene=[MS.floor()], mean=mean, std=std).kwargs(slice(0, 3), 6, "cpu"))
    for bad in (dict(terrain=up), dict(terrain=up, mean=mean), dict(terrain=per[:2], mean=mean, std=std),
                dict(terrain=up, terrain_stand="feet", mean=mean, std=std), dict(terrain_stand="contacts", mean=mean, std=std),
                dict(terrain=up, terrain_stand=torch.zeros(3, 10, 21), mean=mean, std=std),
                dict(terrain=up, terrain_stand=torch.zeros(2, 10, 22), mean=mean, std=std), dict(terrain=[up, up, "x"], mean=mean, std=std)):
        with pytest.raises(ValueError):
            Cond(caps, 263, **bad)
    Tr = pkg("trainer")
    tr = Tr.DDPMTrainer.__new__(Tr.DDPMTrainer)  # the checks run before anything touches a device
    tr.encoder, tr.device = types.SimpleNamespace(num_frames=16, eval=lambda: None), "cpu"
    lens = torch.tensor([16, 12, 8])
    for method in (tr.generate_batch, tr.generate, tr.generate_bucketed):
        with pytest.raises(ValueError, match="mean and std"):
            method(caps, lens, 263, terrain=up)
        with pytest.raises(ValueError, match="one terrain"):
            method(caps, lens, 263, terrain=per[:2], mean=mean, std=std)
    with pytest.raises(ValueError, match="terrain_stand"):  # through an output method's **kw
        tr.generate_joints(caps, lens, 263, mean, std, terrain=up, terrain_stand="feet")


# ---- long motions -------------------------------------------------------------------------------------------------------
def test_check_canvas_control_kwargs_with_a_terrain():
    D, MS, MF = pkg("diffusion"), pkg("motion_scene"), pkg("motion_features")
    B, n, F, J = 1, 8, 263, 22
    hs, rec = MS.batch_terrain([MS.stairs((0, 0), 0.2, 3, 0.2, 0.3, 1.0, cell=0.1)], 1)
    base = {"canvas_control_offsets": torch.tensor([0, 6]), "canvas_control_rows": torch.arange(6),
            "canvas_control_mean": torch.zeros(1, F), "canvas_control_std": torch.ones(1, F), "canvas_control_terrain": hs,
            "canvas_control_terrain_rec": rec}
    c = D.check_canvas_control_kwargs(base, (B, n, F))  # a terrain alone: no scene, no tracks, no targets
    assert c["targets"] is None and c["scene"].shape == (1, 0, 12) and c["terrain"].shape == (1, 2, 10) and c["total"] == 6
    assert c["terrain_rec"].shape == (1, 8) and c["joint_params"].shape == (1, J, 2) and "stand" not in c and "stand_feet" not in c
    both = dict(base, canvas_control_joints=torch.zeros(6, J, 3), canvas_control_weights=torch.ones(6),
                canvas_control_scene=MS.batch_scene([MS.floor()], 1), canvas_control_stand=torch.rand(6, J))
    c = D.check_canvas_control_kwargs(both, (B, n, F))
    assert c["targets"].shape == (6, J, 3) and c["scene"].shape == (1, 1, 12) and c["stand"].shape == (6, J)
    c = D.check_canvas_control_kwargs(dict(base, canvas_control_stand="contacts", canvas_control_stand_threshold=0.3), (B, n, F))
    assert c["stand_feet"] == tuple(MF.SKELETONS["t2m"].feet) and c["stand_threshold"] == 0.3
    assert D.check_control_kwargs(dict(base, control_scale=0.1), (B, n, F)) is None  # the scale is the canvas control's
    bad_rec = rec.clone()
    bad_rec[0, 4] = 0.0
    for change in (dict(canvas_control_mean=None), dict(canvas_control_rows=None), dict(canvas_control_terrain_rec=None),
                   dict(canvas_control_terrain=None), dict(canvas_control_terrain=None, canvas_control_terrain_rec=None,
                                                           canvas_control_stand="contacts"),
                   dict(canvas_control_terrain=torch.zeros(2, 2, 10)), dict(canvas_control_terrain=torch.zeros(1, 1, 10)),
                   dict(canvas_control_terrain=torch.zeros(1, 2, 513)), dict(canvas_control_terrain=torch.zeros(2, 10)),
                   dict(canvas_control_terrain=torch.full((1, 2, 10), float("inf"))), dict(canvas_control_terrain_rec=torch.zeros(1, 7)),
                   dict(canvas_control_terrain_rec=bad_rec), dict(canvas_control_stand=torch.zeros(5, J)),
                   dict(canvas_control_stand=torch.zeros(1, 6, J)), dict(canvas_control_stand=torch.full((6, J), -1.0)),
                   dict(canvas_control_stand="feet"), dict(canvas_control_stand_threshold=0.5),
                   dict(canvas_control_stand="contacts", canvas_control_stand_threshold=float("inf")),
                   dict(control_terrain=torch.zeros(1, 2, 2), control_terrain_rec=rec)):
        kw = {k: v for k, v in dict(base, **change).items() if v is not None}
        with pytest.raises(ValueError):
            D.check_canvas_control_kwargs(kw, (B, n, F))
    with pytest.raises(ValueError, match="contacts"):
        D.check_canvas_control_kwargs(dict({k: (v[:, :23] if k.endswith(("mean", "std")) else v) for k, v in base.items()},
                                           canvas_control_stand="contacts"), (B, n, 23))  # no skeleton of two joints
    with pytest.raises(ValueError, match="whole long motions"):
        pkg("dist").shard_kwargs(base, 0, 1)


def test_canvas_control_takes_a_terrain_per_motion():
    import types
    ML, MS = pkg("motion_long"), pkg("motion_scene")
    plans = ML.script_plans([[("a", 16), ("b", 12)], [("c", 10)]], 4, 16)
    mean, std = np.zeros(263, np.float32), np.ones(263, np.float32)
    grounds = [MS.stairs((0.5, 0.0), 0.0, 4, 0.18, 0.28, 1.2), MS.ramp((0, 0), 0.3, 2.0, 0.5, 1.0)]
    tables = ML.canvas_control(plans, 263, mean=mean, std=std, terrain=grounds, terrain_stand="contacts", terrain_stand_threshold=0.4,
                               scene_joint_radius=[0.1] * 22, control_iters=2)
    kw = tables([1, 0], 16)
    assert "canvas_control_joints" not in kw and "canvas_control_tracks" not in kw and kw["control_iters"] == 2
    assert kw["canvas_control_terrain"].shape == (2, 2, grounds[0].heights.shape[1]) and kw["canvas_control_terrain_rec"].shape == (2, 8)
    assert kw["canvas_control_terrain_rec"][0].tolist() == grounds[1].record.float().tolist()  # motion 1 comes first
    assert kw["canvas_control_stand"] == "contacts" and kw["canvas_control_stand_threshold"] == 0.4
    assert kw["canvas_control_scene"].shape == (2, 0, 12) and float(kw["canvas_control_joint_params"][0, 3, 0]) == pytest.approx(0.1)
    full = dict(kw, **ML.batch_tables(plans, [1, 0], 16, 4), length=torch.tensor([10, 16, 12]))
    c = pkg("diffusion").check_canvas_control_kwargs(full, (3, 16, 263))
    assert c["targets"] is None and c["terrain"].shape[0] == 2 and c["stand_threshold"] == 0.4 and c["total"] == 34
    given = [torch.rand(24, 22), torch.rand(10, 22)]
    kw = ML.canvas_control(plans, 263, mean=mean, std=std, terrain=grounds, terrain_stand=given)([1, 0], 16)
    assert torch.equal(kw["canvas_control_stand"], torch.cat([given[1], given[0]])) and "canvas_control_stand_threshold" not in kw
    assert tables([1], 16)["canvas_control_terrain"].shape[0] == 1
    assert ML.canvas_control(plans, 263)([0], 16) == {}  # without a terrain: what it was
    for bad in (dict(terrain=grounds), dict(terrain=grounds, mean=mean), dict(terrain=grounds[0], mean=mean, std=std),
                dict(terrain=grounds[:1], mean=mean, std=std), dict(terrain=[grounds[0], None], mean=mean, std=std),
                dict(terrain=grounds, terrain_stand="feet", mean=mean, std=std), dict(terrain_stand="contacts", mean=mean, std=std),
                dict(terrain=grounds, terrain_stand=given[:1], mean=mean, std=std),
                dict(terrain=grounds, terrain_stand=[given[0], torch.rand(9, 22)], mean=mean, std=std),
                dict(terrain=grounds, terrain_stand=torch.rand(2, 24, 22), mean=mean, std=std)):
        with pytest.raises(ValueError):
            ML.canvas_control(plans, 263, **bad)
    Tr = pkg("trainer")
    tr = Tr.DDPMTrainer.__new__(Tr.DDPMTrainer)  # the checks run before anything touches a device
    tr.encoder, tr.device = types.SimpleNamespace(num_frames=16, eval=lambda: None), "cpu"
    with pytest.raises(ValueError, match="one terrain per motion"):
        tr.generate_long([[("a", 16)]], 263, overlap=4, terrain=grounds[0], mean=mean, std=std)
    with pytest.raises(ValueError, match="mean and std"):
        tr.generate_long([[("a", 16)]], 263, overlap=4, terrain=grounds[:1])
    with pytest.raises(ValueError, match="terrain_stand"):
        tr.generate_long([[("a", 16)]], 263, overlap=4, terrain=grounds[:1], terrain_stand="feet", mean=mean, std=std)

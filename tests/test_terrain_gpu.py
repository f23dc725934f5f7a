"""GPU: terrain: a height-map ground joints stay above and planted feet stand on, next to the scene of §24 and
the tracks of §25.

* mdm_joint_terrain_loss_grad against the fp64 autograd restatement of tests/terrain_ref.py: (B, T) = (1, 2) and (3, 40) at
  F = 263 and 251, (2, 196) at F = 263, ragged lengths with 0 and 1, each on four grids: 2 x 2 (the smallest: the i = Gx - 2
  clamp acts), 3 x 5 with cell_x != cell_z and yaw 0.4 (a transposed axis or an un-turned gradient shows), 512 x 512 with
  cells of 0.5 m; terrain only / with fractional stand weights S / with joint weights that include zeros and non-zero radii /
  with a static scene, tracks and fractional target weights.  The grids are placed from the reference's own positions, and the
  test asserts that placement on the reference alone before it looks at the kernel: every penalised joint >= LINE_CLEAR from a
  grid line and a clamp edge along x and z, each term penalising >= 5 % of (t, j) in some sample, joints beside the 2 x 2 and
  3 x 5 grids past every one of their four edges in every sample (a 512 x 512 grid of 0.5 m cells is 255 m wide, wider than
  any test motion: its low corner stands at the motion's median, so joints lie beside it past two edges and over it; a
  fourth grid, the same with its high corner at the median, puts joints past the two high edges and over the last cells, where
  the i = Gx - 2 clamp acts at Gx = 512; it runs at T = 2 and 40).
  LINE_CLEAR = 20 x 6.853e-6 m = 1.371e-4 m: 6.853e-6 m is the largest difference of the reference positions computed in fp32
  and in fp64 on these inputs, measured on the CPU (python tests/terrain_ref.py).  A placement that does not clear within 20
  origin shifts fails the test.  Gates are §14's: loss rel <= 1e-5, gradient rel_inf <= 1e-4, exact zeros;
* bitwise: a NULL terrain is mdm_joint_tracks_loss_grad / _guidance; a terrain of weight 0, and one no joint touches with
  S = 0, leave x and x0 (-0.0 included); masked entries keep their bits;
* to the gates: a flat grid at height c with S = 0 is floor(c) of the same weight and margin; a grid turned by a yaw with its
  heights counter-rotated is the unrotated one;
* the guidance kernel's single step, its update of x and k iterations = k chained steps; the argument errors;
* mdm_terrain_stand_weights against its torch restatement, exactly, contact columns kept >= 0.05 from the threshold;
* the canvas kernel: two motions of 300 and 700 frames through shuffled rows against the restatement at §23's gates, and a
  40-frame canvas against the window kernel; the Python entries;
* loops: cfg_dpmpp and ddim eta = 0.5 with a terrain, control_stand="contacts", §24's loop scene and a root path against the
  loop restated in tests/sampler_ref.py with the autograd guidance, teacher-forced, <= 1e-4 per step, one with an edit mask;
  graph == eager bitwise; the trainer's batch split, bucketing and joints front end with terrain= / terrain_stand=;
* the canvas guidance kernel, with and without an edit mask, on the two shuffled motions and on a 40-frame canvas with
  tracks: single step, update of x, untouched rows, k iterations, NULL stand and balls, weight 0 and an untouched ground;
* a long motion of two windows at overlap 20 with terrain=, terrain_stand="contacts", a scene and a root path against the
  restated canvas loop, <= 1e-4 per step, once with an edit mask, graph == eager; generate_long(terrain=) over batch splits;
* behaviour: a ramp that rises along a pelvis path: the terrain cuts L_terrain of the final sample.
"""
import ctypes as C
import functools
import math

import pytest
import torch

from conftest import pkg, rel_inf
from test_motion_control_host import ref_positions

import scene_tracks_ref as TR
import terrain_ref as G
from sampler_ref import make_diffusion as _diffusion, vp as _vp
from test_motion_scene_gpu import _case as _scene_case, _scene_lg
from test_scene_tracks_gpu import _bits, _cu, _tracks_lg

pytestmark = pytest.mark.gpu

VARIANTS = ("terrain", "stand", "joints", "all")
SHAPES = [(1, 2, 263), (1, 2, 251), (3, 40, 263), (3, 40, 251), (2, 196, 263)]
# name -> (Gx, Gz, cells or None (0.8 of the positions' spread: joints beside the grid on every side), yaw, low corner at the median)
GRIDS = {"2x2": (2, 2, None, 0.0, False), "3x5": (5, 3, None, 0.4, False), "512": (512, 512, (0.5, 0.5), 0.0, True),
         "512hi": (512, 512, (0.5, 0.5), 0.0, "high")}


@functools.lru_cache(maxsize=None)
def _placed_tracks(B, T, F):
    """Five tracks per sample that follow the reference's positions (tests/scene_tracks_ref.py), shared by the grids."""
    c = _scene_case(B, T, F, 5, "targets")
    return torch.stack([TR.place_tracks(c["P"][b], c["jp"][b], 5, seed=2 + b, T=T) for b in range(B)]).float()


@functools.lru_cache(maxsize=None)
def _case(B, T, F, grid, variant):
    """The draws of test_motion_scene_gpu._case (x0, mean, std, lengths with 0 and 1) and a terrain per sample placed from
    the reference's positions.  "terrain": S NULL; "stand": fractional S with zeros; "joints": joint weights with zeros and
    non-zero radii, with S; "all": S, the static scene of that case, five tracks and fractional target weights.  Shared by the
    tests, left unchanged."""
    J = (F + 1) // 12
    c = dict(_scene_case(B, T, F, 5, "targets" if variant == "all" else "scene"))
    gen = torch.Generator().manual_seed(B + T + F + len(grid))
    if variant == "joints":
        jp = torch.zeros(B, J, 2)
        jp[..., 1] = torch.rand(B, J, generator=gen) * 2
        jp[..., 1][torch.rand(B, J, generator=gen) < 0.15] = 0.0
        jp[..., 0] = torch.rand(B, J, generator=gen) * 0.15
        c["jp"] = jp
    S = None
    if variant != "terrain":
        S = torch.rand(B, T, J, generator=gen) * 1.5
        S[S < 0.45] = 0.0
    c["S"] = S
    c["scene"] = c["scene"] if variant == "all" else None
    c["tracks"] = None
    if variant == "all":
        c["tracks"] = _placed_tracks(B, T, F)
    else:
        c["tg"] = c["w"] = None
    Gx, Gz, cell, yaw, corner = GRIDS[grid]
    placed = [G.place_terrain(c["P"][b], c["jp"][b], None if S is None else S[b], Gx, Gz, cell, yaw, seed=7 + b, corner=corner)
              for b in range(B)]
    c["grid"], c["rec"] = torch.stack([p[0] for p in placed]).float(), torch.stack([p[1] for p in placed]).float()
    c["shifts"] = [p[2] for p in placed]
    c["lines"] = [G.line_distance(c["P"][b], c["grid"][b], c["rec"][b], c["jp"][b], None if S is None else S[b]) for b in range(B)]
    c["sides"] = [G.outside_sides(c["P"][b], c["grid"][b], c["rec"][b]) for b in range(B)]
    c["ref"] = G.ref_terrain_loss_grad(c["x0"], c["lens"], c["mean"], c["std"], c["grid"], c["rec"], c["jp"], S, c["scene"],
                                       c["tracks"], c["tg"], c["w"])
    return c


def _terrain_lg(x0, lens, mean, std, jp, grid, rec, S=None, scene=None, tracks=None, bounds=None, tg=None, w=None, dims=None):
    """mdm_joint_terrain_loss_grad on packed arguments: grid (B, Gz, Gx) or None, rec (B, 8), S (B, T, J) or None, scene
    (B, K, 12) or None, tracks (B, T, Km, 12) or None."""
    L = pkg("_lib")
    B, T, F = x0.shape
    dev = [_cu(v) for v in (x0, mean, std, tg, w, scene, jp, tracks, bounds, grid, rec, S)]
    ln = lens.cuda().to(torch.int32)
    loss, grad = torch.empty(B, device="cuda"), torch.empty(B, T, F, device="cuda")
    K, Km = (0 if scene is None else scene.shape[1]), (0 if tracks is None else tracks.shape[2])
    Gz, Gx = (0, 0) if grid is None else grid.shape[1:]
    Gx, Gz = (Gx, Gz) if dims is None else dims
    L.check(L.lib().mdm_joint_terrain_loss_grad(
        _vp(dev[0]), _vp(ln), _vp(dev[1]), _vp(dev[2]), _vp(dev[3]), _vp(dev[4]), _vp(dev[5] if K else None), C.c_int32(K),
        _vp(dev[6]), _vp(dev[7] if Km else None), C.c_int32(Km), _vp(dev[8]), _vp(dev[9]), _vp(dev[10]), C.c_int32(Gx),
        C.c_int32(Gz), _vp(dev[11]), C.c_int32(B), C.c_int32(T), C.c_int32(F), _vp(loss), _vp(grad), C.c_void_p(L.stream_ptr())))
    return loss.cpu(), grad.cpu()


def _case_lg(c, **over):
    a = dict(grid=c["grid"], rec=c["rec"], S=c["S"], scene=c["scene"], tracks=c["tracks"], tg=c["tg"], w=c["w"])
    a.update(over)
    return _terrain_lg(c["x0"], c["lens"], c["mean"], c["std"], c["jp"], **a)


# ---- mdm_joint_terrain_loss_grad ----------------------------------------------------------------------------------------
# every shape on the first three grids; the high-corner grid at T = 2 and 40, where the placement clears within 20 shifts for
# every variant (at T = 196, with 4312 joints and more of them over the grid after every shift, two variants do not: checked on
# the CPU; the 512 x 512 grid at T = 196 is the low-corner one)
LOSS_GRAD_CASES = [(*shape, grid) for shape in SHAPES for grid in GRIDS if not (grid == "512hi" and shape[1] > 40)]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("B,T,F,grid", LOSS_GRAD_CASES)
def test_terrain_loss_grad_matches_fp64_autograd(B, T, F, grid, variant):
    c = _case(B, T, F, grid, variant)
    D = 3 * ((F + 1) // 12) + 1
    # the placement, on the reference alone
    live = [b for b in range(B) if int(c["lens"][b]) > 0]
    dx, dz = min(c["lines"][b][0] for b in live), min(c["lines"][b][1] for b in live)
    below, above = max(c["lines"][b][2] for b in live), max(c["lines"][b][3] for b in live)
    print(f"[terrain B={B} T={T} F={F} {grid} {variant}] origin shifts {c['shifts']}, least distance to a line along x {dx:.2e} m, "
          f"along z {dz:.2e} m; share of (t, j) penalised (best sample): kept above {below:.3f}, pulled down {above:.3f}; joints "
          f"beside the grid (low x, high x, low z, high z) {[c['sides'][b] for b in live]}")
    assert max(c["shifts"]) <= G.SHIFTS, c["shifts"]
    assert min(dx, dz) >= G.LINE_CLEAR, (dx, dz)
    assert below >= 0.05 and (variant == "terrain" or above >= 0.05), (below, above)
    for b in live:
        # a 512 x 512 grid: past its two low edges, or ("512hi") past its two high ones (module docstring)
        need = (1, 3) if GRIDS[grid][4] == "high" else (0, 2) if GRIDS[grid][4] else (0, 1, 2, 3)
        assert all(c["sides"][b][k] > 0 for k in need), (b, c["sides"][b])
    if GRIDS[grid][4]:
        n0 = int(c["lens"][0]) * ((F + 1) // 12)
        assert all(c["sides"][0][k] < n0 for k in range(4))  # and joints over it
    loss, grad = _case_lg(c)
    rl, rg = c["ref"]
    worst_l = worst_g = 0.0
    for b in range(B):
        n = int(c["lens"][b])
        assert torch.equal(grad[b, :, D:], torch.zeros(T, F - D)), b
        assert torch.equal(grad[b, n:], torch.zeros(T - n, F)), b
        if n == 0:
            assert float(loss[b]) == 0.0
            continue
        assert float(rl[b]) > 0
        el = abs(float(loss[b]) - float(rl[b])) / float(rl[b])
        eg = rel_inf(grad[b], rg[b])
        worst_l, worst_g = max(worst_l, el), max(worst_g, eg)
        assert el <= 1e-5, (b, el)
        assert eg <= 1e-4, (b, n, eg)
    print(f"[terrain B={B} T={T} F={F} {grid} {variant}] worst loss rel {worst_l:.2e}, worst gradient rel_inf {worst_g:.2e}")


def test_python_entry_equals_the_packed_call():
    """motion_scene.scene_loss_grad(terrain=, stand=) on terrains made by the constructors: one shared, one per sample (padded
    to a common grid), with a scene and tracks; and terrain_height against the restatement."""
    MS = pkg("motion_scene")
    c = _case(3, 40, 263, "3x5", "stand")
    med = c["P"][0].reshape(-1, 3).median(0).values
    gen = torch.Generator().manual_seed(4)
    hts = float(med[1]) + 0.3 * torch.randn(4, 6, generator=gen)
    one = MS.heightfield(hts, (0.7, 0.45), (float(med[0]) - 1.6, float(med[2]) - 0.8), 0.3, margin=0.03, weight=1.25)
    hs, rec = MS.batch_terrain(one, 3)
    jp = MS.joint_params(22, [0.05] * 22, None)[None].expand(3, -1, -1)
    args = (c["x0"].cuda(), c["lens"], c["mean"], c["std"])
    loss, grad = MS.scene_loss_grad(*args, None, joint_radius=[0.05] * 22, terrain=one, stand=c["S"])
    l2, g2 = _terrain_lg(c["x0"], c["lens"], c["mean"], c["std"], jp, hs, rec, c["S"])
    assert torch.equal(loss.cpu(), l2) and torch.equal(grad.cpu(), g2) and float(l2[0]) > 0
    rl, rg = G.ref_terrain_loss_grad(c["x0"], c["lens"], c["mean"], c["std"], hs, rec, jp, c["S"])
    assert abs(float(l2[0]) - float(rl[0])) <= 1e-5 * float(rl[0])
    pts = c["P"][0].reshape(-1, 3)
    want = G.height(pts, one.heights.double(), one.record)
    assert float((MS.terrain_height(one, pts[:, [0, 2]]) - want).abs().max()) <= 1e-12
    # one per sample, padded by edge replication: sample 0 keeps its result
    per = [one, MS.ramp((float(med[0]), float(med[2])), 0.2, 2.0, 0.5, 3.0), MS.stairs((0, 0), 0.0, 3, 0.2, 0.3, 1.0)]
    l3, g3 = MS.scene_loss_grad(*args, None, joint_radius=[0.05] * 22, terrain=per, stand=c["S"])
    assert abs(float(l3[0]) - float(l2[0])) <= 1e-6 * float(l2[0]) and rel_inf(g3[0].cpu(), g2[0]) <= 1e-6
    # with a scene and tracks the three terms add up (to rounding)
    prims = [MS.sphere((0.3, 0.8, 0.2), 0.7, margin=0.05), MS.floor(0.1)]
    trk = [MS.moving_sphere(c["P"][0][:, 15].float() + torch.tensor([0.1, 0.0, 0.1]), 0.4, margin=0.05)]
    l4, g4 = MS.scene_loss_grad(*args, prims, joint_radius=[0.05] * 22, tracks=trk, terrain=one, stand=c["S"])
    l5, g5 = MS.scene_loss_grad(*args, prims, joint_radius=[0.05] * 22, tracks=trk)
    assert rel_inf(l4.cpu(), l5.cpu() + l2) <= 1e-5 and rel_inf(g4.cpu(), g5.cpu() + g2) <= 1e-5
    with pytest.raises(ValueError, match="stand"):
        MS.scene_loss_grad(*args, None, terrain=one, stand=c["S"][:, :39])


# ---- equivalences -------------------------------------------------------------------------------------------------------
def test_null_terrain_is_the_tracks_loss_grad_bitwise():
    c = _case(3, 40, 263, "3x5", "all")
    bounds = pkg("motion_scene").track_bounds(c["tracks"])
    loss, grad = _case_lg(c, grid=None, bounds=bounds)  # rec and S given, no grid: not looked at
    l0, g0 = _tracks_lg(c["x0"], c["lens"], c["mean"], c["std"], c["scene"], c["jp"], c["tracks"], bounds, c["tg"], c["w"])
    assert torch.equal(_bits(loss), _bits(l0)) and torch.equal(_bits(grad), _bits(g0)) and float(l0[0]) > 0
    # a terrain of weight 0 through the terrain instantiation: the same values up to fp32 rounding (another instantiation may
    # contract its products differently)
    off = c["rec"].clone()
    off[:, 6] = 0.0
    loss, grad = _case_lg(c, rec=off, bounds=bounds)
    assert rel_inf(loss, l0) <= 1e-6 and rel_inf(grad, g0) <= 1e-6
    # the broad phase's balls change no bit of the terrain instantiation either
    a, b = _case_lg(c, bounds=bounds), _case_lg(c)
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))
    # nothing that bites: zero
    loss, grad = _case_lg(c, rec=off, scene=None, tracks=None, tg=None, w=None)
    assert not loss.any() and not grad.any()


def test_a_flat_grid_is_the_floor():
    """A flat grid at height c with S = 0 against floor(c) of the same weight and margin through the scene entry, with radii."""
    MS = pkg("motion_scene")
    c = _case(3, 40, 263, "3x5", "joints")
    h = float(c["P"][0][..., 1].median())
    grid = torch.full((3, 4, 3), h)
    rec = c["rec"].clone()
    rec[:, 6], rec[:, 7] = 1.75, 0.04
    loss, grad = _case_lg(c, grid=grid, rec=rec, S=None)
    fl = MS.pack_scene([MS.floor(float(torch.tensor(h).float()), margin=0.04, weight=1.75)])[None].expand(3, -1, -1)
    l0, g0 = _scene_lg(c["x0"], c["lens"], c["mean"], c["std"], fl, c["jp"])
    assert float(l0[0]) > 0
    for b in (0, 2):
        assert abs(float(loss[b]) - float(l0[b])) <= 1e-5 * float(l0[b]), b
        assert rel_inf(grad[b], g0[b]) <= 1e-4, b
    assert float(loss[1]) == 0.0 and not grad[1].any()


def test_a_turned_grid_with_counter_rotated_heights_is_the_unrotated_one():
    """A quarter turn maps grid samples onto grid samples: the grid seen from its far-z corner, turned by pi / 2, has the
    flipped and transposed heights and the cells swapped, and gives the same heights everywhere."""
    c = _case(3, 40, 263, "3x5", "stand")
    grid, rec = c["grid"], c["rec"]  # (3, 3, 5), yaw 0.4
    gz, gx = grid.shape[1:]
    turned, trec = torch.zeros(3, gx, gz), rec.clone()
    for b in range(3):
        # new local x = (gz - 1) cell_z - old local z, new local z = old local x: sample [k', i'] = old [gz - 1 - i', k']
        turned[b] = grid[b].flip(0).t()
        cy, sy, cz = (float(v) for v in (rec[b, 2], rec[b, 3], 1 / rec[b, 5].double()))
        ext = (gz - 1) * cz
        trec[b, 0], trec[b, 1] = float(rec[b, 0]) + sy * ext, float(rec[b, 1]) + cy * ext  # origin + R_y(yaw) (0, 0, ext)
        yaw = math.atan2(sy, cy) + math.pi / 2
        trec[b, 2], trec[b, 3], trec[b, 4], trec[b, 5] = math.cos(yaw), math.sin(yaw), rec[b, 5], rec[b, 4]
    P = c["P"][0].reshape(-1, 3)
    assert float((G.height(P, turned[0].double(), trec[0].double()) - G.height(P, grid[0].double(), rec[0].double())).abs().max()) < 1e-5
    a, b = _case_lg(c), _case_lg(c, grid=turned, rec=trec)
    for s in (0, 2):
        assert abs(float(a[0][s]) - float(b[0][s])) <= 1e-5 * float(a[0][s]), s
        assert rel_inf(b[1][s], a[1][s]) <= 1e-4, s


def _guide(x, x0, mask, k, scale, iters, coef, steps, t, shape=None, dims=None, **over):
    L = pkg("_lib")
    a = dict(k)
    a.update(over)
    B, T, F = x0.shape if shape is None else shape
    K, Km = (0 if a["scene"] is None else k["scene"].shape[1]), (0 if a["tracks"] is None else k["tracks"].shape[2])
    Gz, Gx = (0, 0) if a["grid"] is None else a["grid"].shape[1:]
    Gx, Gz = (Gx, Gz) if dims is None else dims
    return L.lib().mdm_joint_terrain_guidance(
        _vp(x), _vp(x0), _vp(mask), _vp(a["lens"]), _vp(a["mean"]), _vp(a["std"]), _vp(a["tg"]), _vp(a["w"]), _vp(a["scene"]),
        C.c_int32(K), _vp(a["jp"]), _vp(a["tracks"]), C.c_int32(Km), _vp(a["bounds"]), _vp(a["grid"]), _vp(a["rec"]), C.c_int32(Gx),
        C.c_int32(Gz), _vp(a["S"]), C.c_int32(B), C.c_int32(T), C.c_int32(F), C.c_float(scale), C.c_int32(iters), _vp(coef),
        C.c_int32(steps), C.c_void_p(0), C.c_int32(t), C.c_void_p(L.stream_ptr()))


def _kernel_case(variant="all", grid="3x5", shape=(3, 40, 263)):
    c = _case(*shape, grid, variant)
    gen = torch.Generator().manual_seed(3)
    k = {n: _cu(c[n]) for n in ("mean", "std", "tg", "w", "scene", "jp", "tracks", "grid", "rec", "S")}
    k["bounds"] = None if c["tracks"] is None else _cu(pkg("motion_scene").track_bounds(c["tracks"]))
    k["lens"] = c["lens"].cuda().to(torch.int32)
    return c, k, torch.randn(*shape, generator=gen).cuda(), _cu(c["x0"])


def test_guidance_kernel_steps_and_update():
    L = pkg("_lib")
    d = _diffusion("ddim10")
    N = d.num_timesteps
    c, k, x, x0 = _kernel_case()
    lens, D = k["lens"], 67

    def grad_of(y, **over):
        a = dict(grid=c["grid"], rec=c["rec"], S=c["S"], scene=c["scene"], tracks=c["tracks"], tg=c["tg"], w=c["w"])
        a.update(over)
        return _terrain_lg(y, c["lens"], c["mean"], c["std"], c["jp"], **a)[1].cuda()

    scale = 0.01
    for kind in ("ddim", "dpmpp", "ddpm"):
        coef = d._device_coef(kind, 0.0, 2, "cuda")
        for t in (N - 1, N // 2, 0):
            c0 = float(coef[t, 1])
            xo, x0o = x.clone(), x0.clone()
            L.check(_guide(xo, x0o, None, k, scale, 1, coef, N, t))
            # one fp32 step each way, a few ulp of the largest value involved (as §24's test: the gradients are large)
            want = x0 - scale * grad_of(x0)
            assert float((x0o - want).abs().max()) <= 1e-6 * float(torch.maximum(x0.abs(), want.abs()).max()), (kind, t)
            delta = x0o - x0
            big = max(1.0, float(x.abs().max()), abs(c0) * float(delta.abs().max()))
            assert float((xo - x - c0 * delta).abs().max()) <= 1e-6 * big, (kind, t)
            assert torch.equal(x0o[:, :, D:], x0[:, :, D:]) and torch.equal(xo[:, :, D:], x[:, :, D:])
            for b in range(3):  # frames past the length are not touched
                n = int(lens[b])
                assert torch.equal(x0o[b, n:], x0[b, n:]) and torch.equal(xo[b, n:], x[b, n:])
            assert not torch.equal(x0o, x0)
    # k iterations = k chained loss-grad steps, at the step size §24's test derives for these weights (1e-5)
    coef = d._device_coef("ddim", 0.0, 2, "cuda")
    scale = 1e-5
    for it in (2, 5):
        xo, x0o = x.clone(), x0.clone()
        L.check(_guide(xo, x0o, None, k, scale, it, coef, N, 3))
        y = x0.clone()
        for _ in range(it):
            y = y - scale * grad_of(y)
        e = float((x0o - y).abs().max()) / float(x0.abs().max())
        print(f"[terrain guidance] {it} iterations vs chained loss-grad steps: {e:.2e}")
        assert e <= 1e-6, (it, e)
    # a terrain alone (no scene, no tracks, no targets, no S) moves x0 as well; so does the NULL-terrain call, bit for bit the
    # tracks call
    alone = dict(scene=None, tracks=None, bounds=None, tg=None, w=None, S=None)
    xo, x0o = x.clone(), x0.clone()
    L.check(_guide(xo, x0o, None, k, 0.01, 1, coef, N, 3, **alone))
    want = x0 - 0.01 * grad_of(x0, scene=None, tracks=None, tg=None, w=None, S=None)
    assert float((x0o - want).abs().max()) <= 1e-6 * float(torch.maximum(x0.abs(), want.abs()).max())
    assert not torch.equal(x0o, x0)
    gen = torch.Generator().manual_seed(5)
    mask = (torch.rand(x0.shape, generator=gen) < 0.5).float().cuda()
    for m in (None, mask):
        xo, x0o = x.clone(), x0.clone()
        L.check(_guide(xo, x0o, m, k, 1e-5, 3, coef, N, 4, grid=None))
        x1, x01 = x.clone(), x0.clone()
        L.check(L.lib().mdm_joint_tracks_guidance(
            _vp(x1), _vp(x01), _vp(m), _vp(lens), _vp(k["mean"]), _vp(k["std"]), _vp(k["tg"]), _vp(k["w"]), _vp(k["scene"]),
            C.c_int32(5), _vp(k["jp"]), _vp(k["tracks"]), C.c_int32(5), _vp(k["bounds"]), C.c_int32(3), C.c_int32(40),
            C.c_int32(263), C.c_float(1e-5), C.c_int32(3), _vp(coef), C.c_int32(N), C.c_void_p(0), C.c_int32(4),
            C.c_void_p(L.stream_ptr())))
        assert torch.equal(_bits(x1), _bits(xo)) and torch.equal(_bits(x01), _bits(x0o)) and not torch.equal(x0o, x0)


@pytest.mark.parametrize("grid", ["2x2", "3x5", "512"])
def test_untouched_terrain_and_masked_entries_are_bitwise_unchanged(grid):
    L = pkg("_lib")
    d = _diffusion("ddim10")
    N = d.num_timesteps
    coef = d._device_coef("dpmpp", 0.0, 2, "cuda")
    c, k, x, x0 = _kernel_case("stand", grid)
    x, x0 = x.clone(), x0.clone()
    x0[0, :5, :10] = -0.0
    x[0, :5, :10] = -0.0
    alone = dict(scene=None, tracks=None, bounds=None, tg=None, w=None)
    off, deep = k["rec"].clone(), k["grid"] - 1000.0  # weight 0 (with S); a ground 1 km below every joint with S = 0
    off[:, 6] = 0.0
    for over in (dict(rec=off), dict(grid=deep, S=None), dict(grid=deep, S=torch.zeros_like(k["S"]))):
        for m in (None, (torch.rand(x0.shape, generator=torch.Generator().manual_seed(6)) < 0.5).float().cuda()):
            xo, x0o = x.clone(), x0.clone()
            L.check(_guide(xo, x0o, m, k, 0.05, 3, coef, N, 4, **alone, **over))
            assert torch.equal(_bits(xo), _bits(x)) and torch.equal(_bits(x0o), _bits(x0)), list(over)
    gen = torch.Generator().manual_seed(8)
    mask = (torch.rand(x0.shape, generator=gen) < 0.5).float().cuda()
    xo, x0o = x.clone(), x0.clone()
    L.check(_guide(xo, x0o, mask, k, 1e-3, 3, coef, N, 4, **alone))
    keep = mask == 1
    assert torch.equal(_bits(x0o[keep]), _bits(x0[keep])) and torch.equal(_bits(xo[keep]), _bits(x[keep]))
    assert not torch.equal(x0o[~keep], x0[~keep])


def test_argument_errors():
    L = pkg("_lib")
    d = _diffusion("ddim10")
    N = d.num_timesteps
    coef = d._device_coef("ddim", 0.0, 2, "cuda")
    c, k, x, x0 = _kernel_case()
    a = (x.clone(), x0.clone(), None, k, 0.001, 1, coef, N, 0)
    assert _guide(*a) == 0
    for dims in ((1, 3), (5, 1), (513, 3), (5, 513), (0, 0), (-2, 3)):
        assert _guide(*a, dims=dims) == 1, dims
    assert _guide(*a, rec=None) == 1  # a grid without its record
    buf = torch.zeros(4 + k["rec"].numel(), device="cuda")  # the records 16 and 4 bytes into an aligned buffer
    buf[4:], odd = k["rec"].flatten(), buf[1:]
    assert _guide(*a, rec=buf[4:]) == 0 and _guide(*a, rec=odd) == 1
    for name in ("lens", "mean", "std", "jp", "tg", "w"):  # what the tracks calls refuse; targets without weights
        assert _guide(*a, **{name: None}) == 1, name
    assert _guide(*a, tracks=k["tracks"].flatten()[1:]) == 1
    for i, v in ((4, float("nan")), (5, 0), (5, L.CONTROL_MAX_ITERS + 1), (7, 0), (8, N), (8, -1)):
        bad = list(a)
        bad[i] = v
        assert _guide(*bad) == 1, (i, v)
    for shape in ((3, 40, 262), (3, 0, 263), (-1, 40, 263), (3, 205, 263)):
        assert _guide(*a, shape=shape) == 1, shape
    assert _guide(*a, grid=None, rec=None, dims=(0, 0)) == 0  # no terrain: the tracks call, the rest not looked at
    torch.cuda.synchronize()


# ---- mdm_terrain_stand_weights ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [263, 251])
def test_stand_weights_match_the_torch_restatement(F):
    L = pkg("_lib")
    sk = next(s for s in pkg("motion_features").SKELETONS.values() if s.feats == F)
    J, n, rows_total = (F + 1) // 12, 300, 520
    gen = torch.Generator().manual_seed(F)
    x0 = torch.randn(rows_total, F, generator=gen)
    mean, std = torch.randn(F, generator=gen) * 0.2, torch.rand(F, generator=gen) + 0.5
    thr = 0.5
    lab = x0[:, F - 4:] * std[F - 4:] + mean[F - 4:]
    near = (lab - thr).abs() < 0.05  # keep the labels clear of the threshold: the comparison is then exact
    x0[:, F - 4:] = torch.where(near, (thr + 0.2 - mean[F - 4:]) / std[F - 4:], x0[:, F - 4:])
    lab = x0[:, F - 4:] * std[F - 4:] + mean[F - 4:]
    assert float((lab - thr).abs().min()) >= 0.05 and 0.2 < float((lab > thr).float().mean()) < 0.8
    rows = torch.randperm(rows_total, generator=gen)[:n].to(torch.int32)
    feet = (C.c_int32 * 4)(*sk.feet)
    x0_d, mean_d, std_d, rows_d = x0.cuda(), mean.cuda(), std.cuda(), rows.cuda()
    for fr in (None, rows):
        count = n if fr is not None else rows_total
        out = torch.full((count, J), -1.0, device="cuda")
        L.check(L.lib().mdm_terrain_stand_weights(_vp(x0_d), _vp(None if fr is None else rows_d), C.c_int32(count), _vp(mean_d),
                                                  _vp(std_d), C.c_int32(F), C.c_int32(0), feet, C.c_float(thr), _vp(out),
                                                  C.c_void_p(L.stream_ptr())))
        want = torch.zeros(count, J)
        src = lab if fr is None else lab[fr.long()]
        for kf, j in enumerate(sk.feet):
            want[:, j] = (src[:, kf] > thr).float()
        assert torch.equal(out.cpu(), want) and 0 < float(want.sum())
    # a row of mean / std per group of frames (a batch of windows with per-sample statistics), in one launch
    Bq, Tq = 13, 40
    means, stds = torch.randn(Bq, F, generator=gen) * 0.2, torch.rand(Bq, F, generator=gen) + 0.5
    xq = x0[:Bq * Tq].reshape(Bq, Tq, F).clone()
    labq = xq[..., F - 4:] * stds[:, None, F - 4:] + means[:, None, F - 4:]
    xq[..., F - 4:] = torch.where((labq - thr).abs() < 0.05, (thr + 0.2 - means[:, None, F - 4:]) / stds[:, None, F - 4:], xq[..., F - 4:])
    labq = xq[..., F - 4:] * stds[:, None, F - 4:] + means[:, None, F - 4:]
    assert float((labq - thr).abs().min()) >= 0.05
    xq_d, means_d, stds_d = xq.cuda(), means.cuda(), stds.cuda()
    out = torch.full((Bq, Tq, J), -1.0, device="cuda")
    L.check(L.lib().mdm_terrain_stand_weights(_vp(xq_d), None, C.c_int32(Bq * Tq), _vp(means_d), _vp(stds_d), C.c_int32(F),
                                              C.c_int32(Tq), feet, C.c_float(thr), _vp(out), C.c_void_p(L.stream_ptr())))
    want = torch.zeros(Bq, Tq, J)
    for kf, j in enumerate(sk.feet):
        want[..., j] = (labq[..., kf] > thr).float()
    assert torch.equal(out.cpu(), want) and not torch.equal(want[0], want[1])


# ---- the canvas kernel --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _canvas_case(canvases, F):
    """test_motion_scene_gpu._canvas_case's draws (rows shuffled over windows of 200 frames, a scene, fractional targets, radii)
    with a 3 x 5 terrain turned by 0.4 and fractional S per motion, and the reference's loss and gradient."""
    from test_motion_scene_gpu import _canvas_case as scene_canvas
    c = dict(scene_canvas(canvases, F, True))
    J = (F + 1) // 12
    total = int(c["off"][-1])
    gen = torch.Generator().manual_seed(total + F)
    S = torch.rand(total, J, generator=gen) * 1.5
    S[S < 0.45] = 0.0
    flat = c["x"].reshape(-1, F)
    grids, recs, lines, shifts, loss, grad = [], [], [], [], [], torch.zeros(total, F, dtype=torch.float64)
    for m in range(len(canvases)):
        a, b = int(c["off"][m]), int(c["off"][m + 1])
        rows = flat[c["fr"][a:b]]
        P = ref_positions(rows, c["mean"][m], c["std"][m]).detach()
        g, r, sh = G.place_terrain(P, c["jp"][m], S[a:b], 5, 3, None, 0.4, seed=11 + m)
        grids.append(g.float()), recs.append(r.float()), shifts.append(sh)
        lines.append(G.line_distance(P, grids[-1], recs[-1], c["jp"][m], S[a:b]))
        l, gr = G.ref_terrain_loss_grad(rows[None], [b - a], c["mean"][m], c["std"][m], grids[-1][None], recs[-1][None],
                                        c["jp"][m][None], S[a:b][None], c["scene"][m][None], None, c["tg"][a:b][None], c["w"][a:b][None])
        loss.append(l[0])
        grad[a:b] = gr[0]
    c.update(S=S, grid=torch.stack(grids), rec=torch.stack(recs), lines=lines, shifts=shifts, ref=(torch.stack(loss), grad))
    return c


CANVAS_KEYS = ("mean", "std", "tg", "w", "scene", "jp", "tracks", "bounds", "grid", "rec", "S")


def _canvas_dev(c, **over):
    """The canvas case's arguments on the device (tracks (total, Km, 12) and their balls where the case has them)."""
    a = {k: c.get(k) for k in CANVAS_KEYS}
    a.update(over)
    k = {n: _cu(v) for n, v in a.items()}
    k.update(off=c["off"].cuda().to(torch.int32), fr=c["fr"].cuda().to(torch.int32))
    return k


def _canvas_lg(c, x=None, **over):
    """mdm_canvas_terrain_loss_grad on packed arguments; ``x``: other rows than the case's (B, Tw, F)."""
    L = pkg("_lib")
    F = c["x"].shape[-1]
    M, total = c["off"].numel() - 1, c["fr"].numel()
    k = _canvas_dev(c, **over)
    xd = _cu(c["x"] if x is None else x)
    loss, grad = torch.zeros(M, device="cuda"), torch.zeros(total, F, device="cuda")
    ws = torch.empty(int(L.lib().mdm_canvas_control_workspace_floats(total, F)), device="cuda")
    K, Km = (0 if k["scene"] is None else k["scene"].shape[1]), (0 if k["tracks"] is None else k["tracks"].shape[1])
    L.check(L.lib().mdm_canvas_terrain_loss_grad(
        _vp(xd), _vp(k["off"]), _vp(k["fr"]), _vp(k["mean"]), _vp(k["std"]), _vp(k["tg"]), _vp(k["w"]), _vp(k["scene"]), C.c_int32(K),
        _vp(k["jp"]), _vp(k["tracks"]), C.c_int32(Km), _vp(k["bounds"]), _vp(k["grid"]), _vp(k["rec"]), C.c_int32(k["grid"].shape[2]),
        C.c_int32(k["grid"].shape[1]), _vp(k["S"]), C.c_int32(M), C.c_int32(F), _vp(loss), _vp(grad), _vp(ws),
        C.c_void_p(L.stream_ptr())))
    return loss.cpu(), grad.cpu()


def _canvas_guide(c, x, x0, mask, scale, iters, coef, steps, t, **over):
    """mdm_canvas_terrain_guidance in place on the rows x / x0 (B, Tw, F) on the device."""
    L = pkg("_lib")
    F = c["x"].shape[-1]
    M, total = c["off"].numel() - 1, c["fr"].numel()
    k = _canvas_dev(c, **over)
    ws = torch.empty(int(L.lib().mdm_canvas_control_workspace_floats(total, F)), device="cuda")
    K, Km = (0 if k["scene"] is None else k["scene"].shape[1]), (0 if k["tracks"] is None else k["tracks"].shape[1])
    L.check(L.lib().mdm_canvas_terrain_guidance(
        _vp(x), _vp(x0), _vp(mask), _vp(k["off"]), _vp(k["fr"]), _vp(k["mean"]), _vp(k["std"]), _vp(k["tg"]), _vp(k["w"]),
        _vp(k["scene"]), C.c_int32(K), _vp(k["jp"]), _vp(k["tracks"]), C.c_int32(Km), _vp(k["bounds"]), _vp(k["grid"]), _vp(k["rec"]),
        C.c_int32(k["grid"].shape[2]), C.c_int32(k["grid"].shape[1]), _vp(k["S"]), C.c_int32(M), C.c_int32(F), C.c_float(scale),
        C.c_int32(iters), _vp(coef), C.c_int32(steps), C.c_void_p(0), C.c_int32(t), _vp(ws), C.c_void_p(L.stream_ptr())))
    torch.cuda.synchronize()


def _short_canvas():
    """The (3, 40) "all" case's first sample (40 frames) as a one-motion canvas, its rows in order, with its five tracks."""
    c = _case(3, 40, 263, "3x5", "all")
    return c, dict(x=c["x0"][:1], off=torch.tensor([0, 40]), fr=torch.arange(40), mean=c["mean"][:1], std=c["std"][:1], tg=c["tg"][0],
                   w=c["w"][0], jp=c["jp"][:1], scene=c["scene"][:1], grid=c["grid"][:1], rec=c["rec"][:1], S=c["S"][0],
                   tracks=c["tracks"][0], bounds=pkg("motion_scene").track_bounds(c["tracks"][0]))


@pytest.mark.parametrize("mask_on", [False, True])
def test_canvas_guidance_kernel_steps_and_update(mask_on):
    """mdm_canvas_terrain_guidance (with and without an edit mask: its two instantiations) on the two shuffled motions with a
    scene, targets and S, and on the 40-frame canvas with tracks: one iteration is x0 - scale (1 - m) grad over the canvas
    rows with x moved by c0 delta, every other row keeps its bits, k iterations are k chained steps, and a terrain of weight
    0, a ground no joint touches and NULL stand leave what they must."""
    d = _diffusion("ddim10")
    N = d.num_timesteps
    short_c, short = _short_canvas()
    for c, scale, tag in ((_canvas_case((300, 700), 263), 1e-7, "300 + 700"), (short, 1e-5, "40, tracks")):
        F, fr = c["x"].shape[-1], c["fr"].long()
        gen = torch.Generator().manual_seed(9)
        x0, x = _cu(c["x"]), torch.randn(c["x"].shape, generator=gen).cuda()
        mask = (torch.rand(c["x"].shape, generator=gen) < 0.5).float().cuda() if mask_on else None
        keep = 1.0 if mask is None else 1.0 - mask.reshape(-1, F)[fr.cuda()]

        def step(y, **over):  # one restated step: the loss-grad's gradient on the canvas rows
            g = _canvas_lg(c, x=y, **over)[1].cuda()
            flat = y.clone().reshape(-1, F)
            flat[fr.cuda()] = flat[fr.cuda()] - scale * keep * g
            return flat.view_as(y)

        for kind, t in (("ddim", N - 1), ("dpmpp", N // 2), ("ddpm", 0)):
            coef = d._device_coef(kind, 0.0, 2, "cuda")
            c0 = float(coef[t, 1])
            xo, x0o = x.clone(), x0.clone()
            _canvas_guide(c, xo, x0o, mask, scale, 1, coef, N, t)
            want = step(x0)
            assert float((x0o - want).abs().max()) <= 1e-6 * float(torch.maximum(x0.abs(), want.abs()).max()), (tag, kind)
            delta = x0o - x0
            big = max(1.0, float(x.abs().max()), abs(c0) * float(delta.abs().max()))
            assert float((xo - x - c0 * delta).abs().max()) <= 1e-6 * big, (tag, kind)
            assert torch.equal(x0o[..., 67:], x0[..., 67:]) and torch.equal(xo[..., 67:], x[..., 67:])
            other = torch.ones(x0.numel() // F, dtype=torch.bool)
            other[fr] = False  # rows that are no canvas frame
            assert torch.equal(_bits(x0o.reshape(-1, F)[other.cuda()]), _bits(x0.reshape(-1, F)[other.cuda()]))
            assert torch.equal(_bits(xo.reshape(-1, F)[other.cuda()]), _bits(x.reshape(-1, F)[other.cuda()]))
            assert not torch.equal(x0o, x0)
            if mask is not None:
                assert torch.equal(_bits(x0o[mask == 1]), _bits(x0[mask == 1])) and torch.equal(_bits(xo[mask == 1]), _bits(x[mask == 1]))
        coef = d._device_coef("ddim", 0.0, 2, "cuda")
        for it in (2, 5):
            xo, x0o = x.clone(), x0.clone()
            _canvas_guide(c, xo, x0o, mask, scale, it, coef, N, 3)
            y = x0.clone()
            for _ in range(it):
                y = step(y)
            e = float((x0o - y).abs().max()) / float(x0.abs().max())
            print(f"[canvas terrain guidance {tag} mask {mask_on}] {it} iterations vs chained loss-grad steps: {e:.2e}")
            assert e <= 1e-6, (tag, it, e)
        # NULL stand and NULL balls: the step of the loss-grad called the same way
        xo, x0o = x.clone(), x0.clone()
        _canvas_guide(c, xo, x0o, mask, scale, 1, coef, N, 3, S=None, bounds=None)
        want = step(x0, S=None, bounds=None)
        assert float((x0o - want).abs().max()) <= 1e-6 * float(torch.maximum(x0.abs(), want.abs()).max()), tag
        # the terrain alone with weight 0 (with S), and a ground 1 km below with S NULL or 0: no bit moves, -0.0 included
        x0z, xz = x0.clone(), x.clone()
        x0z.reshape(-1, F)[fr[:5].cuda(), :10] = -0.0
        xz.reshape(-1, F)[fr[:5].cuda(), :10] = -0.0
        alone = dict(scene=None, tracks=None, bounds=None, tg=None, w=None)
        off = c["rec"].clone()
        off[:, 6] = 0.0
        for over in (dict(rec=off), dict(grid=c["grid"] - 1000.0, S=None), dict(grid=c["grid"] - 1000.0, S=torch.zeros_like(c["S"]))):
            xo, x0o = xz.clone(), x0z.clone()
            _canvas_guide(c, xo, x0o, mask, 0.05, 3, coef, N, 4, **alone, **over)
            assert torch.equal(_bits(xo), _bits(xz)) and torch.equal(_bits(x0o), _bits(x0z)), (tag, list(over))


def test_canvas_terrain_loss_grad_matches_fp64_autograd():
    canvases, F = (300, 700), 263
    c = _canvas_case(canvases, F)
    print(f"[canvas terrain] origin shifts {c['shifts']}, (least distance to a line along x, z; share kept above, pulled down) "
          f"{c['lines']}")
    assert max(c["shifts"]) <= G.SHIFTS
    assert all(min(ln[0], ln[1]) >= G.LINE_CLEAR and ln[2] >= 0.05 and ln[3] >= 0.05 for ln in c["lines"])
    loss, grad = _canvas_lg(c)
    rl, rg = c["ref"]
    assert torch.equal(grad[:, 67:], torch.zeros(sum(canvases), F - 67))
    for m, n in enumerate(canvases):
        a = int(c["off"][m])
        el = abs(float(loss[m]) - float(rl[m])) / float(rl[m])
        eg = rel_inf(grad[a:a + n], rg[a:a + n])
        print(f"[canvas terrain n={n}] loss rel {el:.2e} gradient rel_inf {eg:.2e}")
        assert el <= 1e-5, (m, el)
        assert eg <= 1e-4, (m, eg)


def test_canvas_kernel_equals_the_window_kernel_on_a_short_motion():
    """The (3, 40) case's first sample (40 frames) as a one-motion canvas, its rows in order: the two kernels' summation
    orders differ, so they agree to the gates, not bit for bit; and the Python entry with stand weights."""
    c, one = _short_canvas()
    for S, tag in ((c["S"], "tracks, S"), (None, "tracks, NULL stand")):  # with the five tracks and their balls
        loss, grad = _canvas_lg(one, S=None if S is None else S[0])
        wl, wg = _terrain_lg(c["x0"][:1], c["lens"][:1], c["mean"][:1], c["std"][:1], c["jp"][:1], c["grid"][:1], c["rec"][:1],
                             None if S is None else S[:1], c["scene"][:1], c["tracks"][:1], one["bounds"][None], c["tg"][:1], c["w"][:1])
        el, eg = abs(float(loss[0]) - float(wl[0])) / float(wl[0]), rel_inf(grad, wg[0])
        print(f"[canvas vs window, terrain, {tag}] loss rel {el:.2e} gradient rel_inf {eg:.2e}")
        assert el <= 1e-5 and eg <= 1e-4
        rl, rg = G.ref_terrain_loss_grad(c["x0"][:1], c["lens"][:1], c["mean"][:1], c["std"][:1], c["grid"][:1], c["rec"][:1], c["jp"][:1],
                                         None if S is None else S[:1], c["scene"][:1], c["tracks"][:1], c["tg"][:1], c["w"][:1])
        assert abs(float(loss[0]) - float(rl[0])) <= 1e-5 * float(rl[0]) and rel_inf(grad, rg[0]) <= 1e-4
    nb = _canvas_lg(one, bounds=None)  # the broad phase's balls change no bit
    wb = _canvas_lg(one)
    assert torch.equal(_bits(nb[0]), _bits(wb[0])) and torch.equal(_bits(nb[1]), _bits(wb[1]))
    MS = pkg("motion_scene")
    med = c["P"][0].reshape(-1, 3).median(0).values
    one_t = MS.stairs((float(med[0]) - 0.5, float(med[2])), 0.3, 4, 0.15, 0.3, 2.0, margin=0.02)
    one_t.heights += float(med[1]) - 0.3
    l1, g1 = MS.canvas_scene_loss_grad(c["x0"][:1].cuda(), [0, 40], torch.arange(40), c["mean"][0], c["std"][0], None, terrain=[one_t],
                                       stand=c["S"][0])
    l2, g2 = MS.scene_loss_grad(c["x0"][:1].cuda(), [40], c["mean"][0], c["std"][0], None, terrain=one_t, stand=c["S"][:1])
    assert float(l2[0]) > 0 and abs(float(l1[0]) - float(l2[0])) <= 1e-5 * float(l2[0]) and rel_inf(g1.cpu(), g2[0].cpu()) <= 1e-4


# ---- loops --------------------------------------------------------------------------------------------------------------
def _loop_terrain():
    """A 2 x 2 grid of 200 m cells centred on the origin, turned by 0.3: every joint of a window lies over its one cell, so
    no step of a loop meets a line where the slope jumps (the loop's x0 moves, and a placement cannot be kept clear)."""
    MS = pkg("motion_scene")
    c, s = math.cos(0.3), math.sin(0.3)
    return MS.heightfield([[-1.0, 1.5], [0.5, 4.0]], 200.0, (-100.0 * (c + s), -100.0 * (c - s)), 0.3, margin=0.05, weight=1.5)


def _control(B, T, scale=0.001, iters=2, stand="contacts"):
    """A root path, §24's loop scene and a terrain over the loops_tiny batch, as control_* kwargs (CPU tensors)."""
    from test_motion_scene_gpu import _control as scene_control
    ctl = scene_control(B, T, scale, iters)
    hs, rec = pkg("motion_scene").batch_terrain(_loop_terrain(), B)
    ctl.update(control_terrain=hs, control_terrain_rec=rec, control_stand=stand)
    return ctl


def _contacts(x0, mean, std, feet, thr=0.5):
    """The torch restatement of mdm_terrain_stand_weights on x0 (B, T, F) with mean / std (B, F), in fp32 as the kernel."""
    B, T, F = x0.shape
    lab = x0.float()[..., F - 4:] * std.float()[:, None, F - 4:] + mean.float()[:, None, F - 4:]
    S = torch.zeros(B, T, (F + 1) // 12)
    for k, j in enumerate(feet):
        S[..., j] = (lab[..., k] > thr).float()
    return S, float((lab - thr).abs().min())


def _restated(d, mode, m, g, ctl, inputs, scale, eta=0.0, step_noise=None, known=None, mask=None):
    """As test_motion_scene_gpu._restated, with L_terrain in the guidance: the stand weights are the contacts of the x0 the
    guidance of a step starts from, fixed over its iterations."""
    import sampler_ref as SR
    one_minus_m = 1.0 if mask is None else 1.0 - mask.double()
    feet = pkg("motion_features").SKELETONS["t2m"].feet
    near = []

    def guide(x0):
        stand, gap = _contacts(x0, ctl["control_mean"], ctl["control_std"], feet)
        near.append(gap)
        for _ in range(ctl["control_iters"]):
            _, gr = G.ref_terrain_loss_grad(x0, g["length"], ctl["control_mean"], ctl["control_std"], ctl["control_terrain"],
                                            ctl["control_terrain_rec"], ctl["control_joint_params"], stand, ctl["control_scene"],
                                            None, ctl["control_joints"], ctl["control_weights"])
            x0 = x0 - ctl["control_scale"] * one_minus_m * gr
        return x0

    out = SR.loop_ref(d, mode, scale, SR.device_eps(m, g["length"]), prompts=[(g["xf_proj"], g["xf_out"])],
                      uncond=m.uncond_embedding(g["x_T"].shape[0], "cuda"), inputs=inputs, eta=eta, step_noise=step_noise,
                      clip=True, known=known, mask=mask, x0_hook=guide)
    return out, min(near)


@pytest.mark.parametrize("mode,eta,edit", [("cfg_dpmpp", 0.0, False), ("ddim", 0.5, False), ("cfg_dpmpp", 0.0, True)])
def test_terrain_loops_match_the_restated_loop(mode, eta, edit):
    import sampler_ref as SR
    from test_motion_scene_gpu import _check_against_restated, _cuda, _setup
    g, meta, m, noises, kw = _setup()
    d = _diffusion("ddim10")
    N, sc = d.num_timesteps, meta["cfg_scale"]
    B, T, F_ = g["x_T"].shape
    ctl = _control(B, T)
    ns = noises(f"terrain.{mode}.{eta}", N)
    known = mask = None
    skw = dict(kw, **_cuda(ctl))
    if edit:
        known = pkg("synth").uniform_pm1((B, T, F_), "terrain.known", meta["iseed"])
        mask = torch.broadcast_to(pkg("motion_edit").inbetween_mask(T, 3, 4), (B, T, F_))
        skw.update(inpaint_motion=known.cuda(), inpaint_mask=mask.cuda())
    outs = []
    for use_graph in (True, False):
        got = []
        out = SR.run_loop(d, mode, m, skw, sc, eta, use_graph, x_T=g["x_T"].cuda(), step_noise=ns, clip=True,
                          cb=lambda i, t, x: got.append(x.clone().cpu())).cpu()
        assert len(got) == N and torch.equal(out, got[-1]) and torch.isfinite(out).all()
        outs.append(out)
        if use_graph:
            want, gap = _restated(d, mode, m, g, ctl, [g["x_T"]] + got[:-1], sc, eta, ns, known, mask)
            print(f"[terrain loop {mode}] the contact label nearest the threshold is {gap:.2e} away")
            assert gap > 1e-5  # no label the two sides could see on different sides of the threshold
            _check_against_restated(got, want, f"terrain {mode} eta {eta} edit {edit}")
    assert torch.equal(outs[0], outs[1])  # graph == eager
    if edit:
        assert torch.equal(outs[0][mask == 1], known[mask == 1])
    run = lambda k: SR.run_loop(d, mode, m, k, sc, eta, True, x_T=g["x_T"].cuda(), step_noise=ns, clip=True).cpu()  # noqa: E731
    no_terrain = {k: v for k, v in skw.items() if k not in ("control_terrain", "control_terrain_rec", "control_stand")}
    assert not torch.equal(run(no_terrain), outs[0])
    assert not torch.equal(run(dict(skw, control_stand=None)), outs[0])  # the stand term acts
    # given stand weights in the place of the contacts; the terrain alone, without scene and targets
    given = torch.rand(B, T, 22, generator=torch.Generator().manual_seed(1)).cuda()
    out = run(dict(skw, control_stand=given))
    assert torch.isfinite(out).all() and not torch.equal(out, outs[0])
    alone = {k: v for k, v in skw.items() if k not in ("control_joints", "control_weights", "control_scene", "control_joint_params")}
    out = run(alone)
    assert torch.isfinite(out).all() and not torch.equal(out, outs[0])


def test_trainer_terrain_is_independent_of_the_batch_split():
    """generate(terrain=, terrain_stand=) over batch splits, bucketing and the joints front end.  The trainer samples unclipped,
    so the grounds are planes (2 x 2 grids far larger than a motion): heights are linear in x0 and a fixed step is stable."""
    from test_motion_scene_gpu import _setup, _trainer
    from test_motion_control_gpu import _stats
    MS = pkg("motion_scene")
    g, meta, m, noises, kw = _setup()
    tr = _trainer(m, meta)
    caps = ["a", "b", "c", "d"]
    mean, std = (v[0].numpy() for v in _stats(263, 1, 21))
    grounds = [MS.ramp((-500.0, 0.0), 0.0, 1000.0, 100.0, 1000.0), MS.ramp((-500.0, 0.0), 0.4, 1000.0, -50.0, 1000.0, margin=0.1),
               MS.heightfield([[0.5, 0.5], [0.5, 0.5]], 1000.0, (-500.0, -500.0)), _loop_terrain()]
    opts = dict(seed=3, sampler="ddim", sample_steps=10, eta=0.5, terrain=grounds, terrain_stand="contacts",
                scene_joint_radius=[0.05] * 22, control_scale=0.01, control_iters=2, mean=mean, std=std)
    same = torch.tensor([16, 16, 16, 16])
    one = torch.stack(tr.generate(caps, same, 263, batch_size=1, **opts)).cpu()
    two = torch.stack(tr.generate(caps, same, 263, batch_size=2, **opts)).cpu()
    assert torch.isfinite(one).all() and rel_inf(one, two) < 1e-5, rel_inf(one, two)
    plain = torch.stack(tr.generate(caps, same, 263, batch_size=2, seed=3, sampler="ddim", sample_steps=10, eta=0.5)).cpu()
    assert all(not torch.equal(plain[i], two[i]) for i in range(4))
    shared = torch.stack(tr.generate(caps, same, 263, batch_size=2, **dict(opts, terrain=grounds[0]))).cpu()
    assert rel_inf(shared[0], two[0]) < 1e-5 and not torch.equal(shared[1], two[1])
    none = torch.stack(tr.generate(caps, same, 263, batch_size=2, **dict(opts, terrain_stand=None))).cpu()
    assert not torch.equal(none, two)
    lens = torch.tensor([8, 16, 12, 4])
    stand = torch.rand(4, 16, 22, generator=torch.Generator().manual_seed(2))
    o2 = dict(opts, terrain_stand=stand)
    serial = tr.generate(caps, lens, 263, batch_size=2, **o2)
    bucket = tr.generate_bucketed(caps, lens, 263, batch_size=2, unit_length=4, **o2)
    for i, n in enumerate(lens.tolist()):
        assert rel_inf(bucket[i][:n].cpu(), serial[i][:n].cpu()) < 1e-4, i
    ex = {k: v for k, v in opts.items() if k not in ("mean", "std")}
    joints = tr.generate_joints(caps, lens, 263, mean, std, batch_size=2, sigma=0.0, **ex)
    assert [tuple(j.shape) for j in joints] == [(n, 22, 3) for n in lens.tolist()]
    depth, share = MS.penetration(torch.stack([torch.nn.functional.pad(j, (0, 0, 0, 0, 0, 16 - j.shape[0])) for j in joints]),
                                  lens, None, [0.05] * 22, terrain=grounds)
    assert depth.shape == (4,) and share.shape == (4,) and bool(torch.isfinite(depth).all())
    with pytest.raises(ValueError):
        tr.generate(caps, same, 263, batch_size=2, seed=3, terrain=grounds)  # no mean / std


# ---- behaviour ----------------------------------------------------------------------------------------------------------
RAMP_RATIO_MEASURED = 4.7e-3  # on an MI355X: 4.68e-3 and 7.3e-4 for the two samples of loops_tiny
RAMP_RATIO_GATE = 0.5 if RAMP_RATIO_MEASURED is None else min(4 * RAMP_RATIO_MEASURED, 0.5)


def test_a_ramp_is_climbed():
    """§24's avoidance setting (loops_tiny, guided DDIM-20, x0 clipped, the pelvis path of test_an_obstacle_on_the_path_is_avoided,
    mean 0, std 1 except the heading velocity's 0.05, control_scale 0.002, control_iters 8) on a ramp that rises 0.5 m over the
    path's first 2 m, with control_stand="contacts": L_terrain of the final sample (its own contact labels as stand weights)
    with the terrain against the run without it (the path alone).  The weight follows §14's rule scale x curvature < 2: a
    height is linear in x0, so the curvature is 2 a u std^2 per term and a = 100 gives 0.002 x 200 = 0.4."""
    from test_motion_scene_gpu import _cuda, _setup
    M, MS = pkg("motion_control"), pkg("motion_scene")
    g, meta, m, noises, kw = _setup()
    d = _diffusion("ddim20")
    B, T, F_ = g["x_T"].shape
    tg, w = M.root_path_targets(T, [[0.0, 0.0], [2.0, 0.0], [2.0, 2.0]], [0, T // 2, T - 1])
    mean, std = torch.zeros(B, F_), torch.ones(B, F_)
    std[:, 0] = 0.05
    ground = MS.ramp((0.0, 0.0), 0.0, 2.0, 0.5, 20.0, weight=100.0)
    hs, rec = MS.batch_terrain(ground, B)
    ctl = {"control_joints": tg.expand(B, -1, -1, -1).clone(), "control_weights": w.expand(B, -1, -1, -1).clone(),
           "control_mean": mean, "control_std": std, "control_scale": 0.002, "control_iters": 8}
    tr = {"control_terrain": hs, "control_terrain_rec": rec, "control_stand": "contacts"}
    outs = {}
    for name, k in (("path", dict(kw, **_cuda(ctl))), ("terrain", dict(kw, **_cuda(ctl), **_cuda(tr)))):
        outs[name] = d.ddim_sample_loop_with_cfg(m, (B, T, F_), clip_denoised=True, model_kwargs=k, cfg_scale=2.5, seed=7)
    feet = pkg("motion_features").SKELETONS["t2m"].feet
    lt = {k: MS.scene_loss_grad(v, g["length"], mean, std, None, terrain=ground, stand=_contacts(v.cpu(), mean, std, feet)[0])[0].cpu()
          for k, v in outs.items()}
    lp = {k: M.joint_loss_grad(v, g["length"], mean, std, ctl["control_joints"], ctl["control_weights"])[0].cpu()
          for k, v in outs.items()}
    ratio = lt["terrain"] / lt["path"]
    print(f"[ramp] L_terrain without terrain= {lt['path'].tolist()} with {lt['terrain'].tolist()} ratio {ratio.tolist()}; "
          f"path loss without {lp['path'].tolist()} with {lp['terrain'].tolist()}")
    assert bool((lt["path"] > 0).all())
    assert bool((ratio <= RAMP_RATIO_GATE).all()), ratio


# ---- a long motion ------------------------------------------------------------------------------------------------------
def test_long_motion_with_a_terrain_matches_the_restated_canvas_loop():
    """Two windows of 48 and 40 frames at overlap 20 (§24's long setting) with a terrain in the canvas frame,
    terrain_stand="contacts", §24's loop scene and a root path: canvas_control's tables through the samplers against the loop
    restated with the autograd guidance over the canvas, teacher-forced; once with an edit mask; graph == eager."""
    import sampler_ref as SR
    from test_long_control_gpu import _blend_np, _owner, _run
    from test_motion_control_gpu import _stats
    from test_motion_scene_gpu import CANVAS, H, LENS, TW, _cuda, _long_setup, _loop_scene
    M, ML = pkg("motion_control"), pkg("motion_long")
    g, meta, m, text, x_T, plans = _long_setup()
    d = _diffusion("ddim10")
    N, scale = d.num_timesteps, meta["cfg_scale"]
    tg, w = M.root_path_targets(CANVAS, [[0.0, 0.0], [1.0, 0.5], [1.5, 2.0]], [0, CANVAS // 2, CANVAS - 1])
    mean, std = _stats(263, 1, 21)
    std[:, 0] = 0.05
    control = ML.canvas_control(plans, 263, [tg], [w], 2e-4, 2, mean[0], std[0], "cpu", [_loop_scene()], [0.03] * 22,
                                terrain=[_loop_terrain()], terrain_stand="contacts")
    ctl = control([0], TW)
    assert tuple(ctl["canvas_control_terrain"].shape) == (1, 2, 2) and tuple(ctl["canvas_control_terrain_rec"].shape) == (1, 8)
    assert ctl["canvas_control_stand"] == "contacts" and ctl["canvas_control_stand_threshold"] == 0.5
    tab_kw = ML.batch_tables(plans, [0], TW, H, "linear")
    tab = {k[len("handshake_"):]: v.numpy() for k, v in tab_kw.items()}
    kw = {"xf_proj": text["xf_proj"].cuda(), "xf_out": text["xf_out"].cuda(), "length": text["length"].cuda(), **tab_kw}
    fr = ctl["canvas_control_rows"].long()
    feet = pkg("motion_features").SKELETONS["t2m"].feet
    near = []

    def guide_under(mask):
        one_minus_m = 1.0 if mask is None else 1.0 - mask.double().reshape(-1, 263)[fr]

        def guide(x0):
            flat = x0.clone().reshape(-1, 263)
            c = flat[fr]
            stand, gap = _contacts(c[None], mean, std, feet)  # this step's labels, fixed over its iterations
            near.append(gap)
            for _ in range(2):
                _, gr = G.ref_terrain_loss_grad(c[None], [CANVAS], mean[0], std[0], ctl["canvas_control_terrain"],
                                                ctl["canvas_control_terrain_rec"], ctl["canvas_control_joint_params"], stand,
                                                ctl["canvas_control_scene"], None, tg[None], w[None])
                c = c - 2e-4 * one_minus_m * gr[0]
            flat[fr] = c
            return _owner(flat.view_as(x0), tab)

        return guide

    known_c = pkg("synth").uniform_pm1((CANVAS, 263), "longterrain.known", meta["iseed"])
    starts = plans[0][2]
    known = ML.canvas_to_windows(known_c, starts, LENS, TW)
    mask = ML.canvas_to_windows(torch.broadcast_to(pkg("motion_edit").prefix_mask(CANVAS, 34), (CANVAS, 263)), starts, LENS, TW)
    for mode, eta, edit in (("cfg_dpmpp", 0.0, False), ("ddim", 0.5, False), ("cfg_dpmpp", 0.0, True)):
        ns = [pkg("synth").uniform_pm1((2, TW, 263), f"longterrain.{mode}.{i}", meta["iseed"]) * (3.0 ** 0.5) for i in range(N)]
        if edit:
            kw = dict(kw, inpaint_motion=known.cuda(), inpaint_mask=mask.cuda())
        guide = guide_under(mask if edit else None)
        out, got, got0 = _run(d, mode, m, dict(kw, **_cuda(ctl)), scale, eta, True, x_T, ns)
        assert torch.isfinite(out).all()
        if edit:
            canvas = ML.windows_to_canvas(out, starts, LENS)
            assert torch.equal(canvas[:34], known_c[:34]) and not torch.equal(canvas[34:], known_c[34:])
        for v in got + got0:
            assert torch.equal(v[0, LENS[0] - H:LENS[0]], v[1, :H])
        want = SR.loop_ref(d, mode, scale, SR.device_eps(m, text["length"]), prompts=[(text["xf_proj"], text["xf_out"])],
                           uncond=m.uncond_embedding(2, "cuda"), inputs=[_owner(x_T, tab)] + got[:-1], eta=eta, step_noise=ns,
                           clip=True, eps_hook=lambda e: _blend_np(e, tab), noise_hook=lambda z: _owner(z, tab), x0_hook=guide,
                           known=known if edit else None, mask=mask if edit else None)
        worst = max(rel_inf(got[i], want[i]) for i in range(N))
        print(f"[long terrain] {mode} eta {eta} edit {edit}: worst step rel_inf vs restated canvas loop {worst:.2e}; the contact "
              f"label nearest the threshold is {min(near):.2e} away")
        assert min(near) > 1e-5
        assert worst <= 1e-4, worst
        eager, _, _ = _run(d, mode, m, dict(kw, **_cuda(ctl)), scale, eta, False, x_T, ns)
        assert torch.equal(eager, out)
        no_terrain = {k: v for k, v in ctl.items() if "terrain" not in k and "stand" not in k}
        plain, _, _ = _run(d, mode, m, dict(kw, **_cuda(no_terrain)), scale, eta, True, x_T, ns)
        assert not torch.equal(plain, out)
        no_stand = {k: v for k, v in ctl.items() if "stand" not in k}
        other, _, _ = _run(d, mode, m, dict(kw, **_cuda(no_stand)), scale, eta, True, x_T, ns)
        assert not torch.equal(other, out)  # the stand term acts


def test_trainer_generate_long_with_a_terrain():
    """generate_long(terrain=, terrain_stand=) on planes (the trainer samples unclipped): independent of the batch split, with
    contacts and with given stand weights, through the joints front end."""
    import numpy as np
    from test_motion_scene_gpu import _long_setup, _trainer
    MS = pkg("motion_scene")
    g, meta, m, text, x_T, plans = _long_setup()
    tr = _trainer(m, meta)
    scripts = [[("walk", 48), ("sit", 40)], [("jump", 44)], [("run", 44), ("stop", 48)]]
    mean, std = np.zeros(263, np.float32), np.ones(263, np.float32)
    std[0] = 0.05
    grounds = [MS.ramp((-500.0, 0.0), 0.0, 1000.0, 100.0, 1000.0), MS.heightfield([[0.5, 0.5], [0.5, 0.5]], 1000.0, (-500.0, -500.0)),
               _loop_terrain()]
    opts = dict(overlap=20, seed=3, sampler="ddim", sample_steps=10, eta=0.5, terrain=grounds, terrain_stand="contacts",
                scene_joint_radius=[0.05] * 22, control_scale=0.01, control_iters=2)
    outs = {bs: [o.cpu() for o in tr.generate_long(scripts, 263, batch_size=bs, mean=mean, std=std, **opts)] for bs in (2, 5)}
    assert [o.shape[0] for o in outs[2]] == [68, 44, 72]
    for a, b in zip(outs[2], outs[5]):
        assert torch.isfinite(a).all() and rel_inf(a, b) < 1e-5, rel_inf(a, b)
    plain = tr.generate_long(scripts, 263, batch_size=5, overlap=20, seed=3, sampler="ddim", sample_steps=10, eta=0.5)
    assert all(not torch.equal(p.cpu(), o) for p, o in zip(plain, outs[5]))
    gen = torch.Generator().manual_seed(4)
    given = [torch.rand(n, 22, generator=gen) for n in (68, 44, 72)]
    o2 = [o.cpu() for o in tr.generate_long(scripts, 263, batch_size=5, mean=mean, std=std, **dict(opts, terrain_stand=given))]
    assert all(torch.isfinite(a).all() and not torch.equal(a, b) for a, b in zip(o2, outs[5]))
    joints = tr.generate_long_joints(scripts, 263, mean, std, batch_size=5, sigma=0.0, **opts)
    assert [tuple(j.shape) for j in joints] == [(68, 22, 3), (44, 22, 3), (72, 22, 3)]
    with pytest.raises(ValueError):
        tr.generate_long(scripts, 263, mean=mean, std=std, **dict(opts, terrain=grounds[0]))  # one terrain, not one per motion

"""CPU: the body view of the motion preview as far as it goes without a device.

* every ValueError of ``render_mesh`` and of the trainer's ``view=`` / ``mesh=``, and the C entries' argument checks through
  the library (they return before the device is touched);
* on every input of the GPU tests (tests/mesh_render_ref.py ``cases``): the non-decisive pixels are at most 5 % of the pixels
  the body covers, and the all-fp32 restatement agrees with the fp64 one to one grey level on every decisive pixel;
* watertightness: on closed convex meshes every pixel whose centre lies more than 0.5 pixel inside the silhouette is covered;
* each of twelve likely mistakes moves at least 20 decisive pixels of one 48 x 64 image by at least 32 levels, shown from the
  restatement alone.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import pkg

import mesh_render_ref as R


@functools.lru_cache(maxsize=None)
def all_cases():
    return R.cases()


@functools.lru_cache(maxsize=None)
def truth(name):
    """(fp64 image, details) of a case; shared, read-only."""
    return R.run(all_cases()[name], detail=True)


# ---- arguments -------------------------------------------------------------------------------------------------------

def test_value_errors():
    MR_ = pkg("motion_render")
    v, f, root = torch.zeros(2, 4, 5, 3), torch.tensor([[0, 1, 2]]), torch.zeros(2, 4, 3)
    ok = dict(root=root, size=(16, 16))
    bad = [
        (dict(vertices=torch.zeros(2, 4, 5, 2)), "last dim"),
        (dict(vertices=torch.zeros(2, 0, 5, 3), root=torch.zeros(2, 0, 3)), "no frame"),
        (dict(vertices=torch.zeros(2, 4, 5, 3, dtype=torch.int32)), "integer vertices"),
        (dict(faces=torch.zeros(1, 4, dtype=torch.int64)), "quads"),
        (dict(faces=torch.zeros(1, 3)), "float faces"),
        (dict(faces=torch.zeros(0, 3, dtype=torch.int64)), "no face"),
        (dict(root=torch.zeros(2, 3, 3)), "root frames"),
        (dict(root=torch.zeros(3, 4, 3)), "root batch"),
        (dict(root=torch.zeros(2, 4, 2)), "root dim"),
        (dict(normals=torch.zeros(2, 4, 4, 3)), "normals shape"),
        (dict(size=(16, 18)), "W % 4"),
        (dict(size=(2, 16)), "H < 4"),
        (dict(size=(16, 8196)), "W too large"),
        (dict(lengths=[4, 5]), "length > T"),
        (dict(lengths=[4, 0]), "length 0"),
        (dict(lengths=[4]), "lengths count"),
        (dict(camera=dict(elev=90.0)), "elev"),
        (dict(camera=dict(near=6.0)), "near >= dist"),
        (dict(camera="front"), "camera type"),
        (dict(frames=[4]), "frame index"),
        (dict(frames=0), "stride"),
        (dict(chain_width=2.0), "a render_motion style"),
        (dict(shininess=2.0), "unknown style"),
        (dict(body_color=(1.0, 0.0)), "colour length"),
        (dict(body_color=(1.0, 0.0, 1.5)), "colour range"),
        (dict(body_alpha=1.5), "alpha"),
        (dict(ambient=-0.1), "ambient"),
        (dict(trajectory_width=-1.0), "width"),
        (dict(light=(0.0, 0.0, 0.0)), "light"),
        (dict(light=(1.0, float("nan"), 0.0)), "light nan"),
    ]
    for change, what in bad:
        kw = dict(ok, vertices=v, faces=f)
        kw.update(change)
        with pytest.raises(ValueError):
            MR_.render_mesh(kw.pop("vertices"), kw.pop("faces"), kw.pop("lengths", None), **kw)
            pytest.fail(what)
    with pytest.raises(TypeError):
        MR_.render_mesh(v, f)                                      # root is required
    with pytest.raises(pkg("_lib").MdmError):
        MR_.render_mesh(v, f, **ok)                                # tensors on the CPU: no eager fallback
    assert set(MR_.MESH_STYLE) == {"background", "floor_color", "floor_alpha", "trajectory_color", "trajectory_alpha",
                                   "trajectory_width", "body_color", "body_alpha", "ambient", "light"}
    assert MR_.MESH_STYLE["body_alpha"] == 1.0
    for k in ("background", "floor_color", "floor_alpha", "trajectory_color", "trajectory_alpha", "trajectory_width"):
        assert MR_.MESH_STYLE[k] == MR_.STYLE[k]                   # §21's entries, unchanged
    for k, val in R.STYLE.items():
        assert tuple(np.ravel(MR_.MESH_STYLE[k])) == tuple(np.ravel(val)), k   # the restatement's defaults are the module's
    # joints as root: joint 0 is taken; one clip without the batch dim
    x, _, _, r, _, _ = MR_.check_mesh(torch.zeros(4, 5, 3), f, None, torch.ones(4, 22, 3), None, (16, 16))
    assert x.shape == (1, 4, 5, 3) and r.shape == (1, 4, 3)
    x, _, _, r, _, _ = MR_.check_mesh(v, f, None, torch.ones(2, 4, 22, 3), None, (16, 16))
    assert r.shape == (2, 4, 3)


def test_trainer_view_argument():
    tr = pkg("trainer").DDPMTrainer
    for view in ("sky", "Body", None):
        with pytest.raises(ValueError):
            tr._body_args(view, None, {})
    for view in ("root", "world"):
        assert tr._body_args(view, None, dict(fix_feet=True)) is None
        with pytest.raises(ValueError):
            tr._body_args(view, object(), {})                      # mesh= belongs to the body view
    kw = dict(fix_feet=True, blend=3, seed=1, offsets="o", pin_blend=2)
    got = tr._body_args("body", None, kw)
    assert got == dict(pin=None, offsets="o", fix_feet=True, blend=3, pin_blend=2) and kw == dict(seed=1)
    kw = dict(feet_blend=7, blend=9)
    assert tr._body_args("body", None, kw, "feet_blend")["blend"] == 7 and kw == dict(blend=9)   # generate_long's own blend stays
    with pytest.raises(ValueError):
        tr._body_args("body", None, dict(pin_targets=True))        # pins need the call's control arguments


def test_c_entry_argument_checks():
    lib = pkg("_lib").lib()
    ERR_ARG, ERR_UNSUPPORTED, OK = 1, 3, 0
    cam = (C.c_float * 8)(30, 0, 5, 40, 0, 0.9, 0, 0.1)
    style = (C.c_float * 20)(1, 1, 1, .5, .5, .5, .5, 0, 0, 1, 1, 1, .7, .7, .8, 1, .35, -.4, .6, .7)
    p = 4096  # stands for a device pointer: every check below returns before the device is touched

    def call(**change):
        a = dict(vertices=p, normals=None, faces=p, root=p, length=None, B=1, T=4, V=5, F=2, H=16, W=16, camera=cam, style=style,
                 mode=0, frames=None, n_frames=0, out=p, scratch=p, stream=None)
        a.update(change)
        return lib.mdm_mesh_render(*a.values())

    for name in ("vertices", "faces", "root", "camera", "style", "out", "scratch"):
        assert call(**{name: None}) == ERR_ARG, name
    for change in (dict(B=-1), dict(T=0), dict(V=0), dict(V=(1 << 24) + 1), dict(F=0), dict(F=(1 << 24) + 1), dict(H=3), dict(W=0),
                   dict(H=8193), dict(W=8196), dict(W=18), dict(mode=4), dict(mode=-1), dict(mode=2), dict(mode=3),
                   dict(frames=p, n_frames=0), dict(out=p + 2), dict(scratch=p + 4)):
        assert call(**change) == ERR_ARG, change
    for i, val in ((0, 90.0), (2, 0.0), (3, 180.0), (7, 6.0), (5, float("nan"))):
        c2 = (C.c_float * 8)(*cam)
        c2[i] = val
        assert call(camera=c2) == ERR_ARG, (i, val)
    for i, val in ((11, -1.0), (15, float("inf")), (17, 0.0)):
        s2 = (C.c_float * 20)(*style)
        s2[i] = val
        if i == 17:
            s2[18] = s2[19] = 0.0
        assert call(style=s2) == ERR_ARG, (i, val)
    assert call(B=65536) == ERR_UNSUPPORTED and call(frames=p, n_frames=65536) == ERR_UNSUPPORTED
    assert call(B=0) == OK                                          # no-ops: nothing is launched
    q = lib.mdm_mesh_render_scratch_floats
    assert q(1, 4, 4, 5, 2, 0) == 8 * 8 + 4 * 8 + 4 * 5 * 8 + 4 * 2 * 2
    assert q(1, 4, 4, 5, 2, 1) - q(1, 4, 4, 5, 2, 0) == 4 * 5 * 4 and q(0, 4, 4, 5, 2, 1) == 0 and q(3, 4, 0, 5, 2, 1) == 3 * 64
    assert q(2, 4, 3, 5, 1, 0) % 4 == 0 and q(2, 4, 3, 5, 1, 0) >= 2 * 64 + 6 * 8 + 6 * 5 * 8 + 6 * 2
    assert q(1, 0, 4, 5, 2, 0) == -1 and q(1, 4, 4, 0, 2, 0) == -1 and q(1, 4, 4, 5, 0, 0) == -1 and q(-1, 4, 4, 5, 2, 0) == -1
    assert q(65535, 196, 196, 1 << 24, 1 << 24, 1) > 1 << 40      # 64-bit


# ---- the conditions on the test inputs --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_inputs_are_decided_and_fp32_agrees(name):
    """Condition: non-decisive pixels <= 5 % of the pixels the body covers, in every image.  Measurement behind the deltas:
    the all-fp32 restatement against the fp64 one."""
    case = all_cases()[name]
    im, det = truth(name)
    im32 = R.run(case, ft=np.float32)
    dec, cov = R.masks(det, im.shape[:4])
    assert cov.sum() >= 100, "the body must show"
    for b in range(len(im)):
        for k in range(im.shape[1]):
            if det[b][k] is not None:
                assert (~dec[b, k]).sum() <= 0.05 * cov[b, k].sum(), (name, b, k, int((~dec[b, k]).sum()), int(cov[b, k].sum()))
    bad_dec, bad_nd, differ = R.check_against(im32, im, det)
    diff = np.abs(im.astype(np.int32) - im32.astype(np.int32)).max(-1)
    print(name, f"covered {int(cov.sum())}, non-decisive {int((~dec).sum())}; fp32 against fp64: {differ} pixels differ, "
                f"{int((diff > 1).sum())} by more than one level, of them decisive {bad_dec}, unexplained non-decisive {bad_nd}")
    assert bad_dec == 0 and bad_nd == 0


def test_deltas_measured():
    """The smallest deltas at which fp32 and fp64 agree on every decisive pixel: with all three at 0 every pixel but exact
    ties counts as decisive, and the count of pixels more than one level apart is what the header of mesh_render_ref.py
    records."""
    total = apart = 0
    for name, case in all_cases().items():
        im = truth(name)[0]
        im32 = R.run(case, ft=np.float32)
        diff = np.abs(im.astype(np.int32) - im32.astype(np.int32)).max(-1)
        total, apart = total + diff.size, apart + int((diff > 1).sum())
    print(f"fp32 against fp64 with the deltas at 0: {apart} of {total} pixels more than one level apart")
    assert apart == 0, "re-measure DELTA_E / DELTA_D / DELTA_N (4 x the smallest that excludes these pixels) and record them"


def test_a_vertex_that_is_not_finite_inside_the_length():
    """The rule for a NaN or infinite vertex in a valid frame: its faces are dropped and its coordinates are no part of MINS /
    MAXS.  The octahedron with such a vertex on a face without area is the octahedron's picture."""
    plain = all_cases()["octahedron_flat"]
    for ft in (np.float64, np.float32):
        assert np.array_equal(R.run(R.nonfinite_case(), ft=ft), R.run(plain, ft=ft))


# ---- watertightness ---------------------------------------------------------------------------------------------------

def hull(pts):
    """Convex hull of 2-D points, counter-clockwise (monotone chain)."""
    pts = sorted(map(tuple, pts))
    cross = lambda o, a, b: (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])
    lower, upper = [], []
    for seq, out in ((pts, lower), (pts[::-1], upper)):
        for q in seq:
            while len(out) >= 2 and cross(out[-2], out[-1], q) <= 0:
                out.pop()
            out.append(q)
    return np.array(lower[:-1] + upper[:-1])


def sphere(n_lat=7, n_lon=9, r=0.5):
    v = [(0.0, r, 0.0)]
    for i in range(1, n_lat):
        th = np.pi * i / n_lat
        v += [(r * np.sin(th) * np.cos(2 * np.pi * k / n_lon), r * np.cos(th), r * np.sin(th) * np.sin(2 * np.pi * k / n_lon))
              for k in range(n_lon)]
    v.append((0.0, -r, 0.0))
    f, last = [], len(v) - 1
    for k in range(n_lon):
        k1 = (k + 1) % n_lon
        f.append((0, 1 + k1, 1 + k))
        for i in range(n_lat - 2):
            a, b = 1 + i * n_lon, 1 + (i + 1) * n_lon
            f += [(a + k, a + k1, b + k1), (b + k1, a + k, b + k)]          # the two triangles wound differently on purpose
        f.append((last, last - n_lon + k, last - n_lon + k1))
    return np.array(v), np.array(f)


@pytest.mark.parametrize("ft", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("shape", ["octahedron", "box", "sphere"])
def test_watertight(shape, ft):
    v, f = {"octahedron": R.octahedron, "box": lambda: R.box((0, 0, 0), (0.4, 0.3, 0.2), 0.4), "sphere": sphere}[shape]()
    vv, root, _ = R._moving(v, B=2, T=4)
    H, W = 48, 64
    for cam in (None, R.CAMERA2):
        _, det = R.render(vv, f, None, root, H, W, camera=cam, ft=ft, detail=True)
        eye, r, u, fwd = R.RR.camera_basis(dict(R.RR.CAMERA, **(cam or {})), np.float64)
        F = H / 2 / np.tan(np.deg2rad(dict(R.RR.CAMERA, **(cam or {}))["fov"]) / 2)
        X, Y = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
        for b in range(2):
            lo = vv[b].reshape(-1, 3).min(0).astype(np.float64)
            for t in range(4):
                p = vv[b, t].astype(np.float64) - (root[b, t, 0], lo[1], root[b, t, 2]) - eye
                s = np.stack([W / 2 + F * (p @ r) / (p @ fwd), H / 2 - F * (p @ u) / (p @ fwd)], -1)
                h = hull(s)
                inside = np.full((H, W), np.inf)
                for a, c in zip(h, np.roll(h, -1, 0)):
                    e = c - a
                    inside = np.minimum(inside, (e[0] * (Y - a[1]) - e[1] * (X - a[0])) / np.hypot(*e))
                deep = inside > 0.5
                assert deep.sum() > 30
                assert det[b][t].covered[deep].all(), (shape, cam, b, t, int((deep & ~det[b][t].covered).sum()))


# ---- likely mistakes --------------------------------------------------------------------------------------------------

def strip():
    """An open mesh: two triangles of a bent quad, wound against each other."""
    v = np.array([[-0.5, -0.4, 0.1], [0.5, -0.4, -0.1], [0.5, 0.4, 0.1], [-0.5, 0.4, -0.1]])
    return v, np.array([(0, 1, 2), (0, 2, 3)[::-1]])


def mistake_inputs():
    cs = all_cases()
    dark_floor = dict(floor_color=(0.0, 0.0, 0.0), floor_alpha=0.9)
    sv, sf = strip()
    svv, sroot, _ = R._moving(sv, turn=0.2)
    strip_case = R._case(svv, sf, sroot)
    padded = cs["body_t2m_high_flat"]
    pv = padded.vertices.copy()
    for b, n in enumerate(padded.lengths):
        pv[b, n:] = 3.0                                            # what padding may hold
    padded = R._case(pv, padded.faces, padded.root, None, padded.camera)
    body = cs["body_t2m_high_flat"]
    return {"no_depth_test": cs["crossing_boxes"], "farthest_wins": cs["crossing_boxes"], "back_faces_culled": strip_case,
            "normal_not_turned": strip_case, "light_in_world": R._case(cs["octahedron_flat"].vertices, cs["octahedron_flat"].faces,
                                                                       cs["octahedron_flat"].root, None, R.CAMERA2),
            "mirror_x": body, "flip_y": body, "integer_centres": cs["body_kit_default_flat"], "root_kept": body,
            "floor_over_body": R._case(body.vertices, body.faces, body.root, None, body.camera, style=dark_floor),
            "past_length": body, "padding_in_extent": padded}


@pytest.mark.parametrize("wrong", R.WRONG)
def test_likely_mistakes_show(wrong):
    case = mistake_inputs()[wrong]
    right, det = R.run(case, detail=True)
    other = R.run(case, wrong=wrong)
    dec, _ = R.masks(det, right.shape[:4])
    per_image = [R.moved(right[b, k], other[b, k], dec[b, k]) for b in range(len(right)) for k in range(right.shape[1])]
    print(wrong, f"decisive pixels moved by >= 32 levels: most in one 48 x 64 image {max(per_image)}, over the batch {sum(per_image)}")
    assert right.shape[2:4] == (48, 64) and max(per_image) >= 20, (wrong, per_image)

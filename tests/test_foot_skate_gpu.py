"""GPU: foot-skate clean-up (mdm_foot_skate) against its restatement tests/foot_skate_ref.py.

* parity of joints, slide and pair counts: t2m and KIT, B = 3, T = 24, lengths 24 / 2 / 1; labels given as a tensor, read from
  normalised rows in place, and detected; blend 0, 5 and 12 (the swing gap is 4 frames);
* frames and lengths: T = 300 with a run across frames 255 | 256, one run over a whole clip, a clip without contact, targets
  beyond the leg's reach, n = 1 and 2, NaN past every length, every sample equal to its own run at B = 1, T = length;
* rotations from motion_to_joints_fk on the rows joints_to_motion makes of a walk clip: parity of R', R' offset + parent =
  joint, R'^T R' = I, untouched rotations bit-equal;
* through a tiny trainer: fix_feet on generate_joints, generate_long_joints and generate_rotations equals remove_foot_skate by
  hand, and the defaults are the parent's results bit for bit;
* bad arguments on the device path.

Tolerances.  A case's yardstick is the error of the restatement's all-fp32 form against its fp64 form on the same inputs, for
the quantity compared; GATE = 4 x that, the convention of tests/test_motion_fk_gpu.py.  A quantity whose yardstick is 0 is
compared bit for bit.  Nothing is gated against the kernel's own output, and no entry is left out: the clips keep the margins
that foot_skate_ref.walk_clip asserts.  tests/test_foot_skate_host.py shows that each likely mistake lies >= 100 gates away.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import pkg

import foot_skate_ref as FS
import test_motion_features_gpu as TF
import test_motion_fk_gpu as TK

pytestmark = pytest.mark.gpu

GATE = 4.0
HALF = np.full(4, 0.5, np.float32)
_MEMO = {}


def case(name, what="parity"):
    """Inputs and both forms of the restatement are computed once and shared; nothing writes to them."""
    if (name, what) not in _MEMO:
        sk = TF.ref_skel(name)
        if what == "parity":
            _MEMO[name, what] = (sk,) + FS.parity_case(sk, name)
        else:
            j, v = getattr(FS, what)(sk)
            _MEMO[name, what] = (sk, j[None], v[None], [len(j)])
    return _MEMO[name, what]


def held(what, got, w32, w64):
    """got against the fp64 form within GATE x the fp32 form's own error; bit for bit where that error is 0."""
    yard = float(np.abs(w32.astype(np.float64) - w64).max()) if w64.size else 0.0
    err = float(np.abs(got.astype(np.float64) - w64).max()) if w64.size else 0.0
    print(f"{what}: measured {err:.3g} yardstick {yard:.3g}")
    if yard == 0.0:
        assert np.array_equal(got, w32), what
    else:
        assert err <= GATE * yard, (what, err, yard)
    return err, yard


def compare(name, sk, j, lens, blend, dev_contacts, ref_kw, what, feet_thre=None, rotations=None):
    P = pkg("postprocess")
    w64 = FS.remove_foot_skate(sk, j, lens, blend=blend, ft=np.float64, rotations=rotations, **ref_kw)
    w32 = FS.remove_foot_skate(sk, j, lens, blend=blend, ft=np.float32, rotations=rotations, **ref_kw)
    rot = None if rotations is None else torch.from_numpy(rotations).cuda()
    res = P.remove_foot_skate(torch.from_numpy(j).cuda(), lens, dev_contacts, skeleton=name, feet_thre=feet_thre, blend=blend,
                              rotations=rot, return_slide=True)
    out, (slide, pairs) = res[0].cpu().numpy(), res[-1]
    assert out.shape == j.shape and out.dtype == np.float32 and slide.shape == (len(lens), 2, 4) and pairs.shape == (len(lens), 4)
    for b, n in enumerate(lens):
        assert not out[b, n:].any()
    held(f"{what} joints", out, w32[0], w64[0])
    held(f"{what} slide", slide.cpu().numpy(), w32[2], w64[2])
    assert np.array_equal(pairs.cpu().numpy(), w64[3]), what
    legs = FS.legs_of(sk)
    kept = [x for x in range(sk.J) if x not in [y for leg in legs for y in leg[1:]]]
    assert np.array_equal(out[:, :, kept], np.where(np.arange(j.shape[1])[None, :, None, None] < np.asarray(lens)[:, None, None, None],
                                                    j[:, :, kept], 0)), what  # hips and upper body: every bit
    if rotations is not None:
        r = res[1].cpu().numpy()
        held(f"{what} rotations", r, w32[1], w64[1])
        return out, r, w32, w64
    return out, None, w32, w64


@pytest.mark.parametrize("source", ["tensor", "rows", "detect"])
@pytest.mark.parametrize("name", ["t2m", "kit"])
def test_parity(name, source):
    sk, j, v, lens = case(name)
    rows, mean, std = FS.rows_with_contacts(v, lens, 12 * sk.J - 1, 3)
    for blend in (0, 5, 12):
        what = f"{name} {source} blend {blend}"
        if source == "tensor":
            compare(name, sk, j, lens, blend, torch.from_numpy(v).cuda(), dict(values=v, thre=HALF), what)
        elif source == "rows":
            thre = FS.row_thresholds(mean, std)
            assert np.array_equal(FS.value_labels(rows[..., -4:], thre), FS.value_labels(v, HALF))
            before = torch.from_numpy(rows).cuda()
            x = before.clone()
            compare(name, sk, j, lens, blend, (x, mean, std), dict(values=rows[..., -4:], thre=thre), what)
            assert torch.equal(x, before)  # read in place, not written
        else:
            thre = FS.FEET_THRE[name]
            compare(name, sk, j, lens, blend, None, dict(feet_thre=thre), what, feet_thre=None if blend else thre)


@pytest.mark.parametrize("what", ["long_clip", "whole_clip", "clamped_clip"])
def test_frames(what):
    """More frames than threads with a run across 255 | 256; one run over the whole clip; targets beyond reach."""
    sk, j, v, lens = case("t2m", what)
    out, _, w32, w64 = compare("t2m", sk, j, lens, 5, torch.from_numpy(v).cuda(), dict(values=v, thre=HALF), what)
    if what == "long_clip":
        compare("t2m", sk, j, lens, 5, None, dict(feet_thre=0.002), what + " detected")
    if what == "clamped_clip":
        assert w64[2][0, 1, [0, 2]].max() > 1e-4  # the ankles cannot be pinned where the leg does not reach


def test_no_contact_comes_back_bit_for_bit():
    P = pkg("postprocess")
    sk = TF.ref_skel("t2m")
    j, v = FS.walk_clip(sk, 24, 7, contact=False)
    jt = torch.from_numpy(j).cuda()[None]
    rot = torch.randn(1, 24, 22, 3, 3, generator=torch.Generator().manual_seed(0)).cuda()
    out, r, (slide, pairs) = P.remove_foot_skate(jt, None, torch.from_numpy(v).cuda()[None], rotations=rot, return_slide=True)
    assert torch.equal(out, jt) and torch.equal(r, rot) and not slide.any() and not pairs.any()


@pytest.mark.parametrize("n", [1, 2])
def test_the_shortest(n):
    sk, j, v, lens = case("t2m")
    b = lens.index(n)
    jj, vv = j[b:b + 1, :n], v[b:b + 1, :n]
    compare("t2m", sk, jj, [n], 5, torch.from_numpy(vv).cuda(), dict(values=vv, thre=HALF), f"n = {n} tensor")
    compare("t2m", sk, jj, [n], 5, None, dict(feet_thre=0.002), f"n = {n} detected")


def test_lengths():
    """NaN past every length changes nothing, and every sample equals its own run at B = 1, T = length."""
    P = pkg("postprocess")
    sk, j, v, lens = case("t2m")
    rows, mean, std = FS.rows_with_contacts(v, lens, 263, 3)
    rot = torch.randn(3, 24, 22, 3, 3, generator=torch.Generator().manual_seed(1)).cuda()
    jt, vt, xt = torch.from_numpy(j).cuda(), torch.from_numpy(v).cuda(), torch.from_numpy(rows).cuda()
    clean = {}
    for src, cont in (("tensor", vt), ("rows", (xt, mean, std)), ("detect", None)):
        clean[src] = P.remove_foot_skate(jt, lens, cont, rotations=rot, return_slide=True)
    for b, n in enumerate(lens):
        for t in (jt, vt, xt, rot):
            t[b, n:] = float("nan")
    for src, cont in (("tensor", vt), ("rows", (xt, mean, std)), ("detect", None)):
        o, r, (s, p) = P.remove_foot_skate(jt, lens, cont, rotations=rot, return_slide=True)
        for got, want in zip((o, r, s, p), (clean[src][0], clean[src][1]) + clean[src][2]):
            assert torch.equal(got, want), src
        for b, n in enumerate(lens):
            assert not o[b, n:].any() and not r[b, n:].any()
            c1 = None if cont is None else (cont[b:b + 1, :n] if src == "tensor" else (xt[b:b + 1, :n], mean, std))
            o1, r1, (s1, p1) = P.remove_foot_skate(jt[b:b + 1, :n], None, c1, rotations=rot[b:b + 1, :n], return_slide=True)
            assert torch.equal(o1[0], o[b, :n]) and torch.equal(r1[0], r[b, :n]) and torch.equal(s1[0], s[b]) and torch.equal(p1[0], p[b]), (src, b)


@pytest.mark.parametrize("name", ["t2m", "kit"])
def test_rotations(name):
    MF, P = pkg("motion_features"), pkg("postprocess")
    sk = TF.ref_skel(name)
    clip, vals = FS.walk_clip(sk, 25, 4, scale=FS.SCALE[name])
    F = 12 * sk.J - 1
    rows = MF.joints_to_motion(torch.from_numpy(clip).cuda()[None], skeleton=name)
    fj, fr, off = P.motion_to_joints_fk(rows, np.zeros(F, np.float32), np.ones(F, np.float32), skeleton=name, sigma=0.0,
                                        return_rotations=True, return_offsets=True)
    j, R, off = fj.cpu().numpy(), fr.cpu().numpy(), off[0].cpu().numpy().astype(np.float64)
    v = vals[None, :24]
    FS.check_margins(sk, j[0], FS.value_labels(v[0], HALF), 5)  # the inputs, not the kernel's output
    out, r, w32, w64 = compare(name, sk, j, [24], 5, torch.from_numpy(v).cuda(), dict(values=v, thre=HALF), f"{name} fk", rotations=R)
    legs = FS.legs_of(sk)
    turned = [y for leg in legs for y in leg[1:]]
    kept = [x for x in range(sk.J) if x not in turned]
    assert np.array_equal(r[:, :, kept], R[:, :, kept])
    assert np.abs(r[:, :, turned] - R[:, :, turned]).max() > 1e-3  # and the legs' did turn
    par = np.asarray(sk.parents)

    def residuals(jo, ro):
        jo, ro = np.asarray(jo, np.float64), np.asarray(ro, np.float64)
        bone = np.einsum("ntjab,jb->ntja", ro[:, :, turned], off[turned]) + jo[:, :, par[turned]] - jo[:, :, turned]
        orth = np.einsum("ntjab,ntjac->ntjbc", ro[:, :, turned], ro[:, :, turned]) - np.eye(3)
        return float(np.abs(bone).max()), float(np.abs(orth).max())

    (e_bone, e_orth), (y_bone, y_orth) = residuals(out, r), residuals(w32[0], w32[1])
    print(f"{name} R' offset + parent - joint: measured {e_bone:.3g} yardstick {y_bone:.3g}; R'^T R' - I: measured {e_orth:.3g} "
          f"yardstick {y_orth:.3g}")
    assert e_bone <= GATE * y_bone and e_orth <= GATE * y_orth


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_through_the_trainer():
    P = pkg("postprocess")
    tr = TF._tiny_trainer()
    mean, std = TK._mean_std(263, 22, 12)
    mean[-4:], std[-4:] = 0.5, 1.0  # generated contact columns around 0 then fall on both sides of the threshold
    caps, lens = ["a", "b", "c", "d"], torch.tensor([16, 16, 12, 9])
    opts = dict(seed=0, sampler="ddim", sample_steps=5, batch_size=2)
    motions = tr.generate(caps, lens, 263, **opts)
    x = torch.zeros(4, 16, 263, device="cuda")
    for i, (m, n) in enumerate(zip(motions, lens.tolist())):
        x[i, :n] = m[:n]
    labels = (x[..., -4:] > 0).cpu()
    assert labels.any() and not labels.all()
    # generate_joints: after the temporal filter, labels from the rows' own columns
    plain = tr.generate_joints(caps, lens, 263, mean, std, **opts)
    old = P.motion_to_joints(x, mean, std, lens, 22, 1.0)
    assert all(_bits(plain[i], old[i, :n]) for i, n in enumerate(lens.tolist()))  # the default: the parent's result
    fixed = tr.generate_joints(caps, lens, 263, mean, std, fix_feet=True, blend=3, **opts)
    want = P.remove_foot_skate(old, lens, (x, mean, std), blend=3)
    assert all(_bits(fixed[i], want[i, :n]) for i, n in enumerate(lens.tolist()))
    assert any(not _bits(fixed[i], plain[i]) for i in range(4))
    # from_rotations composes
    fk = tr.generate_joints(caps, lens, 263, mean, std, from_rotations=True, fix_feet=True, **opts)
    fj, fr, fo = P.motion_to_joints_fk(x, mean, std, lens, None, return_rotations=True, return_offsets=True)
    want = P.remove_foot_skate(fj, lens, (x, mean, std), blend=5)
    assert all(_bits(fk[i], want[i, :n]) for i, n in enumerate(lens.tolist()))
    assert all(_bits(a, fj[i, :n]) for i, (a, n) in enumerate(zip(tr.generate_joints(caps, lens, 263, mean, std, from_rotations=True, **opts),
                                                                 lens.tolist())))
    # generate_rotations: the rotations go through
    res = tr.generate_rotations(caps, lens, 263, mean, std, fix_feet=True, **opts)
    fj0, fr0, fo0 = P.motion_to_joints_fk(x, mean, std, lens, None, sigma=0.0, return_rotations=True, return_offsets=True)
    wj, wr = P.remove_foot_skate(fj0, lens, (x, mean, std), rotations=fr0)
    for i, n in enumerate(lens.tolist()):
        assert _bits(res[i][0], wj[i, :n]) and _bits(res[i][1], wr[i, :n]) and _bits(res[i][2], fo0[i])
    res0 = tr.generate_rotations(caps, lens, 263, mean, std, **opts)
    assert all(_bits(res0[i][0], fj0[i, :n]) and _bits(res0[i][1], fr0[i, :n]) for i, n in enumerate(lens.tolist()))
    # a long motion of two segments: one clean-up over the canvas, across the overlap
    scripts = [[("a", 16), ("b", 16)]]
    lopts = dict(overlap=4, seed=4, sampler="ddim", sample_steps=5)
    canvas = tr.generate_long(scripts, 263, **lopts)[0]
    lj = tr.generate_long_joints(scripts, 263, mean, std, fix_feet=True, **lopts)[0]
    base = P.motion_to_joints(canvas[None], mean, std, None, 22, 1.0)
    assert lj.shape == (28, 22, 3) and _bits(lj, P.remove_foot_skate(base, None, (canvas[None], mean, std))[0])
    assert _bits(tr.generate_long_joints(scripts, 263, mean, std, **lopts)[0], base[0])
    with pytest.raises(ValueError, match="fix_feet"):
        tr.generate_joints(caps, lens, 263, mean, std, joints_num=21, fix_feet=True, **opts)


def test_bad_arguments_on_the_device_path():
    P, L, MF = pkg("postprocess"), pkg("_lib"), pkg("motion_features")
    lib = L.lib()
    j = torch.zeros(2, 8, 22, 3, device="cuda")
    o, sc = torch.empty_like(j), torch.empty(2, 8, 4, 2, device="cuda")
    rot = torch.zeros(2, 8, 22, 3, 3, device="cuda")
    v = torch.zeros(2, 8, 4, device="cuda")
    thre = (C.c_float * 4)(0.5, 0.5, 0.5, 0.5)
    s = MF._skeleton_struct(MF.SKELETONS["t2m"])

    def call(joints=j, skel=s, contact=v, stride=4, th=thre, feet=0.002, blend=5, B=2, T=8, rin=None, out=o, rout=None, scratch=sc):
        p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())  # noqa: E731
        return lib.mdm_foot_skate(p(joints), None, C.byref(skel) if skel is not None else None, p(contact), C.c_int64(stride), th,
                                  C.c_double(feet), C.c_int32(blend), C.c_int32(B), C.c_int32(T), p(rin), p(out), p(rout), None,
                                  None, p(scratch), C.c_void_p(L.stream_ptr()))

    ARG, UNSUPPORTED = 1, 3
    assert call() == 0 and call(contact=None) == 0 and call(rin=rot, rout=torch.empty_like(rot)) == 0 and call(B=0) == 0
    for kw in (dict(joints=None), dict(skel=None), dict(out=None), dict(scratch=None), dict(th=None), dict(T=0), dict(blend=-1),
               dict(B=-1), dict(stride=3), dict(contact=None, feet=-1.0), dict(contact=None, feet=float("nan")), dict(rin=rot),
               dict(rout=rot), dict(out=j), dict(rin=rot, rout=rot)):
        assert call(**kw) == ARG, kw
    odd = MF._skeleton_struct(MF.SKELETONS["t2m"])
    odd.feet[0], odd.feet[1] = odd.feet[1], odd.feet[0]  # toe and ankle swapped: no chain ends ankle, toe
    assert call(skel=odd) == ARG
    odd = MF._skeleton_struct(MF.SKELETONS["t2m"])
    odd.feet[2], odd.feet[3] = odd.feet[0], odd.feet[1]  # one leg twice
    assert call(skel=odd) == ARG
    odd = MF._skeleton_struct(MF.SKELETONS["t2m"])
    odd.feet[1] = 99                                     # an index outside the skeleton
    assert call(skel=odd) == ARG
    assert call(T=P.foot_skate_max_frames() + 1) == UNSUPPORTED  # returns before any launch
    assert P.foot_skate_max_frames() >= pkg("trainer").MAX_JOINTS_FRAMES
    torch.cuda.synchronize()
    with pytest.raises(L.MdmError):
        P.remove_foot_skate(j.cpu())                                   # a CPU tensor
    with pytest.raises(ValueError):
        P.remove_foot_skate(j, None, torch.zeros(2, 8, 3, device="cuda"))
    with pytest.raises(L.MdmError):
        P.remove_foot_skate(j, None, v.cpu())                          # labels on the CPU
    with pytest.raises(ValueError):
        P.remove_foot_skate(j, [8, 9])

"""CPU restatement of the foot-skate clean-up (TEST INFRASTRUCTURE ONLY), and the clips it is tested on.

The reference project has no such function (it only produces the contact labels, ``foot_detect``,
utils/motion_process.py:39-62), so the yardstick is this restatement of DESIGN.md §18 in numpy: ``ft=np.float64`` is the truth,
``ft=np.float32`` is the same arithmetic with every step in fp32, double only where §18 says double (the anchor's sum, the
slide's sum, the comparison of a squared foot speed with ``feet_thre``).  The input joints, label values and rotations are fp32
in both forms.  The error of the fp32 form against the fp64 form on a case's inputs is that case's yardstick.

A (frame, leg) is worked on where one of its two foot joints is in a run or within ``blend`` frames of one; every other
(frame, leg), and every other joint, is copied.

``WRONG`` names the mistakes an implementation most easily makes; ``wrong=name`` makes one of them.

``walk_clip`` builds a walking skeleton by construction and refuses a clip whose frames do not keep the margins that make a
comparison of every entry meaningful (``check_margins``).
"""
from __future__ import annotations

import numpy as np

WRONG = ("neg_bend",         # the knee bends along -w
         "anchor_first",     # a run's anchor is its first frame
         "unnormalised",     # the blend weights are not divided by max(1, wL + wR)
         "left_only",        # only the contact on the left of a frame is blended in
         "toe_translated",   # the toe is moved by its delta instead of aimed
         "q_right",          # R' = R Q
         "label_order")      # labels read as (ankle, ankle, toe, toe)


def legs_of(sk):
    """((hip, knee, ankle, toe), (hip, knee, ankle, toe)): the last four entries of the chains that end in the toes."""
    legs = []
    for ankle, toe in (sk.feet[0:2], sk.feet[2:4]):
        c = [c for c in sk.chains if len(c) >= 4 and c[-1] == toe and c[-2] == ankle]
        assert c, (ankle, toe)
        legs.append(tuple(c[0][-4:]))
    return tuple(legs)


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _reject(e, u):
    return e - _dot(e, u)[..., None] * u


def _unit(a, n):
    return a / n[..., None]


def _same_bits(a, b):
    ui = np.uint32 if a.dtype == np.float32 else np.uint64
    return (np.ascontiguousarray(a).view(ui) == np.ascontiguousarray(b).view(ui)).all(-1)


def detect_labels(sk, p, feet_thre):
    """foot_detect on one clip (n, J, 3) in p's dtype: (labels (n, 4) bool, squared speeds (n - 1, 4))."""
    n = len(p)
    lab = np.zeros((n, 4), bool)
    s2 = np.zeros((0, 4), p.dtype)
    if n > 1:
        d = p[1:, list(sk.feet)] - p[:-1, list(sk.feet)]
        s2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        lab[:-1] = s2.astype(np.float64) < np.float64(feet_thre)
        lab[-1] = lab[-2]
    return lab, s2


def value_labels(values, thre):
    """Given values (n, 4) against four thresholds, both fp32 as the device reads them."""
    return np.asarray(values, np.float32) > np.asarray(thre, np.float32)


def row_thresholds(mean, std, contact_thre=0.5):
    """The thresholds of the normalised contact columns: (contact_thre - mean) / std in fp64, rounded to fp32 once."""
    m, s = np.asarray(mean, np.float64)[-4:], np.asarray(std, np.float64)[-4:]
    return ((contact_thre - m) / s).astype(np.float32)


def _fade(k, blend, ft):
    x = ft(k) / ft(blend + 1)
    x2 = x * x
    return ft(1) - (ft(3) * x2 - ft(2) * (x2 * x))


def deltas(sk, p, lab, blend, ft, wrong=None):
    """-> (delta (n, 4, 2), active (n, 4) bool) of one clip p (n, J, 3) of dtype ft with labels lab (n, 4)."""
    n = len(p)
    delta, act = np.zeros((n, 4, 2), ft), np.zeros((n, 4), bool)
    for f in range(4):
        j = sk.feet[f]
        t = 0
        while t < n:
            if not lab[t, f]:
                t += 1
                continue
            e, sx, sz = t, np.float64(0), np.float64(0)
            while e < n and lab[e, f]:
                sx, sz = sx + np.float64(p[e, j, 0]), sz + np.float64(p[e, j, 2])
                e += 1
            ax, az = ft(sx / np.float64(e - t)), ft(sz / np.float64(e - t))
            if wrong == "anchor_first":
                ax, az = p[t, j, 0], p[t, j, 2]
            delta[t:e, f, 0], delta[t:e, f, 1] = ax - p[t:e, j, 0], az - p[t:e, j, 2]
            act[t:e, f] = True
            t = e
        for t in range(n):
            if lab[t, f]:
                continue
            kl = next((k for k in range(1, blend + 1) if t - k >= 0 and lab[t - k, f]), 0)
            kr = next((k for k in range(1, blend + 1) if t + k < n and lab[t + k, f]), 0)
            if wrong == "left_only":
                kr = 0
            if not (kl or kr):
                continue
            wl, wr = (_fade(kl, blend, ft) if kl else ft(0)), (_fade(kr, blend, ft) if kr else ft(0))
            dl = delta[t - kl, f] if kl else np.zeros(2, ft)
            dr = delta[t + kr, f] if kr else np.zeros(2, ft)
            den = ft(1) if wrong == "unnormalised" else max(ft(1), wl + wr)
            delta[t, f] = (wl * dl + wr * dr) / den
            act[t, f] = True
    return delta, act


def _turn(R, old, new, ft, wrong=None):
    """R' = Q R, Q the shortest arc from bone old to bone new; rows (m, 3, 3), (m, 3), (m, 3)."""
    same = _same_bits(old, new)
    with np.errstate(all="ignore"):
        x, y = _unit(old, np.sqrt(_dot(old, old))), _unit(new, np.sqrt(_dot(new, new)))
        v = _cross(x, y)
        s = ft(1) + _dot(x, y)
        K = np.zeros(R.shape, ft)
        K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -v[:, 2], v[:, 1], v[:, 2], -v[:, 0], -v[:, 1], v[:, 0]
        Q, out = np.zeros(R.shape, ft), np.zeros(R.shape, ft)
        for r in range(3):
            for c in range(3):
                k2 = K[:, r, 0] * K[:, 0, c] + K[:, r, 1] * K[:, 1, c] + K[:, r, 2] * K[:, 2, c]
                Q[:, r, c] = (ft(1 if r == c else 0) + K[:, r, c]) + k2 / s
        for r in range(3):
            for c in range(3):
                if wrong == "q_right":
                    out[:, r, c] = R[:, r, 0] * Q[:, 0, c] + R[:, r, 1] * Q[:, 1, c] + R[:, r, 2] * Q[:, 2, c]
                else:
                    out[:, r, c] = Q[:, r, 0] * R[:, 0, c] + Q[:, r, 1] * R[:, 1, c] + Q[:, r, 2] * R[:, 2, c]
    out[same] = R[same]
    return out


def slide_of(sk, p, lab, ft):
    """Per foot joint the mean |XZ step| over the pairs of neighbouring contact frames, and the pair counts."""
    out, cnt = np.zeros(4, ft), np.zeros(4, np.int32)
    for f in range(4):
        j, acc = sk.feet[f], np.float64(0)
        for t in range(len(p) - 1):
            if lab[t, f] and lab[t + 1, f]:
                dx, dz = p[t + 1, j, 0] - p[t, j, 0], p[t + 1, j, 2] - p[t, j, 2]
                acc += np.float64(np.sqrt(dx * dx + dz * dz))
                cnt[f] += 1
        out[f] = ft(acc / np.float64(cnt[f])) if cnt[f] else ft(0)
    return out, cnt


def clean_clip(sk, joints, lab, blend, ft=np.float64, rotations=None, wrong=None, diag=None):
    """One clip (n, J, 3) fp32 with labels (n, 4) bool -> (joints' (n, J, 3), rotations' or None, slide (2, 4), pairs (4,)) in
    ``ft``.  ``diag``: a dict that receives the margins of every (frame, leg) worked on."""
    p = np.asarray(joints, np.float32).astype(ft)
    lab = np.asarray(lab, bool)
    R = None if rotations is None else np.asarray(rotations, np.float32).astype(ft)
    use = lab[:, [0, 2, 1, 3]] if wrong == "label_order" else lab
    delta, act = deltas(sk, p, use, blend, ft, wrong)
    out, Rout = p.copy(), None if R is None else R.copy()
    for leg, (jh, jk, ja, jt) in enumerate(legs_of(sk)):
        on = act[:, 2 * leg] | act[:, 2 * leg + 1]
        if not on.any():
            continue
        h, k, a, toe = p[on, jh], p[on, jk], p[on, ja], p[on, jt]
        da, dt = delta[on, 2 * leg], delta[on, 2 * leg + 1]
        kh, ak = k - h, a - k
        l1, l2 = np.sqrt(_dot(kh, kh)), np.sqrt(_dot(ak, ak))
        tgt = a.copy()
        tgt[:, 0], tgt[:, 2] = a[:, 0] + da[:, 0], a[:, 2] + da[:, 1]
        d = tgt - h
        nd = np.sqrt(_dot(d, d))
        u = _unit(d, nd)
        lo, hi = np.abs(l1 - l2) * (ft(1) + ft(1e-4)) + ft(1e-6), (l1 + l2) * (ft(1) - ft(1e-4))
        dist = np.minimum(np.maximum(nd, lo), hi)
        bound = ft(1e-10) * (l1 * l1)
        w = _reject(kh, u)
        w2 = _dot(w, w)
        w_own = w2.copy()
        for axis in ((0, 0, 1), (1, 0, 0)):
            bad = w2 < bound
            if bad.any():
                e = np.broadcast_to(np.asarray(axis, ft), u.shape)
                w = np.where(bad[:, None], _reject(e, u), w)
                w2 = _dot(w, w)
        w = _unit(w, np.sqrt(w2))
        if wrong == "neg_bend":
            w = -w
        ca = ((l1 * l1 + dist * dist) - l2 * l2) / ((ft(2) * l1) * dist)
        ca = np.minimum(np.maximum(ca, ft(-1)), ft(1))
        sa = np.sqrt(ft(1) - ca * ca)
        k2 = h + l1[:, None] * (ca[:, None] * u + sa[:, None] * w)
        a2 = h + dist[:, None] * u
        ta = toe - a
        l3 = np.sqrt(_dot(ta, ta))
        tt = toe.copy()
        tt[:, 0], tt[:, 2] = toe[:, 0] + dt[:, 0], toe[:, 2] + dt[:, 1]
        v = tt - a2
        v2 = _dot(v, v)
        small = v2 < ft(1e-10) * (l3 * l3)
        with np.errstate(all="ignore"):
            t2 = np.where(small[:, None], a2 + ta, a2 + l3[:, None] * _unit(v, np.sqrt(v2)))
        if wrong == "toe_translated":
            t2 = tt
        out[on, jk], out[on, ja], out[on, jt] = k2, a2, t2
        if R is not None:
            Rout[on, jk] = _turn(R[on, jk], kh, k2 - h, ft, wrong)
            Rout[on, ja] = _turn(R[on, ja], ak, a2 - k2, ft, wrong)
            Rout[on, jt] = _turn(R[on, jt], ta, t2 - a2, ft, wrong)
        if diag is not None:
            cos = [_dot(o, m) / np.sqrt(_dot(o, o) * _dot(m, m)) for o, m in ((kh, k2 - h), (ak, a2 - k2), (ta, t2 - a2))]
            diag.setdefault("bend", []).extend(np.sqrt(w_own) / l1)
            diag.setdefault("reach", []).extend((l1 + l2 - nd) / (l1 + l2))
            diag.setdefault("edge", []).extend(np.minimum(np.abs(nd - hi) / hi, np.abs(nd - lo) / lo))
            diag.setdefault("aim", []).extend(np.sqrt(v2) / l3)
            diag.setdefault("cos", []).extend(np.min(cos, axis=0))
    before, pairs = slide_of(sk, p, lab, ft)
    after, _ = slide_of(sk, out, lab, ft)
    return out, Rout, np.stack([before, after]), pairs


def remove_foot_skate(sk, joints, lengths=None, values=None, thre=None, *, feet_thre=None, blend=5, rotations=None,
                      ft=np.float64, wrong=None, diag=None):
    """Batch form of the device function: joints (B, T, J, 3) fp32 -> (joints', rotations' or None, slide (B, 2, 4), pairs
    (B, 4)), zero past each length.  Labels: ``values`` (B, T, 4) against ``thre`` (4,), or detected with ``feet_thre``."""
    joints = np.asarray(joints, np.float32)
    B, T = joints.shape[:2]
    lengths = [T] * B if lengths is None else [int(n) for n in lengths]
    out = np.zeros(joints.shape, ft)
    rot = None if rotations is None else np.zeros(np.asarray(rotations).shape, ft)
    slide, pairs = np.zeros((B, 2, 4), ft), np.zeros((B, 4), np.int32)
    for b, n in enumerate(lengths):
        if values is None:
            lab = detect_labels(sk, joints[b, :n].astype(ft), feet_thre)[0]
        else:
            lab = value_labels(np.asarray(values)[b, :n], thre)
        o, r, s, c = clean_clip(sk, joints[b, :n], lab, blend, ft, None if rotations is None else np.asarray(rotations)[b, :n],
                                wrong, diag)
        out[b, :n], slide[b], pairs[b] = o, s, c
        if rot is not None:
            rot[b, :n] = r
    return out, rot, slide, pairs


def check_margins(sk, joints, lab, blend, reachable=True, speeds=None, feet_thre=None):
    """Assert the margins of DESIGN.md §18 on every (frame, leg) the fp64 algorithm works on for one clip; -> the diag dict."""
    diag = {}
    clean_clip(sk, joints, lab, blend, np.float64, diag=diag)
    if diag:
        d = {k: np.asarray(v) for k, v in diag.items()}
        assert d["bend"].min() >= 0.1, ("bend", d["bend"].min())
        assert d["aim"].min() >= 0.2, ("aim", d["aim"].min())
        assert d["cos"].min() > 0.0, ("a bone turned by 90 degrees or more", d["cos"].min())
        if reachable:
            assert d["reach"].min() >= 0.02, ("reach", d["reach"].min())
        else:
            assert d["edge"].min() >= 1e-3, ("reach boundary", d["edge"].min())
            assert d["reach"].min() < 0, "no target beyond reach"
    if speeds is not None and speeds.size:
        assert np.abs(speeds.astype(np.float64) - feet_thre).min() >= 1e-3 * feet_thre
    return diag


def _smooth(x):
    return x * x * (3 - 2 * x)


def walk_clip(sk, n, seed, slide=0.004, *, scale=1.0, period=12, stance=8, speed=0.02, hip_height=0.74, contact=True,
              blends=(0, 5, 12), feet_thre=None, reachable=True, follow=False):
    """A walking skeleton by construction: -> (joints (n, J, 3) fp32, label values (n, 4) fp32).  The pelvis moves on a
    straight line that is not along an axis, at a height that keeps the legs bent; each foot stands ``stance`` frames of every
    ``period`` on an anchor under its hip and drifts there by ``slide`` a frame (the ankle along a line, the toe also around
    the ankle); knees come from the two-bone solve with a forward bend; the toe lies ahead of and below the ankle; the rest of
    the body is rigid.  The toe's label comes on one frame after the ankle's.  Label values are >= 0.1 away from 0.5.
    ``contact=False``: every label off.  ``follow=True``: the planted feet drift along the walking direction, after the hip,
    and the knees bend sideways, so that a target ahead of or behind the hip stays clear of the thigh's own direction.  Refuses (AssertionError) a clip that breaks a margin for the given labels at any of
    ``blends``, and, with ``feet_thre``, for the detected labels."""
    rng = np.random.RandomState(seed)
    J = len(sk.raw)
    legs = legs_of(sk)
    phi = rng.uniform(0.3, 1.2)
    c, s = np.cos(phi), np.sin(phi)
    Ry = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    fwd, up = Ry @ np.array([0.0, 0, 1]), np.array([0.0, 1, 0])
    l1, l2, l3 = 0.42 * scale, 0.40 * scale, 0.14 * scale
    length = (0.1 + 0.15 * rng.rand(J)) * scale
    for b in range(1, J):  # shoulders wider than hips, as on a person: the facing direction of joints_to_motion depends on it
        if sk.raw[b][0] != 0:
            length[b] = (0.1 if b in sk.face[:2] else 0.22) * scale
    rest = np.zeros((J, 3))
    for ch in sk.chains:
        for a, b in zip(ch[:-1], ch[1:]):
            axis = sk.raw[b].astype(np.float64)
            if axis[0] != 0:  # hips and collars slope down: never exactly along or against the skeleton's own axis, whose
                axis = (axis + (0, -0.3, 0)) / np.linalg.norm(axis + (0, -0.3, 0))  # sign the KIT tables have mirrored
            rest[b] = rest[a] + axis * length[b]
    t = np.arange(n, dtype=np.float64)
    start = np.array([rng.uniform(-1, 1), 0, rng.uniform(-1, 1)]) * scale

    def pelvis(tt):
        tt = np.asarray(tt, np.float64)
        return start + (speed * scale * tt)[..., None] * fwd + up * (hip_height * scale - rest[legs[0][0], 1])

    out = pelvis(t)[:, None] + (Ry @ rest.T).T[None] + (0.01 * scale * np.sin(0.7 * t))[:, None, None] * up
    values = np.zeros((n, 4), np.float32)
    for leg, (jh, jk, ja, jt) in enumerate(legs):
        off = leg * (period // 2)
        drift = rng.uniform(0, 2 * np.pi)
        drift = (fwd if follow else np.array([np.cos(drift), 0, np.sin(drift)])) * slide * scale
        hip_off = Ry @ rest[jh]

        def planted(tt):  # the ankle at stance frame tt
            m = (tt + off) // period
            mid = m * period - off + (stance - 1) / 2
            q = pelvis(mid) + hip_off + drift * (tt - mid)
            return np.array([q[0], 0.08 * scale, q[2]])

        for i in range(n):
            cph = (i + off) % period
            if cph < stance:
                a = planted(i)
            else:
                first = i - cph  # this cycle's first frame
                x = _smooth((cph - stance + 1) / (period - stance + 1))
                a = (1 - x) * planted(first + stance - 1) + x * planted(first + period)
                a[1] += 0.1 * scale * np.sin(np.pi * (cph - stance + 1) / (period - stance + 1))
            h = out[i, jh]
            d = a - h
            if np.linalg.norm(d) > 0.97 * (l1 + l2):  # a leg that cannot reach its foothold drags the foot
                a = h + d / np.linalg.norm(d) * 0.97 * (l1 + l2)
                d = a - h
            dist = np.linalg.norm(d)
            u = d / dist
            w = Ry @ np.array([1.0 - 2 * leg, 0, 0]) if follow else fwd
            w = w - (w @ u) * u
            w /= np.linalg.norm(w)
            ca = (l1 * l1 + dist * dist - l2 * l2) / (2 * l1 * dist)
            out[i, jk] = h + l1 * (ca * u + np.sqrt(1 - ca * ca) * w)
            out[i, ja] = a
            yaw = 0.1 * np.sin(0.5 * i + leg) * min(slide, 0.004) / 0.004
            ahead = np.cos(yaw) * fwd + np.sin(yaw) * (Ry @ np.array([1.0, 0, 0]))
            pitch = np.arcsin(0.06 / 0.14)
            out[i, jt] = a + l3 * (np.cos(pitch) * ahead - np.sin(pitch) * up)
            on_a, on_t = contact and cph < stance, contact and 1 <= cph < stance
            values[i, 2 * leg] = rng.uniform(0.6, 1.0) if on_a else rng.uniform(0.0, 0.4)
            values[i, 2 * leg + 1] = rng.uniform(0.6, 1.0) if on_t else rng.uniform(0.0, 0.4)
    joints = out.astype(np.float32)
    lab = value_labels(values, np.full(4, 0.5, np.float32))
    assert np.abs(values - 0.5).min() >= 0.1
    for blend in blends:
        check_margins(sk, joints, lab, blend, reachable)
        if feet_thre is not None:
            dl, s2 = detect_labels(sk, joints.astype(np.float64), feet_thre)
            check_margins(sk, joints, dl, blend, reachable, s2, feet_thre)
            check_margins(sk, joints, dl, blend, reachable, detect_labels(sk, joints, feet_thre)[1], feet_thre)
    return joints, values


def batch(clips, T=None):
    """[(joints (n_i, J, 3), values (n_i, 4))] -> (joints (B, T, J, 3), values (B, T, 4), lengths) zero-padded fp32."""
    T = T or max(len(j) for j, _ in clips)
    joints = np.zeros((len(clips), T) + clips[0][0].shape[1:], np.float32)
    values = np.zeros((len(clips), T, 4), np.float32)
    for b, (j, v) in enumerate(clips):
        joints[b, :len(j)], values[b, :len(j)] = j, v
    return joints, values, [len(j) for j, _ in clips]


SCALE = {"t2m": 1.0, "kit": 5.0}       # the KIT skeleton's unit, as its feet_thre (0.05 against 0.002) has it
FEET_THRE = {"t2m": 0.002, "kit": 0.05}


def parity_case(sk, name):
    """The GPU parity inputs of one skeleton: B = 3, T = 24, lengths 24 / 2 / 1; the swing of 4 frames is a gap shorter than
    blend 5.  -> (joints, values, lengths)."""
    kw = dict(scale=SCALE[name], feet_thre=FEET_THRE[name])
    return batch([walk_clip(sk, 24, 1, **kw), walk_clip(sk, 2, 2, **kw), walk_clip(sk, 1, 3, **kw)])


def long_clip(sk):
    """T = 300 (more frames than threads), the left ankle's run of frames 240 .. 269 crossing 255 | 256."""
    return walk_clip(sk, 300, 5, period=40, stance=30, blends=(5,), feet_thre=0.002)


def whole_clip(sk):
    """Both ankles in contact on every frame: one run over the whole clip."""
    return walk_clip(sk, 40, 6, period=80, stance=80, speed=0.005, blends=(5,))


def clamped_clip(sk):
    """The feet follow the hip and the hip is high: towards the ends of a run the pinned target is beyond the leg's reach."""
    return walk_clip(sk, 48, 8, 0.018, period=40, stance=30, hip_height=0.865, blends=(5,), reachable=False, follow=True)


def rows_with_contacts(values, lengths, F, seed):
    """Normalised rows (B, T, F) fp32 whose last four columns de-normalise to ``values``, with their mean / std."""
    rng = np.random.RandomState(seed)
    mean, std = (0.1 * rng.randn(F)).astype(np.float32), (0.5 + rng.rand(F)).astype(np.float32)
    rows = rng.randn(*values.shape[:2], F).astype(np.float32)
    rows[..., -4:] = ((values.astype(np.float64) - mean[-4:]) / std[-4:]).astype(np.float32)
    return rows, mean, std

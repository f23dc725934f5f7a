"""CPU restatement of exact reach (TEST INFRASTRUCTURE ONLY), and the clips it is tested on.

The reference project has no such function, so the yardstick is this restatement of DESIGN.md §28 in numpy: ``ft=np.float64``
is the truth, ``ft=np.float32`` is the same arithmetic with every step in fp32, double only where §28 says double (the sum of
the error report's mean).  Joints, targets, weights and rotations are fp32 in both forms.  The error of the fp32 form against the
fp64 form on a case's inputs is that case's yardstick.

Per sample, n = its length:
* a limb is (root, mid, end, tip), tip = -1 without one; frame t < n is a pin frame of a limb iff W[t, end, c] > 0 for all c;
* delta[t] = G[t, end] - p[t, end] in a pin frame; outside, the nearest pin frame within ``blend`` on either side,
  w = 1 - smoothstep(k / (blend + 1)), delta = (wL dL + wR dR) / max(1, wL + wR); neither: the (frame, limb) is copied;
* §18's two-bone solve with the root fixed and the target end + delta (reach clamp, bend plane, fallbacks);
* tip' = end' + Q2 (tip - end), Q2 the shortest arc from the old mid -> end bone to the new one;
* R'[mid] = Q1 R[mid], R'[end] = Q2 R[end], R'[tip] = Q2 R[tip], Q1 the shortest arc of the root -> mid bone;
* report per limb: mean (double, frame order) and maximum of |p[end] - G[end]| over the pin frames before and after, the pin
  count and the count of pin frames whose target lay outside the reach clamp.

``WRONG`` names the mistakes an implementation most easily makes; ``wrong=name`` makes one of them.

``reach_clip`` builds its inputs by construction and refuses a clip whose frames do not keep the margins that make a comparison
of every entry meaningful (``check_margins``).
"""
from __future__ import annotations

import numpy as np

from foot_skate_ref import _cross, _dot, _fade, _reject, _same_bits, _unit

WRONG = ("neg_bend",         # the mid joint bends along -w
         "xz_only",          # delta in XZ only, as foot-skate has it
         "left_only",        # only the pin frame on the left of a frame is blended in
         "unnormalised",     # the blend weights are not divided by max(1, wL + wR)
         "tip_translated",   # the tip moves by the end joint's step instead of being carried
         "q_right",          # R' = R Q
         "pin_any")          # a pin frame where any one coordinate is weighted

LIMB_NAMES = ("right_leg", "left_leg", "right_arm", "left_arm")


def limbs_of(sk):
    """The default limb table (4, 4) of a skeleton namespace (chains, feet, face): right_leg, left_leg, right_arm, left_arm."""
    legs = []
    for ankle, toe in (sk.feet[0:2], sk.feet[2:4]):
        c = [c for c in sk.chains if len(c) >= 4 and c[-1] == toe and c[-2] == ankle]
        assert c, (ankle, toe)
        legs.append(c[0])
    legs.sort(key=lambda c: sk.face[0] not in c)
    arms = sorted([c for c in sk.chains if c[0] != 0], key=lambda c: sk.face[2] not in c)
    assert len(arms) == 2
    return np.asarray([tuple(c[-4:]) for c in legs] + [tuple(c[-3:]) + (-1,) for c in arms], np.int32)


def pin_flags(W, limbs, wrong=None):
    """(n, J, 3) weights -> (n, L) bool, from the weights alone."""
    on = np.asarray(W)[:, [q[2] for q in limbs]] > 0
    return on.any(-1) if wrong == "pin_any" else on.all(-1)


def deltas(p, G, pin, limbs, blend, ft, wrong=None):
    """-> (delta (n, L, 3), active (n, L) bool) of one clip p (n, J, 3) of dtype ft; G is read in pin frames only."""
    n, nl = len(p), len(limbs)
    delta, act = np.zeros((n, nl, 3), ft), np.zeros((n, nl), bool)
    for l, q in enumerate(limbs):
        e = q[2]
        for t in np.flatnonzero(pin[:, l]):
            delta[t, l] = G[t, e].astype(ft) - p[t, e]
            if wrong == "xz_only":
                delta[t, l, 1] = 0
            act[t, l] = True
        for t in range(n):
            if pin[t, l]:
                continue
            kl = next((k for k in range(1, blend + 1) if t - k >= 0 and pin[t - k, l]), 0)
            kr = next((k for k in range(1, blend + 1) if t + k < n and pin[t + k, l]), 0)
            if wrong == "left_only":
                kr = 0
            if not (kl or kr):
                continue
            wl, wr = (_fade(kl, blend, ft) if kl else ft(0)), (_fade(kr, blend, ft) if kr else ft(0))
            dl = delta[t - kl, l] if kl else np.zeros(3, ft)
            dr = delta[t + kr, l] if kr else np.zeros(3, ft)
            den = ft(1) if wrong == "unnormalised" else max(ft(1), wl + wr)
            delta[t, l] = (wl * dl + wr * dr) / den
            act[t, l] = True
    return delta, act


def _arc(old, new, ft):
    """Q (m, 3, 3), the shortest arc from bone old to bone new, and where the bone keeps every bit (Q unused there)."""
    same = _same_bits(old, new)
    with np.errstate(all="ignore"):
        x, y = _unit(old, np.sqrt(_dot(old, old))), _unit(new, np.sqrt(_dot(new, new)))
        v = _cross(x, y)
        s = ft(1) + _dot(x, y)
        K = np.zeros(old.shape[:1] + (3, 3), ft)
        K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -v[:, 2], v[:, 1], v[:, 2], -v[:, 0], -v[:, 1], v[:, 0]
        Q = np.zeros(K.shape, ft)
        for r in range(3):
            for c in range(3):
                k2 = K[:, r, 0] * K[:, 0, c] + K[:, r, 1] * K[:, 1, c] + K[:, r, 2] * K[:, 2, c]
                Q[:, r, c] = (ft(1 if r == c else 0) + K[:, r, c]) + k2 / s
    return Q, same


def _apply(Q, same, v):
    """Q v per row, v where the bone kept every bit."""
    out = np.stack([Q[:, r, 0] * v[:, 0] + Q[:, r, 1] * v[:, 1] + Q[:, r, 2] * v[:, 2] for r in range(3)], -1)
    out[same] = v[same]
    return out


def _turn(Q, same, R, wrong=None):
    out = np.zeros(R.shape, R.dtype)
    for r in range(3):
        for c in range(3):
            if wrong == "q_right":
                out[:, r, c] = R[:, r, 0] * Q[:, 0, c] + R[:, r, 1] * Q[:, 1, c] + R[:, r, 2] * Q[:, 2, c]
            else:
                out[:, r, c] = Q[:, r, 0] * R[:, 0, c] + Q[:, r, 1] * R[:, 1, c] + Q[:, r, 2] * R[:, 2, c]
    out[same] = R[same]
    return out


def _reach(p, delta_l, q):
    """nd, lo, hi, l1, l2 and the vectors of the solve for limb q on frames p (m, J, 3) with deltas (m, 3)."""
    ft = p.dtype.type
    h, k, a = p[:, q[0]], p[:, q[1]], p[:, q[2]]
    kh, ak = k - h, a - k
    l1, l2 = np.sqrt(_dot(kh, kh)), np.sqrt(_dot(ak, ak))
    d = (a + delta_l) - h
    nd = np.sqrt(_dot(d, d))
    lo, hi = np.abs(l1 - l2) * (ft(1) + ft(1e-4)) + ft(1e-6), (l1 + l2) * (ft(1) - ft(1e-4))
    return h, a, kh, ak, l1, l2, d, nd, lo, hi


def _gap(p, g):
    d = p - g
    return np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])


def pin_clip(limbs, joints, G, W, blend, ft=np.float64, rotations=None, wrong=None, diag=None):
    """One clip (n, J, 3) fp32 with targets and weights (n, J, 3) -> (joints' (n, J, 3), rotations' or None, error (L, 2, 2):
    [before | after] x [mean | max], counts (L, 2): pin frames, clamped pin frames) in ``ft``.  ``diag``: a dict that receives the
    margins of every (frame, limb) worked on."""
    p = np.asarray(joints, np.float32).astype(ft)
    G, W = np.asarray(G, np.float32), np.asarray(W, np.float32)
    R = None if rotations is None else np.asarray(rotations, np.float32).astype(ft)
    true_pin = pin_flags(W, limbs)
    pin = pin_flags(W, limbs, wrong)
    delta, act = deltas(p, G, pin, limbs, blend, ft, wrong)
    out, Rout = p.copy(), None if R is None else R.copy()
    err, counts = np.zeros((len(limbs), 2, 2), ft), np.zeros((len(limbs), 2), np.int32)
    for l, q in enumerate(limbs):
        on = act[:, l]
        if on.any():
            h, a, kh, ak, l1, l2, d, nd, lo, hi = _reach(p[on], delta[on, l], q)
            u = _unit(d, nd)
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
            Q2, same2 = _arc(ak, a2 - k2, ft)
            out[on, q[1]], out[on, q[2]] = k2, a2
            if q[3] >= 0:
                ta = p[on, q[3]] - a
                out[on, q[3]] = a2 + (ta if wrong == "tip_translated" else _apply(Q2, same2, ta))
            if R is not None:
                Q1, same1 = _arc(kh, k2 - h, ft)
                Rout[on, q[1]] = _turn(Q1, same1, R[on, q[1]], wrong)
                Rout[on, q[2]] = _turn(Q2, same2, R[on, q[2]], wrong)
                if q[3] >= 0:
                    Rout[on, q[3]] = _turn(Q2, same2, R[on, q[3]], wrong)
            if diag is not None:
                cos = [_dot(o, m) / np.sqrt(_dot(o, o) * _dot(m, m)) for o, m in ((kh, k2 - h), (ak, a2 - k2))]
                diag.setdefault("bend", []).extend(np.sqrt(w_own) / l1)
                diag.setdefault("reach", []).extend(np.minimum((hi - nd) / hi, (nd - lo) / np.maximum(lo, ft(1e-3) * hi)))
                diag.setdefault("edge", []).extend(np.minimum(np.abs(nd - hi) / hi, np.abs(nd - lo) / lo))
                diag.setdefault("cos", []).extend(np.min(cos, axis=0))
        ts = np.flatnonzero(true_pin[:, l])  # the report is about the pins asked for, whatever the variant did
        if len(ts):
            for s, pts in enumerate((p, out)):
                gaps = _gap(pts[ts, q[2]], G[ts, q[2]].astype(ft))
                acc = np.float64(0)
                for g in gaps:
                    acc += np.float64(g)
                err[l, s] = ft(acc / np.float64(len(ts))), gaps.max()
            _, _, _, _, _, _, _, nd, lo, hi = _reach(p[ts], G[ts, q[2]].astype(ft) - p[ts, q[2]], q)
            counts[l] = len(ts), int(((nd < lo) | (nd > hi)).sum())
    return out, Rout, err, counts


def pin_limbs(limbs, joints, lengths, G, W, *, blend=5, rotations=None, ft=np.float64, wrong=None, diag=None):
    """Batch form of the device function: joints (B, T, J, 3) fp32 -> (joints', rotations' or None, error (B, L, 2, 2), counts
    (B, L, 2)), zero past each length."""
    joints = np.asarray(joints, np.float32)
    B, T = joints.shape[:2]
    lengths = [T] * B if lengths is None else [int(n) for n in lengths]
    W = np.broadcast_to(np.asarray(W, np.float32), joints.shape)
    out = np.zeros(joints.shape, ft)
    rot = None if rotations is None else np.zeros(np.asarray(rotations).shape, ft)
    err, counts = np.zeros((B, len(limbs), 2, 2), ft), np.zeros((B, len(limbs), 2), np.int32)
    for b, n in enumerate(lengths):
        o, r, e, c = pin_clip(limbs, joints[b, :n], np.asarray(G)[b, :n], W[b, :n], blend, ft,
                              None if rotations is None else np.asarray(rotations)[b, :n], wrong, diag)
        out[b, :n], err[b], counts[b] = o, e, c
        if rot is not None:
            rot[b, :n] = r
    return out, rot, err, counts


def check_margins(limbs, joints, G, W, blend, reachable=True):
    """Assert the margins of DESIGN.md §28 on every (frame, limb) the fp64 algorithm works on for one clip; -> the diag dict."""
    W = np.asarray(W)
    assert ((W == 0) | (W >= 0.1)).all(), "weights are exactly 0 or >= 0.1"
    diag = {}
    pin_clip(limbs, joints, G, W, blend, np.float64, diag=diag)
    if diag:
        d = {k: np.asarray(v) for k, v in diag.items()}
        assert d["bend"].min() >= 0.1, ("bend", d["bend"].min())
        if reachable:
            assert d["reach"].min() >= 0.02, ("reach", d["reach"].min())
        else:
            assert d["edge"].min() >= 1e-3, ("reach boundary", d["edge"].min())
            assert d["reach"].min() < 0, "no target beyond reach"
        assert d["cos"].min() > 0.0, ("a bone turned by 90 degrees or more", d["cos"].min())
    return diag


def reach_clip(sk, limbs, n, seed, pins, *, scale=1.0, offset=0.06, stretch=0.8, bend=1.0, blends=(0, 5, 12), reachable=True,
               beyond=(), nan=False, distract=True):
    """Inputs by construction: -> (joints (n, J, 3), targets (n, J, 3), weights (n, J, 3)) fp32.  The torso is rigid and moves
    along a straight line that is not along an axis, bobbing a little; every limb of ``limbs`` hangs from its root at
    ``stretch`` of its full length along a direction that swings slowly, its mid joint from the two-bone solve bent along a
    fixed direction (``bend`` scales how far the bend direction leans out of the limb's own), its tip (if any) ahead of and below the end joint.
    ``pins``: {limb index: frames}; there the end joint's target is ``offset`` away in a direction of the limb's own and all
    three weights are drawn from [0.1, 2).  ``beyond``: limb indices whose targets lie ``1.25`` limb lengths from the root
    along the limb instead (out of reach; needs ``reachable=False``).  ``distract``: weights that pin nothing as well: the
    pelvis' XZ path, a height on every end joint outside its pin frames, a full target on every mid joint.  ``nan``: targets
    are NaN wherever the weight is 0.  Refuses (AssertionError) a clip that breaks a margin at any of ``blends``."""
    rng = np.random.RandomState(seed)
    J = len(sk.raw)
    phi = rng.uniform(0.3, 1.2)
    c, s = np.cos(phi), np.sin(phi)
    Ry = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    fwd, up, side = Ry @ np.array([0.0, 0, 1]), np.array([0.0, 1, 0]), Ry @ np.array([1.0, 0, 0])
    length = (0.1 + 0.15 * rng.rand(J)) * scale
    rest = np.zeros((J, 3))
    for ch in sk.chains:
        for a, b in zip(ch[:-1], ch[1:]):
            axis = sk.raw[b].astype(np.float64)
            if axis[0] != 0:
                axis = (axis + (0, -0.3, 0)) / np.linalg.norm(axis + (0, -0.3, 0))
            rest[b] = rest[a] + axis * length[b]
    t = np.arange(n, dtype=np.float64)
    start = np.array([rng.uniform(-1, 1), 0.9, rng.uniform(-1, 1)]) * scale
    pelvis = start + (0.02 * scale * t)[:, None] * fwd + (0.01 * scale * np.sin(0.7 * t))[:, None] * up
    out = pelvis[:, None] + (Ry @ rest.T).T[None]
    G, W = np.zeros((n, J, 3)), np.zeros((n, J, 3), np.float32)
    for l, q in enumerate(limbs):
        jr, jm, je, jt = (int(v) for v in q)
        leg = jt >= 0
        l1, l2, l3 = ((0.42, 0.40, 0.14) if leg else (0.30, 0.27, 0.0))
        l1, l2, l3 = l1 * scale, l2 * scale, l3 * scale
        ph = rng.uniform(0, 2 * np.pi)
        sgn = 1.0 if l % 2 == 0 else -1.0
        swing = 0.35 * np.sin(0.09 * t + ph)
        lift = 0.0 if leg else 0.5 + 0.2 * np.sin(0.05 * t + ph)  # arms reach forward and a little outwards
        direction = (-np.cos(swing) * np.cos(lift))[:, None] * up + (np.sin(swing) + np.sin(lift))[:, None] * fwd + \
            (0.15 * sgn) * side[None]
        direction /= np.linalg.norm(direction, axis=1, keepdims=True)
        h = out[:, jr]
        dist = stretch * (l1 + l2)
        w = (fwd if leg else -fwd) * bend + (1 - bend) * direction + 0.2 * sgn * side  # knees forward, elbows back
        w = w - (w * direction).sum(1, keepdims=True) * direction
        w /= np.linalg.norm(w, axis=1, keepdims=True)
        ca = (l1 * l1 + dist * dist - l2 * l2) / (2 * l1 * dist)
        out[:, jm] = h + l1 * (ca * direction + np.sqrt(1 - ca * ca) * w)
        out[:, je] = h + dist * direction
        if leg:
            pitch = np.arcsin(0.06 / 0.14)
            out[:, jt] = out[:, je] + l3 * (np.cos(pitch) * fwd - np.sin(pitch) * up)
        frames = np.asarray(sorted(pins.get(l, ())), int)
        assert len(frames) == 0 or (0 <= frames.min() and frames.max() < n)
        push = rng.randn(3)
        push = offset * scale * push / np.linalg.norm(push)
        for f in frames:
            wob = 0.3 * offset * scale * np.array([np.sin(0.4 * f + l), np.cos(0.3 * f), np.sin(0.2 * f + 1)])
            if l in beyond:
                far = 1.25 if (f - frames.min()) % 7 < 4 else 0.9  # some pin frames beyond reach, some within
                G[f, je] = h[f] + far * (l1 + l2) * direction[f] + wob
            else:
                G[f, je] = out[f, je] + push + wob
            W[f, je] = rng.uniform(0.1, 2.0, 3)
        if distract:
            rest_frames = np.setdiff1d(np.arange(n), frames)
            G[rest_frames, je, 1], W[rest_frames, je, 1] = out[rest_frames, je, 1] + 0.1 * scale, 0.7   # a height: not a pin
            G[:, jm], W[:, jm] = out[:, jm] + 0.2 * scale, 1.5                                         # an elbow / knee: not an end
    if distract:
        G[:, 0, [0, 2]], W[:, 0, [0, 2]] = pelvis[:, [0, 2]] + 0.05 * scale, 1.0                       # a root path
    joints, G = out.astype(np.float32), G.astype(np.float32)
    if nan:
        G[W == 0] = np.nan
    for blend in blends:
        check_margins(limbs, joints, G, W, blend, reachable)
    return joints, G, W


def batch(clips, T=None):
    """[(joints (n_i, J, 3), targets, weights)] -> (joints, targets, weights (B, T, J, 3), lengths) zero-padded fp32."""
    T = T or max(len(c[0]) for c in clips)
    out = [np.zeros((len(clips), T) + clips[0][0].shape[1:], np.float32) for _ in range(3)]
    for b, c in enumerate(clips):
        for o, v in zip(out, c):
            o[b, :len(v)] = v
    return out[0], out[1], out[2], [len(c[0]) for c in clips]


SCALE = {"t2m": 1.0, "kit": 5.0}  # the KIT skeleton's unit

# the pins of the GPU cases, {limb index: frames}: an interval and a single keyframe (two pin frames 3 apart: closer than
# blend 5), a keyframe alone, an interval on an arm, two keyframes 4 apart
PARITY_PINS = {0: list(range(10, 19)) + [22], 1: [30], 2: list(range(5, 15)), 3: [20, 24]}


def parity_case(sk, name, limbs=None, pins=None, nan=False):
    """The GPU parity inputs of one skeleton: B = 3, T = 40, lengths 40 / 2 / 1.  -> (joints, targets, weights, lengths)."""
    limbs = limbs_of(sk) if limbs is None else limbs
    pins = PARITY_PINS if pins is None else pins
    kw = dict(scale=SCALE[name], nan=nan)
    short = {l: [0] for l in range(len(limbs)) if l % 2 == 0}
    return batch([reach_clip(sk, limbs, 40, 1, pins, **kw), reach_clip(sk, limbs, 2, 2, {0: [1], len(limbs) - 1: [0, 1]}, **kw),
                  reach_clip(sk, limbs, 1, 3, short, **kw)])


def long_clip(sk, limbs=None):
    """T = 300 (more frames than threads), the right arm pinned over frames 250 .. 262 crossing 255 | 256."""
    limbs = limbs_of(sk) if limbs is None else limbs
    return reach_clip(sk, limbs, 300, 5, {2: range(250, 263), 0: [100], 3: [299], 1: [0]}, blends=(5,))


def clamped_clip(sk, limbs=None):
    """The right arm's and the left leg's targets lie beyond reach on some pin frames and within on others."""
    limbs = limbs_of(sk) if limbs is None else limbs
    return reach_clip(sk, limbs, 40, 8, {2: range(8, 24), 1: range(20, 34), 0: [5]}, blends=(5,), reachable=False, beyond=(1, 2))

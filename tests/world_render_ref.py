"""CPU restatement of the world view's image (TEST INFRASTRUCTURE ONLY), and the worlds it is tested on.

The image is defined by DESIGN.md §26; this is that definition in numpy, written from it, generic in the float type:
``ft=np.float64`` is the truth, ``ft=np.float32`` the same arithmetic in fp32.  Camera, capsule coverage and compositing are
render_ref's (§21); the polygon coverage is restated here from homogeneous edge lines, as §21 defines it, so that a corner the
near plane throws far off the image costs the fp32 form nothing.  The style table is ``motion_render.WORLD_STYLE`` itself: its
values are choices, not something to get right twice.

The two decisions of the picture, the order of the items and which faces of a box the eye sees, get no tolerance; ``margins``
returns how far a world's inputs are from flipping either, and the tests assert that it is far.

``WRONG`` names the mistakes an implementation most easily makes; ``wrong=name`` makes one of them.
"""
from __future__ import annotations

import numpy as np

import render_ref as RR
from conftest import pkg

PAD, SPHERE, CAPSULE, BOX, HALF_SPACE = 0, 1, 2, 3, 4

WRONG = ("index_order",         # items composited in index order
         "near_to_far",         # items composited near to far
         "yaw_sign",            # a box's yaw with the wrong sign
         "six_faces",           # all six faces of a box drawn
         "track_frame0",        # a track's record of frame 0 used in every frame
         "inactive_drawn",      # an inactive record drawn (as the track's last live record)
         "past_length",         # a character drawn past its own length
         "sphere_flat",         # a sphere's radius not divided by its depth
         "ground_lowest",       # the ground at the extent's lowest y
         "root_relative",       # characters drawn relative to their own root, as in §21
         "halfspace_tangent")   # a half-space's square spanned by its normal and one tangent


def style_table(style=None):
    return dict(pkg("motion_render").WORLD_STYLE, **(style or {}))


def prim_box(q):
    """The bounding box (lo, hi) of one record in float64, or None for a kind without one."""
    q = np.asarray(q, np.float64)
    kind = int(q[0])
    if kind == SPHERE:
        return q[4:7] - q[7], q[4:7] + q[7]
    if kind == CAPSULE:
        return np.minimum(q[4:7], q[7:10]) - q[10], np.maximum(q[4:7], q[7:10]) + q[10]
    if kind == BOX:
        c, s = abs(q[10]), abs(q[11])
        half = np.array([c * q[7] + s * q[9], q[8], s * q[7] + c * q[9]])
        return q[4:7] - half, q[4:7] + half
    return None


def extent(joints, lens, prims, tracks):
    """(lo, hi) of one world in float64: joints (C, T, J, 3), lens (C,), prims (K, 12), tracks (T, Km, 12)."""
    longest = max(lens)
    pts = [np.asarray(joints[c][:n], np.float64).reshape(-1, 3) for c, n in enumerate(lens) if n > 0]
    boxes = [prim_box(q) for q in prims] + [prim_box(q) for t in range(longest) for q in tracks[t]]
    for bx in boxes:
        if bx is not None:
            pts.append(np.stack(bx))
    pts = np.concatenate(pts)
    return pts.min(0), pts.max(0)


def ground_of(prims):
    """The ground rule: (height, prims without the record that is the ground)."""
    prims = np.array(prims, np.float32).reshape(-1, 12)
    for k, q in enumerate(prims):
        if q[0] == HALF_SPACE and q[1] == 1 and tuple(q[4:7]) == (0.0, 1.0, 0.0):
            height = float(q[7])
            prims[k] = 0
            return height, prims
    return 0.0, prims


def _polygon(corners, F, cx, cy, X, Y, ft):
    """Coverage of the convex polygon of view-space corners (clipped already): clamp(0.5 + the smallest signed distance to its
    edge lines), the lines formed from the homogeneous image points (F x, -F y, z)."""
    m = len(corners)
    if m < 3:
        return None
    h = [np.array([F * v[0], -F * v[1], v[2]], ft) for v in corners]
    s = None
    for i in range(m):
        a, b = h[i], h[(i + 1) % m]
        ln = np.cross(a, b).astype(ft)
        norm = np.sqrt(ln[0] * ln[0] + ln[1] * ln[1])
        if not norm > 0:
            continue
        side = sum((ln * q).sum() / q[2] for q in h)
        if side == 0:
            return None
        ln = ln * (ft(1) if side > 0 else ft(-1)) / norm
        d = ln[0] * (X - cx) + ln[1] * (Y - cy) + ln[2]
        s = d if s is None else np.minimum(s, d)
    return None if s is None else np.clip(ft(0.5) + s, ft(0), ft(1))


def box_frame(q, eye, ft, wrong=None):
    """(centre, half extents, cos, sin, the eye in the box's frame)."""
    q = np.asarray(q, np.float32).astype(ft)
    c, s = q[10], (-q[11] if wrong == "yaw_sign" else q[11])
    d = eye - q[4:7]
    return q[4:7], q[7:10], c, s, np.array([c * d[0] - s * d[2], d[1], s * d[0] + c * d[2]], ft)


def _records_at(tracks, t, wrong):
    """The track records of frame t."""
    if wrong == "track_frame0":
        return tracks[0]
    rec = np.array(tracks[t])
    if wrong == "inactive_drawn":
        for k in range(rec.shape[0]):
            s = t
            while rec[k, 0] == PAD and s > 0:
                s -= 1
                rec[k] = tracks[s][k]
    return rec


def render_one(chains, joints, lens, prims, tracks, H, W, camera, style=None, ground=0.0, ft=np.float64, frames=None, wrong=None,
               keys_out=None):
    """One world: joints (C, T, J, 3) fp32, lens (C,), prims (K, 12) and tracks (T, Km, 12) fp32 records -> (NF, H, W, 3) uint8.
    ``keys_out``: a list that receives, per drawn frame, the depth keys of the frame's drawn items and every box's
    |e_axis - h_axis| (see ``margins``)."""
    st = style_table(style)
    cam = dict(RR.CAMERA, **(camera or {}))
    joints = np.asarray(joints, np.float32)
    Cn, T = joints.shape[:2]
    prims = np.asarray(prims, np.float32).reshape(-1, 12)
    tracks = np.asarray(tracks, np.float32).reshape(T, -1, 12)
    lens = [int(n) for n in lens]
    frames = list(range(T)) if frames is None else list(frames)
    out = np.zeros((len(frames), H, W, 3), np.uint8)
    longest = max(lens)
    if longest < 1:
        return out
    lo, hi = _extent_ft(joints, lens, prims, tracks, ft)
    mid, half_diag = (lo + hi) / ft(2), np.sqrt(((hi - lo) ** 2).sum()) / ft(2)
    gy = lo[1] if wrong == "ground_lowest" else ft(ground)
    eye, r, u, f = RR.camera_basis(cam, ft)
    near = ft(cam["near"])
    F = ft(H) / ft(2) / np.tan(np.deg2rad(ft(cam["fov"])) / ft(2))
    cx, cy = ft(W) / ft(2), ft(H) / ft(2)
    X, Y = np.meshgrid(np.arange(W).astype(ft) + ft(0.5), np.arange(H).astype(ft) + ft(0.5))
    points = lambda w: ft(w) * ft(H) / ft(1440)
    nchains = len(chains)
    chain_alpha = np.broadcast_to(np.asarray(st["chain_alpha"], np.float64), (Cn, nchains))
    chain_width = np.broadcast_to(np.asarray(st["chain_width"], np.float64), (Cn, nchains))
    traj_alpha = np.broadcast_to(np.asarray(st["trajectory_alpha"], np.float64), (Cn,))
    traj_width = np.broadcast_to(np.asarray(st["trajectory_width"], np.float64), (Cn,))
    solid, shade = np.asarray(st["solid_color"], ft), np.asarray(st["shade"], ft)

    def view(p):
        d = np.asarray(p, ft) - eye
        return np.array([(r * d).sum(), (u * d).sum(), (f * d).sum()], ft)

    def pixel(v):
        return (cx + F * v[0] / v[2], cy - F * v[1] / v[2])

    def stroke(segments, w):
        """The maximum over view-space segments (clipped here) of the capsule coverage."""
        cov = np.zeros((H, W), ft)
        for a, b in segments:
            s = RR._clip_segment(a, b, near)
            if s is not None:
                cov = np.maximum(cov, RR.capsule(pixel(s[0]), pixel(s[1]), w, X, Y, ft))
        return cov

    def quad(c, corners, colour, alpha):
        cov = _polygon(RR._clip_polygon(corners, near), F, cx, cy, X, Y, ft)
        return c if cov is None else RR._over(c, cov, colour, alpha, ft)

    def draw_prim(c, q, margins):
        q32 = np.asarray(q, np.float32)
        q = q32.astype(ft)
        kind, keep_in = int(q[0]), q[1] < 0
        if kind == SPHERE:
            v = view(q[4:7])
            w = F * q[7] / (ft(1) if wrong == "sphere_flat" else v[2])
            return RR._over(c, RR.capsule(pixel(v), pixel(v), w, X, Y, ft), solid, st["solid_alpha"], ft) if not v[2] - q[7] < near else c
        if kind == CAPSULE:
            s = RR._clip_segment(view(q[4:7]), view(q[7:10]), near)
            if s is None:
                return c
            w = F * q[10] / ((s[0][2] + s[1][2]) / ft(2))
            return RR._over(c, RR.capsule(pixel(s[0]), pixel(s[1]), w, X, Y, ft), solid, st["solid_alpha"], ft)
        if kind == BOX:
            centre, h, co, si, el = box_frame(q32, eye, ft, wrong)
            margins.extend(float(abs(abs(el[a]) - h[a])) for a in range(3))

            def corner(l):
                return view(centre + np.array([co * l[0] + si * l[2], l[1], -si * l[0] + co * l[2]], ft))

            vis = [0 if keep_in else (1 if el[a] > h[a] else (-1 if el[a] < -h[a] else 0)) for a in range(3)]
            faces = [(a, sg) for a in range(3) for sg in ((-1, 1) if wrong == "six_faces" and not keep_in else (vis[a],)) if sg != 0]
            for a, sg in faces:
                b1, b2 = (a + 1) % 3, (a + 2) % 3
                cs = []
                for s1, s2 in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
                    l = np.zeros(3, ft)
                    l[a], l[b1], l[b2] = sg * h[a], s1 * h[b1], s2 * h[b2]
                    cs.append(corner(l))
                c = quad(c, cs, solid * shade[(1, 0, 2)[a]], st["solid_alpha"])
            segs = []
            for a in range(3):
                b1, b2 = (a + 1) % 3, (a + 2) % 3
                for s1 in (-1, 1):
                    for s2 in (-1, 1):
                        if keep_in or wrong == "six_faces" or vis[b1] == s1 or vis[b2] == s2:
                            l0, l1 = np.zeros(3, ft), np.zeros(3, ft)
                            l0[a], l1[a] = -h[a], h[a]
                            l0[b1] = l1[b1] = s1 * h[b1]
                            l0[b2] = l1[b2] = s2 * h[b2]
                            segs.append((corner(l0), corner(l1)))
            return RR._over(c, stroke(segs, points(st["edge_width"])), st["edge_color"], 1.0, ft)
        if kind == HALF_SPACE:
            n = q[4:7]
            centre = mid - ((n * mid).sum() - q[7]) * n
            t1 = np.array([1, 0, 0], ft) if n[0] == 0 and n[2] == 0 else np.array([-n[2], 0, n[0]], ft) / np.sqrt(n[2] * n[2] + n[0] * n[0])
            t2 = np.cross(n, t1).astype(ft)
            if wrong == "halfspace_tangent":
                t1, t2 = n, t1
            cs = [view(centre + half_diag * (a * t1 + b * t2)) for a, b in ((1, 1), (-1, 1), (-1, -1), (1, -1))]
            an = np.abs(n)
            axis = 0 if an[1] >= an[0] and an[1] >= an[2] else (1 if an[0] >= an[2] else 2)
            return quad(c, cs, solid * shade[axis], st["solid_alpha"])
        return c

    def prim_key(q):
        q = np.asarray(q, np.float32).astype(ft)
        kind = int(q[0])
        if kind == PAD or (q[1] < 0 and kind != BOX):
            return None
        if kind == CAPSULE:
            return view((q[4:7] + q[7:10]) / ft(2))[2]
        if kind == HALF_SPACE:
            return view(mid - ((q[4:7] * mid).sum() - q[7]) * q[4:7])[2]
        return view(q[4:7])[2]

    for k, t in enumerate(frames):
        if t < 0 or t >= longest:
            continue
        c = np.empty((H, W, 3), ft)
        c[:] = np.asarray(st["background"], ft)
        x0, x1, z0, z1 = lo[0] - ft(0.5), hi[0] + ft(0.5), lo[2] - ft(0.5), hi[2] + ft(0.5)
        c = quad(c, [view((x0, gy, z0)), view((x1, gy, z0)), view((x1, gy, z1)), view((x0, gy, z1))], st["floor_color"], st["floor_alpha"])
        for ch in range(Cn):
            if 1 < t < lens[ch]:
                pts = [view((joints[ch, s, 0, 0], gy, joints[ch, s, 0, 2])) for s in range(t)]
                c = RR._over(c, stroke(list(zip(pts[:-1], pts[1:])), points(traj_width[ch])),
                             st["trajectory_colors"][ch % len(st["trajectory_colors"])], traj_alpha[ch], ft)
        items, margins = [], []  # (key, index, draw)
        recs = list(prims) + list(_records_at(tracks, t, wrong))
        for i, q in enumerate(recs):
            key = prim_key(q)
            if key is not None:
                items.append((key, i, (lambda cc, q=q: draw_prim(cc, q, margins))))
        for ch in range(Cn):
            if not (t < lens[ch] or (wrong == "past_length" and lens[ch] > 0)):
                continue
            p = joints[ch, t].astype(ft)
            if wrong == "root_relative":
                p = p - p[0] * np.array([1, 0, 1], ft)
            colours = st["character_colors"][ch % len(st["character_colors"])]
            for g, chain in enumerate(chains):
                vs = [view(p[j]) for j in chain]
                key = sum(v[2] for v in vs) / ft(len(vs))
                items.append((key, len(recs) + ch * nchains + g,
                              (lambda cc, vs=vs, ch=ch, g=g, colours=colours: RR._over(
                                  cc, stroke(list(zip(vs[:-1], vs[1:])), points(chain_width[ch, g])), colours[g % len(colours)],
                                  chain_alpha[ch, g], ft))))
        if wrong == "near_to_far":
            items.sort(key=lambda it: (it[0], it[1]))
        elif wrong != "index_order":
            items.sort(key=lambda it: (-it[0], it[1]))
        for _, _, draw in items:
            c = draw(c)
        if keys_out is not None:
            keys_out.append((sorted(float(it[0]) for it in items), margins))
        out[k] = np.floor(np.clip(ft(255) * c + ft(0.5), 0, 255)).astype(np.uint8)
    return out


def _extent_ft(joints, lens, prims, tracks, ft):
    """The extent in ``ft``: the boxes' sums are rounded in it, as the device rounds them in fp32."""
    longest = max(lens)
    pts = [np.asarray(joints[c][:n], np.float32).astype(ft).reshape(-1, 3) for c, n in enumerate(lens) if n > 0]
    for q in list(prims) + [q for t in range(longest) for q in tracks[t]]:
        q = np.asarray(q, np.float32).astype(ft)
        kind = int(q[0])
        if kind == SPHERE:
            pts.append(np.stack([q[4:7] - q[7], q[4:7] + q[7]]))
        elif kind == CAPSULE:
            pts.append(np.stack([np.minimum(q[4:7], q[7:10]) - q[10], np.maximum(q[4:7], q[7:10]) + q[10]]))
        elif kind == BOX:
            c, s = abs(q[10]), abs(q[11])
            half = np.array([c * q[7] + s * q[9], q[8], s * q[7] + c * q[9]], ft)
            pts.append(np.stack([q[4:7] - half, q[4:7] + half]))
    pts = np.concatenate(pts)
    return pts.min(0), pts.max(0)


def render(chains, joints, lens, prims, tracks, H, W, camera, style=None, ground=None, ft=np.float64, frames=None, wrong=None,
           keys_out=None):
    """Batch form of the device function: joints (B, C, T, J, 3) fp32, lens (B, C), prims (B, K, 12) or None, tracks
    (B, T, Km, 12) or None, ground None (the rule), one height or (B,) -> (B, NF, H, W, 3) uint8."""
    joints = np.asarray(joints, np.float32)
    B, Cn, T = joints.shape[:3]
    prims = np.zeros((B, 0, 12), np.float32) if prims is None else np.asarray(prims, np.float32)
    tracks = np.zeros((B, T, 0, 12), np.float32) if tracks is None else np.asarray(tracks, np.float32)
    out = []
    for b in range(B):
        if ground is None:
            g, pr = ground_of(prims[b])
        else:
            g, pr = float(np.broadcast_to(np.asarray(ground, np.float64), (B,))[b]), prims[b]
        out.append(render_one(chains, joints[b], lens[b], pr, tracks[b], H, W, camera, style, g, ft, frames, wrong, keys_out))
    return np.stack(out)


def margins(keys):
    """From ``keys_out``: (the smallest gap between consecutive depth keys of a frame, the smallest |e_axis - h_axis| of a
    box), in metres; inf where there is nothing to compare."""
    gap = min([b - a for ks, _ in keys for a, b in zip(ks[:-1], ks[1:])] + [np.inf])
    face = min([m for _, ms in keys for m in ms] + [np.inf])
    return gap, face


# ---- the worlds ------------------------------------------------------------------------------------------------------

def placed(sk, n, seed, x=0.0, z=0.0, scale=1.0):
    """A walking character of n frames moved to (x, z): (n, J, 3) fp32."""
    return (RR.walk(sk, n, seed, scale) + np.array([x, 0.0, z], np.float32)).astype(np.float32)


def world(clips, T=None, fill=0.0):
    """[[(n_i, J, 3)] per world] -> (joints (B, C, T, J, 3) fp32 padded with ``fill``, lens (B, C)); a world with fewer
    characters gets absent ones."""
    Cn = max(len(w) for w in clips)
    T = T or max(len(c) for w in clips for c in w)
    J = clips[0][0].shape[1]
    out = np.full((len(clips), Cn, T, J, 3), fill, np.float32)
    lens = np.zeros((len(clips), Cn), np.int64)
    for b, w in enumerate(clips):
        for c, clip in enumerate(w):
            out[b, c, :len(clip)] = clip
            lens[b, c] = len(clip)
    return out, lens


def skel(name):
    """The reference skeleton of the feature tests, from the package's tables."""
    import motion_features_ref as MR
    sk = pkg("motion_features").SKELETONS[name]
    return MR.skeleton_from_tables(sk.chains, sk.raw_offsets, sk.face, sk.feet, sk.legs)


def camera_dict(cam):
    """A ``motion_render.Camera`` as the dict the restatement takes."""
    return dict(elev=cam.elev, azim=cam.azim, dist=cam.dist, fov=cam.fov, target=tuple(cam.target), near=cam.near)


def static_scene():
    """One of each kind: ``floor()``, a sphere, a leaning capsule, a yawed box and a wall half-space behind them."""
    MS = pkg("motion_scene")
    return [MS.floor(0.0), MS.sphere((1.2, 0.4, 0.3), 0.4), MS.capsule((-1.3, 0.0, 0.6), (-1.3, 1.6, 0.9), 0.15),
            MS.box((0.3, 0.45, -1.2), (0.6, 0.45, 0.35), yaw=0.5), MS.half_space((0.0, 0.0, 1.0), -2.2)]


def static_world(name):
    """The parity batch: (skeleton, joints (2, 2, 5, J, 3), lens [[5, 3], [2, 0]], prims (2, 5, 12)): one character ends early,
    one is absent."""
    sk = skel(name)
    j, lens = world([[placed(sk, 5, 1, -0.4, 0.8), placed(sk, 3, 2, 0.7, -0.3)], [placed(sk, 2, 3, 0.2, 0.1)]], T=5)
    prims = pkg("motion_scene").batch_scene(static_scene(), 2).numpy()
    return sk, j, lens, prims


def track_world(sk, T=5):
    """One character among moving things: (joints (1, 1, T, J, 3), lens [[T]], tracks (1, T, 11, 12)): a sphere that crosses, a
    box whose yaw changes with the frame, a sphere that is inactive in frames 1 and 3, and a second character's spine and
    legs as eight capsule tracks of ``character_tracks``."""
    MS = pkg("motion_scene")
    t = np.arange(T, dtype=np.float64)
    j, lens = world([[placed(sk, T, 1, 0.0, 0.5)]])
    on = np.ones(T, bool)
    on[[1, 3]] = False
    tracks = [MS.moving_sphere(np.stack([-1.0 + 0.5 * t, 0.4 + 0 * t, -0.5 + 0 * t], 1), 0.3),
              MS.moving_box(np.stack([0.8 + 0.1 * t, 0.3 + 0 * t, 0.6 + 0 * t], 1), (0.3, 0.3, 0.2), yaw=0.3 * t + 0.2),
              MS.moving_sphere(np.stack([-0.9 + 0 * t, 0.9 + 0 * t, 0.3 + 0 * t], 1), 0.25, active=on)]
    tracks += MS.character_tracks(placed(sk, T, 2, -0.5, -1.0), radius=0.05, bones=TRACK_BONES)
    return j, lens, MS.batch_tracks(tracks, 1, T).numpy()


# spine and legs: with all 21 bones some two of a frame's 29 depth keys lie within a millimetre at any camera
TRACK_BONES = [(0, 3), (3, 6), (6, 9), (9, 12), (0, 1), (1, 4), (0, 2), (2, 5)]


def order_world(sk, T=5):
    """Two characters in one pose on the camera's axis who swap which one is nearer between frames 1 and 3, and a thin box
    between them: (joints (1, 2, T, J, 3), lens, prims (1, 1, 12))."""
    pose = RR.walk(sk, 1, 1)[0]
    pose = pose - pose[0] * np.array([1, 0, 1], np.float32)
    z = np.array([1.0, 1.0, 1.0, -1.0, -1.0])[:T]
    a = np.stack([pose + np.array([0, 0, v], np.float32) for v in z])
    b = np.stack([pose + np.array([0, 0, -v], np.float32) for v in z])
    j, lens = world([[a.astype(np.float32), b.astype(np.float32)]])
    MS = pkg("motion_scene")
    return j, lens, MS.batch_scene([MS.box((0.0, 0.5, 0.0), (0.6, 0.5, 0.1))], 1).numpy()

"""CPU restatement of the motion preview's image (TEST INFRASTRUCTURE ONLY), and the clips it is tested on.

The image is defined by DESIGN.md §21, not by matplotlib: this is that definition in numpy, written from it.  ``ft=np.float64``
is the truth; ``ft=np.float32`` is the same arithmetic with every step in fp32 (the trigonometry of the camera included).  The
input joints are fp32 in both forms.  The device is held to the fp64 form within one grey level on every pixel: coverage and
compositing are continuous in the projected coordinates, so the only difference that fp32 coordinates (good to about 1e-3
pixel) can make is a rounding flip at floor(255 c + 0.5).

``WRONG`` names the mistakes an implementation most easily makes; ``wrong=name`` makes one of them.
"""
from __future__ import annotations

import numpy as np

import foot_skate_ref as FS

CAMERA = dict(elev=30.0, azim=0.0, dist=5.0, fov=40.0, target=(0.0, 0.9, 0.0), near=0.1)
RED, BLUE, BLACK = (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, 0.0)
STYLE = dict(background=(1.0, 1.0, 1.0), floor_color=(0.5, 0.5, 0.5), floor_alpha=0.5, trajectory_color=BLUE,
             trajectory_alpha=1.0, trajectory_width=1.0, chain_colors=(RED, BLUE, BLACK, RED, BLUE), chain_alpha=1.0,
             chain_width=4.0)

WRONG = ("height_kept",       # MINS.y is not subtracted
         "traj_absolute",     # the trajectory is not made relative to the current root
         "traj_at_1",         # the trajectory is drawn at t = 1 (one point: a disc)
         "traj_through_t",    # the trajectory runs through frame t itself
         "floor_unclipped",   # the floor's corners are projected without the near plane
         "chains_reversed",   # the chains are composited last to first
         "mirror_x",          # the image's x grows against the camera's right
         "flip_y",            # the image's y grows with the camera's up
         "integer_centres",   # pixel centres at (i, j)
         "width_pixels",      # a width in points is taken as the full width in pixels
         "padding_in_extent")  # frames past the length enter MINS / MAXS


def camera_basis(cam, ft):
    """-> (eye, r, u, f) of the look-at camera in ``ft``."""
    cam = dict(CAMERA, **(cam or {}))
    e, a = np.deg2rad(ft(cam["elev"])), np.deg2rad(ft(cam["azim"]))
    back = np.array([np.cos(e) * np.sin(a), np.sin(e), np.cos(e) * np.cos(a)], ft)
    target = np.asarray(cam["target"], ft)
    eye = target + ft(cam["dist"]) * back
    f = -back  # normalize(target - eye)
    r = np.cross(f, np.array([0, 1, 0], ft)).astype(ft)
    r = r / np.sqrt((r * r).sum())
    return eye, r, np.cross(r, f).astype(ft), f


def _clip_segment(p, q, near):
    """A view-space segment against z = near: -> (p, q), or None where it lies behind."""
    if p[2] < near and q[2] < near:
        return None
    if p[2] < near:
        p = p + (near - p[2]) / (q[2] - p[2]) * (q - p)
    elif q[2] < near:
        q = q + (near - q[2]) / (p[2] - q[2]) * (p - q)
    return p, q


def _clip_polygon(v, near):
    """Sutherland-Hodgman of a view-space polygon (m, 3) against z >= near."""
    out = []
    for i in range(len(v)):
        p, q = v[i], v[(i + 1) % len(v)]
        if p[2] >= near:
            out.append(p)
        if (p[2] >= near) != (q[2] >= near):
            a, b = (q, p) if p[2] >= near else (p, q)  # a behind
            out.append(a + (near - a[2]) / (b[2] - a[2]) * (b - a))
    return out


def capsule(a, b, w, X, Y, ft):
    """Coverage of the capsule of half-width w between pixels a and b at the pixel centres (X, Y)."""
    ex, ey = b[0] - a[0], b[1] - a[1]
    l2 = max(ex * ex + ey * ey, ft(1e-12))
    dx, dy = X - a[0], Y - a[1]
    t = np.clip((dx * ex + dy * ey) / l2, ft(0), ft(1))
    qx, qy = dx - t * ex, dy - t * ey
    return np.clip(ft(0.5) + w - np.sqrt(qx * qx + qy * qy), ft(0), ft(1))


def polygon(pts, X, Y, ft):
    """Coverage of a convex polygon of pixel corners: clamp(0.5 + the smallest signed distance to its edge lines)."""
    m = len(pts)
    if m < 3:
        return None
    area = sum(pts[i][0] * pts[(i + 1) % m][1] - pts[(i + 1) % m][0] * pts[i][1] for i in range(m))
    if area == 0:
        return None
    sign = ft(1) if area > 0 else ft(-1)
    s = None
    for i in range(m):
        a, b = pts[i], pts[(i + 1) % m]
        ex, ey = b[0] - a[0], b[1] - a[1]
        n = np.sqrt(ex * ex + ey * ey)
        if not n > 0:
            continue
        d = sign * (ex * (Y - a[1]) - ey * (X - a[0])) / n
        s = d if s is None else np.minimum(s, d)
    return None if s is None else np.clip(ft(0.5) + s, ft(0), ft(1))


def _over(c, cov, colour, alpha, ft):
    k = (ft(alpha) * cov)[..., None]
    return c * (ft(1) - k) + np.asarray(colour, ft) * k


def render_clip(chains, clip, n, H, W, camera=None, style=None, ft=np.float64, frames=None, wrong=None):
    """One sample: clip (T, J, 3) fp32 of which the first n frames are valid -> (len(frames), H, W, 3) uint8 (frames: indices,
    default all T); a frame at or past n is zero."""
    st = dict(STYLE, **(style or {}))
    cam = dict(CAMERA, **(camera or {}))
    T = len(clip)
    frames = list(range(T)) if frames is None else list(frames)
    out = np.zeros((len(frames), H, W, 3), np.uint8)
    if n < 1:
        return out
    p = np.asarray(clip, np.float32)[:n].astype(ft)
    seen = np.asarray(clip, np.float32).astype(ft) if wrong == "padding_in_extent" else p
    mins, maxs = seen.reshape(-1, 3).min(0), seen.reshape(-1, 3).max(0)
    p = p.copy()
    if wrong != "height_kept":
        p[..., 1] -= mins[1]
    traj = p[:, 0, [0, 2]].copy()
    eye, r, u, f = camera_basis(cam, ft)
    near = ft(cam["near"])
    F = ft(H) / ft(2) / np.tan(np.deg2rad(ft(cam["fov"])) / ft(2))
    half = (lambda pts: ft(pts) / ft(2)) if wrong == "width_pixels" else (lambda pts: ft(pts) * ft(H) / ft(1440))
    off = ft(0) if wrong == "integer_centres" else ft(0.5)
    X, Y = np.meshgrid(np.arange(W).astype(ft) + off, np.arange(H).astype(ft) + off)
    sx, sy = (ft(-1) if wrong == "mirror_x" else ft(1)), (ft(1) if wrong == "flip_y" else ft(-1))

    def view(q):
        d = np.asarray(q, ft) - eye
        return np.array([(r * d).sum(), (u * d).sum(), (f * d).sum()], ft)

    def pixel(v):
        return (ft(W) / ft(2) + sx * F * v[0] / v[2], ft(H) / ft(2) + sy * F * v[1] / v[2])

    def group(segments, w):
        cov = np.zeros((H, W), ft)
        for a, b in segments:
            s = _clip_segment(view(a), view(b), near)
            if s is not None:
                cov = np.maximum(cov, capsule(pixel(s[0]), pixel(s[1]), w, X, Y, ft))
        return cov

    nchains = len(chains)
    widths = np.broadcast_to(np.asarray(st["chain_width"], np.float64), (nchains,))
    alphas = np.broadcast_to(np.asarray(st["chain_alpha"], np.float64), (nchains,))
    for k, t in enumerate(frames):
        if t < 0 or t >= n:
            continue
        c = np.empty((H, W, 3), ft)
        c[:] = np.asarray(st["background"], ft)
        root = traj[t]
        q = p[t].copy()
        q[:, 0] -= root[0]
        q[:, 2] -= root[1]
        x0, x1, z0, z1 = mins[0] - root[0], maxs[0] - root[0], mins[2] - root[1], maxs[2] - root[1]
        corners = [view((x0, 0, z0)), view((x1, 0, z0)), view((x1, 0, z1)), view((x0, 0, z1))]
        if wrong != "floor_unclipped":
            corners = _clip_polygon(corners, near)
        cov = polygon([pixel(v) for v in corners], X, Y, ft)
        if cov is not None:
            c = _over(c, cov, st["floor_color"], st["floor_alpha"], ft)
        rel = traj - (ft(0) if wrong == "traj_absolute" else root)
        last = t + 1 if wrong == "traj_through_t" else t  # points 0 .. last - 1
        if t > 1 or (wrong == "traj_at_1" and t == 1):
            pts = [(rel[s, 0], ft(0), rel[s, 1]) for s in range(last)]
            segs = list(zip(pts[:-1], pts[1:])) or [(pts[0], pts[0])]
            c = _over(c, group(segs, half(st["trajectory_width"])), st["trajectory_color"], st["trajectory_alpha"], ft)
        order = range(nchains - 1, -1, -1) if wrong == "chains_reversed" else range(nchains)
        for g in order:
            ch = chains[g]
            segs = [(q[a], q[b]) for a, b in zip(ch[:-1], ch[1:])]
            c = _over(c, group(segs, half(widths[g])), st["chain_colors"][g % len(st["chain_colors"])], alphas[g], ft)
        out[k] = np.floor(np.clip(ft(255) * c + ft(0.5), 0, 255)).astype(np.uint8)
    return out


def render(chains, joints, lengths, H, W, camera=None, style=None, ft=np.float64, frames=None, wrong=None):
    """Batch form of the device function: joints (B, T, J, 3) fp32 -> (B, NF, H, W, 3) uint8."""
    joints = np.asarray(joints, np.float32)
    lengths = [joints.shape[1]] * len(joints) if lengths is None else [int(n) for n in lengths]
    return np.stack([render_clip(chains, joints[b], n, H, W, camera, style, ft, frames, wrong) for b, n in enumerate(lengths)])


def palette_index(rgb):
    """The 6 x 7 x 6 cube's index of 8-bit colours (..., 3), in integers."""
    v = np.asarray(rgb).astype(np.int64)
    return (((v[..., 0] * 5 + 127) // 255) * 42 + ((v[..., 1] * 6 + 127) // 255) * 6 + (v[..., 2] * 5 + 127) // 255).astype(np.uint8)


def moved(a, b, levels=64):
    """Pixels at which two images differ by at least ``levels`` grey levels in some channel."""
    return int((np.abs(a.astype(np.int32) - b.astype(np.int32)).max(-1) >= levels).sum())


# ---- the clips -------------------------------------------------------------------------------------------------------

def walk(sk, n, seed=1, scale=1.0):
    """The walking skeleton of foot_skate_ref: (n, J, 3) fp32."""
    return FS.walk_clip(sk, n, seed, scale=scale, blends=())[0]


def far_clip(sk, n=24, scale=1.0):
    """A walk carried 40 m away from the camera's side: the floor, and the trajectory behind the figure, pass behind the
    default camera."""
    w = walk(sk, n, 2, scale).astype(np.float64)
    own = w[-1, 0] - w[0, 0]
    step = (np.array([0.3, 0.0, -0.954]) * 40.0 * scale - own * (1.0, 0.0, 1.0)) / (n - 1)  # the root ends 40 m from its start
    return (w + np.arange(n)[:, None, None] * step).astype(np.float32)


def coincident_clip(sk, n=6):
    """Two joints in one place: the last joint of chain 2 (the head) on the joint before it, a bone without length."""
    j = walk(sk, n, 3).copy()
    j[:, sk.chains[2][-1]] = j[:, sk.chains[2][-2]]
    return j


def pad(clips, T=None, fill=0.0):
    """[(n_i, J, 3)] -> (joints (B, T, J, 3) fp32 padded with ``fill``, lengths)."""
    T = T or max(len(c) for c in clips)
    out = np.full((len(clips), T) + clips[0].shape[1:], fill, np.float32)
    for b, c in enumerate(clips):
        out[b, :len(c)] = c
    return out, [len(c) for c in clips]

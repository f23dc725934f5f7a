"""Motion preview on the device: joints -> image frames, contact sheets and GIF files.

Host side of ``mdm_motion_render`` (csrc/motion_render.hip).  The scene is the one the reference's ``plot_3d_motion``
(utils/plot_script.py) prepares: a floor rectangle from the clip's extent, the root's trajectory up to the frame before, and the
skeleton's five kinematic chains in red, blue, black, red, blue, all relative to the frame's root.  The rasteriser is this
project's own and is defined in DESIGN.md §21 (a look-at pinhole camera, capsules with a one-pixel coverage ramp), not
matplotlib's: two implementations of that definition agree to a grey level.  All pixels are made in the kernel; no eager
fallback.

``render_world`` (``mdm_world_render`` in csrc/motion_world_render.hip) is the world view under the same
definition: up to four characters and the primitives and tracks of a ``motion_scene`` scene in world coordinates, composited
far to near per item; ``world_extent`` / ``fit_camera`` give the camera that shows all of it.

``render_mesh`` (``mdm_mesh_render`` in csrc/motion_mesh_render.hip) is the body view: the vertices of a skinned
mesh (``motion_mesh.skin_vertices``) as shaded triangles with a depth test per pixel, over §21's floor and trajectory.
"""
from __future__ import annotations

import ctypes as C
import io
from dataclasses import dataclass, replace
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib as L

RED, BLUE, BLACK = (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, 0.0)
STYLE = dict(background=(1.0, 1.0, 1.0),
             floor_color=(0.5, 0.5, 0.5), floor_alpha=0.5,
             trajectory_color=BLUE, trajectory_alpha=1.0, trajectory_width=1.0,
             chain_colors=(RED, BLUE, BLACK, RED, BLUE), chain_alpha=1.0, chain_width=4.0)  # widths: points of a 720-point figure
MAX_ELEV = 89.9


@dataclass(frozen=True)
class Camera:
    """Look-at pinhole camera: eye = target + dist (cos e sin a, sin e, cos e cos a), angles and ``fov`` (vertical) in degrees.
    The defaults look at the figure from its front and above, as the reference's axes do; they are a choice."""
    elev: float = 30.0
    azim: float = 0.0
    dist: float = 5.0
    fov: float = 40.0
    target: Tuple[float, float, float] = (0.0, 0.9, 0.0)
    near: float = 0.1

    def block(self):
        """The eight floats of ``mdm_motion_render``'s camera argument, checked."""
        v = [float(self.elev), float(self.azim), float(self.dist), float(self.fov)] + [float(x) for x in self.target] + [float(self.near)]
        if len(v) != 8 or not all(np.isfinite(v)):
            raise ValueError("camera values must be finite, target three of them")
        if abs(self.elev) >= MAX_ELEV:
            raise ValueError(f"|elev| must be below {MAX_ELEV} degrees (the camera's up is the world's)")
        if not (self.dist > 0 and 0 < self.near < self.dist and 0 < self.fov < 180):
            raise ValueError("camera needs dist > 0, 0 < near < dist and 0 < fov < 180")
        return (C.c_float * 8)(*v)


def as_camera(camera) -> Camera:
    if camera is None:
        return Camera()
    if isinstance(camera, Camera):
        return camera
    if isinstance(camera, dict):
        return replace(Camera(), **{k: (tuple(v) if k == "target" else v) for k, v in camera.items()})
    raise ValueError("camera must be a Camera, a dict of its fields, or None")


def _palette() -> np.ndarray:
    r, g, b = np.meshgrid(np.arange(6), np.arange(7), np.arange(6), indexing="ij")
    return np.stack([r * 51, (g * 255 + 3) // 6, b * 51], -1).reshape(252, 3).astype(np.uint8)


PALETTE = _palette()  # entry r6 42 + g7 6 + b6 of the 6 x 7 x 6 colour cube


def palette_index(rgb):
    """8-bit colours (..., 3), a tensor or an array -> the cube's index (...) uint8: ``r6 = (r8 5 + 127) // 255``,
    ``g7 = (g8 6 + 127) // 255``, ``b6 = (b8 5 + 127) // 255``, ``index = r6 42 + g7 6 + b6``, all in integers."""
    if torch.is_tensor(rgb):
        v = rgb.to(torch.int32)
        idx = (torch.div(v[..., 0] * 5 + 127, 255, rounding_mode="floor") * 42
               + torch.div(v[..., 1] * 6 + 127, 255, rounding_mode="floor") * 6 + torch.div(v[..., 2] * 5 + 127, 255, rounding_mode="floor"))
        return idx.to(torch.uint8)
    v = np.asarray(rgb).astype(np.int32)
    return (((v[..., 0] * 5 + 127) // 255) * 42 + ((v[..., 1] * 6 + 127) // 255) * 6 + (v[..., 2] * 5 + 127) // 255).astype(np.uint8)


def style_block(nchains: int, **style):
    """The floats of ``mdm_motion_render``'s style argument from the keyword arguments of ``render_motion`` (``STYLE`` holds
    the names and defaults): background, then colour, alpha and width of the floor, the trajectory and every chain.
    ``chain_alpha`` / ``chain_width``: one value or one per chain; ``chain_colors``: one colour per chain, repeated in turn
    where the skeleton has more chains."""
    unknown = set(style) - set(STYLE)
    if unknown:
        raise ValueError(f"unknown style arguments {sorted(unknown)}: the style is {sorted(STYLE)}")
    st = dict(STYLE, **style)

    def rgb(v, what):
        v = [float(x) for x in v]
        if len(v) != 3 or not all(0.0 <= x <= 1.0 for x in v):
            raise ValueError(f"{what} must be three values in [0, 1]")
        return v

    def per_chain(v, what):
        v = np.broadcast_to(np.asarray(v, np.float64), (nchains,)) if np.ndim(v) == 0 or len(v) == nchains else None
        if v is None or not np.isfinite(v).all() or (v < 0).any():
            raise ValueError(f"{what} must be one non-negative value, or one per chain ({nchains})")
        return [float(x) for x in v]

    colors = [rgb(c, "a chain colour") for c in st["chain_colors"]]
    if not colors:
        raise ValueError("chain_colors is empty")
    alphas, widths = per_chain(st["chain_alpha"], "chain_alpha"), per_chain(st["chain_width"], "chain_width")
    for name in ("floor_alpha", "trajectory_alpha", "trajectory_width"):
        if not (np.isfinite(st[name]) and st[name] >= 0):
            raise ValueError(f"{name} must be finite and >= 0")
    if max(alphas + [st["floor_alpha"], st["trajectory_alpha"]]) > 1:
        raise ValueError("an alpha must lie in [0, 1]")
    v = rgb(st["background"], "background")
    v += rgb(st["floor_color"], "floor_color") + [float(st["floor_alpha"]), 0.0]
    v += rgb(st["trajectory_color"], "trajectory_color") + [float(st["trajectory_alpha"]), float(st["trajectory_width"])]
    for c in range(nchains):
        v += colors[c % len(colors)] + [alphas[c], widths[c]]
    return (C.c_float * len(v))(*v)


def frame_indices(frames, T: int):
    """``frames`` of ``render_motion`` -> the list of frame indices: None (all), an int stride, a slice, or indices."""
    if frames is None:
        return None
    if isinstance(frames, slice):
        idx = list(range(T))[frames]
    elif isinstance(frames, (int, np.integer)):
        if frames < 1:
            raise ValueError("a frame stride must be >= 1")
        idx = list(range(0, T, int(frames)))
    else:
        idx = [int(i) for i in (frames.tolist() if hasattr(frames, "tolist") else frames)]
        idx = [i + T if i < 0 else i for i in idx]
    if not idx or min(idx) < 0 or max(idx) >= T:
        raise ValueError(f"frames must pick at least one frame inside [0, {T})")
    return idx


def _skeleton_for(skeleton, J):
    from .motion_features import get_skeleton
    if skeleton is None:
        if J not in (22, 21):
            raise ValueError(f"{J} joints: pass skeleton= (22 joints default to \"t2m\", 21 to \"kit\")")
        skeleton = {22: "t2m", 21: "kit"}[J]
    sk = get_skeleton(skeleton)
    if sk.joints != J:
        raise ValueError(f"the skeleton has {sk.joints} joints, the motion {J}")
    return sk


@torch.no_grad()
def render_motion(joints, lengths=None, skeleton=None, size=(480, 480), camera=None, palette=False, frames=None, **style):
    """joints (B, T, J, 3) on a GPU (or one clip (T, J, 3)) -> frames (B, T, H, W, 3) uint8 on the device, ``size`` = (H, W),
    W a multiple of 4; with ``palette=True`` (B, T, H, W) uint8 indices into ``PALETTE`` (the same picture: ``palette_index``
    of the RGB frames, a third of the bytes, ready for a GIF).  Frames at or past ``lengths[b]`` are zero and are never read.
    ``skeleton`` defaults by J (22: "t2m", 21: "kit").  ``camera``: a ``Camera`` or a dict of its fields.  ``frames``: a
    slice, an int stride or a list of frame indices: only those frames are drawn (the output's T is their count) while the
    scene's extent and the trajectory still come from all frames, which keeps a long motion's output small.  ``**style``:
    colours in [0, 1], alphas and widths in points, see ``STYLE``."""
    from .motion_features import _skeleton_struct
    x = torch.as_tensor(joints)
    if x.dim() == 3:
        x = x[None]
    if x.dim() != 4 or x.shape[-1] != 3:
        raise ValueError(f"joints of shape {tuple(x.shape)} must be (B, T, J, 3)")
    B, T, J = x.shape[:3]
    if T < 1:
        raise ValueError("a motion needs at least one frame")
    sk = _skeleton_for(skeleton, J)
    H, W = (int(v) for v in size)
    if H < 4 or W < 4 or W % 4:
        raise ValueError(f"size (H, W) = {(H, W)}: both at least 4 and W a multiple of 4 (a thread stores 4 pixels)")
    if lengths is not None:
        lengths = torch.as_tensor(lengths).flatten().to(torch.int64).cpu()
        if lengths.numel() != B or (B and (int(lengths.min()) < 1 or int(lengths.max()) > T)):
            raise ValueError(f"lengths must hold {B} entries in [1, {T}]")
    cam = as_camera(camera).block()
    st = style_block(len(sk.chains), **style)
    idx = frame_indices(frames, T)
    L.require_cuda(x)
    dev = x.device
    x = x.detach().to(torch.float32).contiguous()
    ln = None if lengths is None else lengths.to(dev, torch.int32).contiguous()
    fr = None if idx is None else torch.tensor(idx, dtype=torch.int32, device=dev)
    NF = T if idx is None else len(idx)
    if B > 65535 or NF > 65535:
        raise ValueError("at most 65535 samples and 65535 frames per call")
    out = torch.empty((B, NF, H, W) + (() if palette else (3,)), dtype=torch.uint8, device=dev)
    lib = L.lib()
    scratch = torch.empty(max(1, int(lib.mdm_motion_render_scratch_floats(B, T))), dtype=torch.float32, device=dev)
    s = _skeleton_struct(sk)
    with torch.cuda.device(dev):
        L.check(lib.mdm_motion_render(x.data_ptr(), L.ptr(ln), C.byref(s), B, T, J, H, W, cam, st, 1 if palette else 0, L.ptr(fr),
                                      NF, out.data_ptr(), scratch.data_ptr(), L.stream_ptr()), "mdm_motion_render")
    return out


def contact_sheet(frames_or_joints, cols: Optional[int] = None, every: int = 1, **render_kw):
    """Every ``every``-th frame of each sample side by side, ``cols`` to a row (default: all in one row): frames
    (B, T, H, W, 3) or palette indices (B, T, H, W) -> (B, rows H, cols W[, 3]); cells past the last frame are white.  A float
    tensor is taken as joints (B, T, J, 3) and rendered first with ``render_kw``.  Plain reshaping of ``render_motion``'s output."""
    x = torch.as_tensor(frames_or_joints)
    if x.dtype != torch.uint8:
        x = render_motion(x, frames=slice(None, None, every), **render_kw)
    else:
        if render_kw:
            raise ValueError("rendered frames take no rendering arguments")
        x = x[:, ::every]
    if x.dim() not in (4, 5) or every < 1:
        raise ValueError("frames must be (B, T, H, W, 3) or (B, T, H, W), every >= 1")
    B, n, H, W = x.shape[:4]
    cols = n if cols is None else int(cols)
    if cols < 1:
        raise ValueError("cols must be >= 1")
    rows = -(-n // cols)
    tail = tuple(x.shape[4:])
    white = 255 if tail else int(palette_index(np.array([255, 255, 255])))
    cells = torch.full((B, rows * cols, H, W) + tail, white, dtype=torch.uint8, device=x.device)
    cells[:, :n] = x
    cells = cells.reshape((B, rows, cols, H, W) + tail)
    order = (0, 1, 3, 2, 4) + ((5,) if tail else ())
    return cells.permute(*order).reshape((B, rows * H, cols * W) + tail)


def gif_duration_ms(fps: float) -> int:
    """A GIF's frame delay is a whole number of centiseconds: ``10 round(100 / fps)`` ms, at least 10 (20 fps -> 50 ms,
    12.5 fps -> 80 ms, 30 fps -> 30 ms instead of 33.3)."""
    if not fps > 0:
        raise ValueError("fps must be > 0")
    return 10 * max(1, int(round(100.0 / float(fps))))


def write_gif(indices, path, fps: float, lengths=None):
    """Palette frames -> an animated GIF that loops.  indices: (T, H, W) uint8 of one clip with ``path`` a file name or a
    binary file object, or (B, T, H, W) with one path per clip; ``lengths``: frames to write of each clip (default all).
    The frames go to PIL in its "P" mode with ``PALETTE``: nothing is quantised on the host.  The frame delay is rounded to
    whole centiseconds (``gif_duration_ms``).  PIL stores a frame that repeats the one before as a longer delay of that one.
    Returns ``path``."""
    try:
        from PIL import Image
    except ImportError as e:
        raise ImportError("write_gif needs PIL (the pillow package), which is not installed; the frames themselves, "
                          "render_motion(..., palette=True) and PALETTE, need nothing") from e
    x = indices.detach().cpu().numpy() if torch.is_tensor(indices) else np.asarray(indices)
    if x.dtype != np.uint8 or x.ndim not in (3, 4):
        raise ValueError("indices must be uint8 palette frames (T, H, W) or (B, T, H, W): render_motion(..., palette=True)")
    if x.ndim == 4:
        if isinstance(path, (str, bytes)) or len(path) != len(x):
            raise ValueError(f"a batch of {len(x)} clips needs as many paths")
        ns = [x.shape[1]] * len(x) if lengths is None else [int(n) for n in torch.as_tensor(lengths).flatten().tolist()]
        if len(ns) != len(x):
            raise ValueError(f"lengths must hold {len(x)} entries")
        return [write_gif(x[b], path[b], fps, ns[b]) for b in range(len(x))]
    n = x.shape[0] if lengths is None else int(torch.as_tensor(lengths).flatten()[0])
    if n < 1 or n > x.shape[0]:
        raise ValueError(f"{n} frames of a clip of {x.shape[0]}")
    if int(x[:n].max()) >= len(PALETTE):
        raise ValueError("an index outside the palette")
    pal = PALETTE.tobytes() + bytes(3 * (256 - len(PALETTE)))
    ims = []
    for t in range(n):
        im = Image.fromarray(x[t], "P")
        im.putpalette(pal)
        ims.append(im)
    ims[0].save(path, format="GIF", save_all=True, append_images=ims[1:], duration=gif_duration_ms(fps), loop=0, optimize=False)
    return path


def gif_bytes(indices, fps: float, length=None) -> bytes:
    """``write_gif`` of one clip into memory."""
    buf = io.BytesIO()
    write_gif(indices, buf, fps, length)
    return buf.getvalue()


# ---- the world view: several characters and the primitives of a scene, in world coordinates ----------------
MAX_CHARACTERS = 4
GREEN, ORANGE, PURPLE, TEAL, BROWN, OLIVE = (0.0, 0.55, 0.0), (1.0, 0.55, 0.0), (0.55, 0.0, 0.7), (0.0, 0.6, 0.6), (0.55, 0.3, 0.1), (0.5, 0.5, 0.0)
WORLD_STYLE = dict(background=(1.0, 1.0, 1.0),
                   floor_color=(0.5, 0.5, 0.5), floor_alpha=0.5,
                   trajectory_colors=(BLUE, GREEN, PURPLE, BROWN), trajectory_alpha=1.0, trajectory_width=1.0,
                   character_colors=((RED, BLUE, BLACK, RED, BLUE), (GREEN, ORANGE, BLACK, GREEN, ORANGE),
                                     (PURPLE, TEAL, BLACK, PURPLE, TEAL), (BROWN, OLIVE, BLACK, BROWN, OLIVE)),
                   chain_alpha=1.0, chain_width=4.0,
                   solid_color=(0.55, 0.6, 0.7), solid_alpha=0.9, edge_color=(0.15, 0.15, 0.2), edge_width=1.5,
                   shade=(1.0, 0.8, 0.62))  # a box's top and bottom, its local-x sides, its local-z sides; choices, all of them


def world_style_block(C_: int, nchains: int, **style):
    """The floats of ``mdm_world_render``'s style argument from the keyword arguments of ``render_world`` (``WORLD_STYLE`` holds
    the names and defaults): background; floor colour and alpha; ``solid_color`` / ``solid_alpha`` of the primitives;
    ``edge_color`` / ``edge_width`` of a box's edges; ``shade``; then per character the colour, alpha and width of its
    trajectory and of every chain.  ``trajectory_alpha`` / ``trajectory_width``: one value or one per character;
    ``chain_alpha`` / ``chain_width``: anything that broadcasts to (characters, chains); ``trajectory_colors``: one colour per
    character, ``character_colors``: one list of chain colours per character, both repeated in turn where there are more."""
    unknown = set(style) - set(WORLD_STYLE)
    if unknown:
        raise ValueError(f"unknown style arguments {sorted(unknown)}: the style is {sorted(WORLD_STYLE)}")
    st = dict(WORLD_STYLE, **style)

    def rgb(v, what):
        v = [float(x) for x in v]
        if len(v) != 3 or not all(0.0 <= x <= 1.0 for x in v):
            raise ValueError(f"{what} must be three values in [0, 1]")
        return v

    def spread(v, shape, what, most=None):
        try:
            a = np.broadcast_to(np.asarray(v, np.float64), shape)
        except ValueError:
            raise ValueError(f"{what} must broadcast to {shape}") from None
        if not np.isfinite(a).all() or (a < 0).any() or (most is not None and (a > most).any()):
            raise ValueError(f"{what} must be finite and >= 0" + (f", at most {most}" if most is not None else ""))
        return a

    traj_colors = [rgb(c, "a trajectory colour") for c in st["trajectory_colors"]]
    sets = [[rgb(c, "a chain colour") for c in s] for s in st["character_colors"]]
    if not traj_colors or not sets or not all(sets):
        raise ValueError("trajectory_colors and character_colors must not be empty")
    ta, tw = spread(st["trajectory_alpha"], (C_,), "trajectory_alpha", 1.0), spread(st["trajectory_width"], (C_,), "trajectory_width")
    ca, cw = spread(st["chain_alpha"], (C_, nchains), "chain_alpha", 1.0), spread(st["chain_width"], (C_, nchains), "chain_width")
    v = rgb(st["background"], "background")
    v += rgb(st["floor_color"], "floor_color") + [float(spread(st["floor_alpha"], (), "floor_alpha", 1.0))]
    v += rgb(st["solid_color"], "solid_color") + [float(spread(st["solid_alpha"], (), "solid_alpha", 1.0))]
    v += rgb(st["edge_color"], "edge_color") + [float(spread(st["edge_width"], (), "edge_width"))]
    v += [float(x) for x in spread(st["shade"], (3,), "shade", 1.0)]
    for c in range(C_):
        v += traj_colors[c % len(traj_colors)] + [float(ta[c]), float(tw[c])]
        colors = sets[c % len(sets)]
        for g in range(nchains):
            v += colors[g % len(colors)] + [float(ca[c, g]), float(cw[c, g])]
    return (C.c_float * len(v))(*v)


def pack_world(characters, lengths=None):
    """The characters of B worlds as ``(joints (B, C, T, J, 3) float32, lengths (B, C) int64 on the CPU)``.  ``characters``:
    a tensor (B, C, T, J, 3) with ``lengths`` (B, C) in [0, T] (None: all T), or a list of worlds, each a list of (n_i, J, 3)
    joint clips in world coordinates, which is what ``DDPMTrainer.generate_together`` returns: padded with zeros to the
    longest clip, a world with fewer characters than another gets absent ones (length 0).  At most ``MAX_CHARACTERS``."""
    if isinstance(characters, (list, tuple)):
        if lengths is not None:
            raise ValueError("a list of worlds carries its own lengths")
        worlds = [[torch.as_tensor(c) for c in w] for w in characters]
        clips = [c for w in worlds for c in w]
        if not clips:
            raise ValueError("a world needs at least one character")
        if any(c.dim() != 3 or c.shape[-1] != 3 or c.shape[1] != clips[0].shape[1] for c in clips):
            raise ValueError("every character must be (n, J, 3) joints, with one J")
        Cn = max(len(w) for w in worlds)
        if Cn > MAX_CHARACTERS:
            raise ValueError(f"{Cn} characters in a world: the world view draws at most {MAX_CHARACTERS}")
        T = max(max(c.shape[0] for c in clips), 1)
        x = torch.zeros((len(worlds), Cn, T, clips[0].shape[1], 3), dtype=torch.float32, device=clips[0].device)
        ln = torch.zeros((len(worlds), Cn), dtype=torch.int64)
        for b, w in enumerate(worlds):
            for c, clip in enumerate(w):
                x[b, c, :clip.shape[0]] = clip.to(x.device, torch.float32)
                ln[b, c] = clip.shape[0]
        return x, ln
    x = torch.as_tensor(characters)
    if x.dim() != 5 or x.shape[-1] != 3:
        raise ValueError(f"characters of shape {tuple(x.shape)} must be (B, C, T, J, 3), or a list of worlds of (n, J, 3) clips")
    B, Cn, T = x.shape[:3]
    if not 1 <= Cn <= MAX_CHARACTERS:
        raise ValueError(f"{Cn} characters in a world: the world view draws 1 to {MAX_CHARACTERS}")
    if T < 1:
        raise ValueError("a motion needs at least one frame")
    if lengths is None:
        ln = torch.full((B, Cn), T, dtype=torch.int64)
    else:
        ln = torch.as_tensor(lengths).to(torch.int64).cpu()
        if tuple(ln.shape) != (B, Cn) or (ln.numel() and (int(ln.min()) < 0 or int(ln.max()) > T)):
            raise ValueError(f"lengths must be {(B, Cn)} entries in [0, {T}] (0: the character is absent)")
    return x.detach().to(torch.float32), ln


def world_ground(records):
    """The ground rule of ``render_world(ground=None)``: static records (B, K, 12) -> ``(ground (B,) float32, records)``.  A
    world's ground lies at the offset of its first keep-out half-space whose normal is exactly (0, 1, 0), the one
    ``motion_scene.floor`` makes, and that record becomes padding in the returned copy (it is the ground and is not drawn a
    second time); without one the ground is at 0."""
    rec = torch.as_tensor(records).detach().to("cpu", torch.float32).clone()
    ground = torch.zeros(rec.shape[0])
    for b in range(rec.shape[0]):
        for k in range(rec.shape[1]):
            q = rec[b, k]
            if q[0] == 4 and q[1] == 1 and q[4] == 0 and q[5] == 1 and q[6] == 0:
                ground[b] = q[7]
                rec[b, k] = 0.0
                break
    return ground, rec


def _world(characters, lengths, scene, tracks):
    """The device arguments both world calls share: joints, lengths (CPU and device), static and track records."""
    from . import motion_scene as MS
    x, ln = pack_world(characters, lengths)
    B, Cn, T, J = x.shape[:4]
    rec = None if scene is None else MS.batch_scene(scene, B)
    trk = None if tracks is None else MS.batch_tracks(tracks, B, T, ln.max(dim=1).values if B else None)
    L.require_cuda(x)
    return dict(x=x.contiguous(), ln=ln, ln_dev=ln.to(x.device, torch.int32).contiguous(), rec=rec, trk=trk, B=B, C=Cn, T=T, J=J)


def _records(a):
    dev = a["x"].device
    rec = None if a["rec"] is None or a["rec"].shape[1] == 0 else a["rec"].to(dev).contiguous()
    trk = None if a["trk"] is None or a["trk"].shape[2] == 0 else a["trk"].to(dev).contiguous()
    return rec, (0 if rec is None else rec.shape[1]), trk, (0 if trk is None else trk.shape[2])


def _extent(a, rec, K, trk, Km):
    out = torch.empty((a["B"], 6), dtype=torch.float32, device=a["x"].device)
    with torch.cuda.device(a["x"].device):
        L.check(L.lib().mdm_world_extent(a["x"].data_ptr(), a["ln_dev"].data_ptr(), L.ptr(rec), K, L.ptr(trk), Km, a["B"], a["C"],
                                         a["T"], a["J"], out.data_ptr(), L.stream_ptr()), "mdm_world_extent")
    return out


@torch.no_grad()
def world_extent(characters, lengths=None, scene=None, tracks=None):
    """The extent of B worlds on the device: (B, 6) float32, per-axis minimum then maximum over the valid frames
    of every character, the boxes around the static spheres, capsules and boxes of ``scene`` and around the same kinds among
    the live records of ``tracks`` in frames below the world's length.  Arguments as ``render_world``."""
    a = _world(characters, lengths, scene, tracks)
    return _extent(a, *_records(a))


def fit_camera(extent, elev=30.0, azim=0.0, fov=40.0, size=(480, 480)) -> Camera:
    """A ``Camera`` that shows all of ``extent`` ((6,) or (B, 6): the union of the rows that are finite): its target is the
    extent's centre, and its distance puts the sphere around the extent's box inside the frame of ``size`` = (H, W) at the
    vertical field of view ``fov``.  A tensor on the device is copied to the host, once."""
    e = (extent.detach().cpu().numpy() if torch.is_tensor(extent) else np.asarray(extent)).astype(np.float64).reshape(-1, 6)
    e = e[np.isfinite(e).all(1)]
    if not len(e):
        return Camera(elev=float(elev), azim=float(azim), fov=float(fov))
    lo, hi = e[:, :3].min(0), e[:, 3:].max(0)
    H, W = (float(v) for v in size)
    half = np.deg2rad(float(fov)) / 2.0
    half = min(half, np.arctan(np.tan(half) * W / H))  # the narrower of the frame's two half angles
    radius = max(0.5 * float(np.linalg.norm(hi - lo)), 1e-3)
    dist = radius / np.sin(half)
    return Camera(elev=float(elev), azim=float(azim), dist=float(dist), fov=float(fov), target=tuple(float(v) for v in 0.5 * (lo + hi)),
                  near=float(min(0.1, 0.5 * (dist - radius) if dist - radius > 0 else 0.5 * dist)))


@torch.no_grad()
def render_world(characters, lengths=None, scene=None, tracks=None, skeleton=None, size=(480, 480), camera=None, palette=False,
                 frames=None, ground=None, **style):
    """The world view: every character and every primitive of B worlds in one picture per frame, in world
    coordinates -> (B, T, H, W, 3) uint8 on the device, or (B, T, H, W) palette indices.  ``characters`` / ``lengths``: as
    ``pack_world`` takes them, e.g. what ``generate_together`` returns; a character is not drawn at or past its own length, and
    frames at or past the longest character's are zero.  ``scene`` / ``tracks``: ``motion_scene`` primitives / track stacks,
    one list for all worlds or one per world, or packed records, through ``motion_scene.batch_scene`` / ``batch_tracks``
    (their limits apply); margins and weights do not change the picture.  ``ground``: the height of the ground rectangle, one
    value or one per world; None: ``world_ground``'s rule (the scene's ``floor()``, else 0).  ``camera``: a ``Camera`` or a
    dict of its fields; None: ``fit_camera`` of the union of the batch's extents, one camera for all worlds, at the cost of
    one copy of (B, 6) floats to the host.  ``skeleton`` / ``size`` / ``palette`` / ``frames`` as in ``render_motion``;
    ``**style``: see ``WORLD_STYLE``.  Items are composited far to near, one depth per item (a painter's order)."""
    from .motion_features import _skeleton_struct
    a = _world(characters, lengths, scene, tracks)
    B, Cn, T, J = a["B"], a["C"], a["T"], a["J"]
    sk = _skeleton_for(skeleton, J)
    H, W = (int(v) for v in size)
    if H < 4 or W < 4 or W % 4:
        raise ValueError(f"size (H, W) = {(H, W)}: both at least 4 and W a multiple of 4 (a thread stores 4 pixels)")
    st = world_style_block(Cn, len(sk.chains), **style)
    idx = frame_indices(frames, T)
    dev = a["x"].device
    if ground is None:
        if a["rec"] is None:
            gr = torch.zeros(B)
        else:
            gr, a["rec"] = world_ground(a["rec"])
    else:
        gr = torch.as_tensor(ground, dtype=torch.float32).flatten()
        if gr.numel() not in (1, B) or not bool(torch.isfinite(gr).all()):
            raise ValueError(f"ground must be one finite height, or one per world ({B})")
        gr = gr.expand(B)
    rec, K, trk, Km = _records(a)
    if camera is None:
        camera = fit_camera(_extent(a, rec, K, trk, Km), size=(H, W))
    cam = as_camera(camera).block()
    gr = gr.to(dev, torch.float32).contiguous()
    fr = None if idx is None else torch.tensor(idx, dtype=torch.int32, device=dev)
    NF = T if idx is None else len(idx)
    if B > 65535 or NF > 65535:
        raise ValueError("at most 65535 worlds and 65535 frames per call")
    out = torch.empty((B, NF, H, W) + (() if palette else (3,)), dtype=torch.uint8, device=dev)
    lib = L.lib()
    scratch = torch.empty(max(1, int(lib.mdm_world_render_scratch_floats(B, Cn, T, NF, K, Km))), dtype=torch.float32, device=dev)
    s = _skeleton_struct(sk)
    with torch.cuda.device(dev):
        L.check(lib.mdm_world_render(a["x"].data_ptr(), a["ln_dev"].data_ptr(), C.byref(s), L.ptr(rec), K, L.ptr(trk), Km, B, Cn, T,
                                     J, H, W, cam, st, gr.data_ptr(), 1 if palette else 0, L.ptr(fr), NF, out.data_ptr(),
                                     scratch.data_ptr(), L.stream_ptr()), "mdm_world_render")
    return out


# ---- the body view: a mesh as shaded triangles with a depth test per pixel ----------------------------------
MESH_STYLE = dict(background=(1.0, 1.0, 1.0),
                  floor_color=(0.5, 0.5, 0.5), floor_alpha=0.5,
                  trajectory_color=BLUE, trajectory_alpha=1.0, trajectory_width=1.0,
                  body_color=(0.72, 0.76, 0.85), body_alpha=1.0, ambient=0.35,
                  light=(-0.4, 0.6, 0.7))  # the light: (right, up, towards the eye) of the camera; a look, not a measurement
MAX_SIDE = 8192  # of mdm_mesh_render: a face's pixel box is packed


def mesh_style_block(**style):
    """The 20 floats of ``mdm_mesh_render``'s style argument from the keyword arguments of ``render_mesh`` (``MESH_STYLE`` holds
    the names and defaults): background; floor colour and alpha; trajectory colour, alpha and width in points; ``body_color``
    and ``body_alpha``; ``ambient`` in [0, 1]; ``light``, a direction of any length > 0 fixed to the camera in its (right,
    up, towards the eye) coordinates."""
    unknown = set(style) - set(MESH_STYLE)
    if unknown:
        raise ValueError(f"unknown style arguments {sorted(unknown)}: the style is {sorted(MESH_STYLE)}")
    st = dict(MESH_STYLE, **style)

    def rgb(v, what):
        v = [float(x) for x in v]
        if len(v) != 3 or not all(0.0 <= x <= 1.0 for x in v):
            raise ValueError(f"{what} must be three values in [0, 1]")
        return v

    for name in ("floor_alpha", "trajectory_alpha", "body_alpha", "ambient"):
        if not (np.isfinite(st[name]) and 0 <= st[name] <= 1):
            raise ValueError(f"{name} must lie in [0, 1]")
    if not (np.isfinite(st["trajectory_width"]) and st["trajectory_width"] >= 0):
        raise ValueError("trajectory_width must be finite and >= 0")
    light = [float(x) for x in st["light"]]
    if len(light) != 3 or not all(np.isfinite(light)) or not sum(x * x for x in light) > 0:
        raise ValueError("light must be three finite values, not all zero")
    v = rgb(st["background"], "background")
    v += rgb(st["floor_color"], "floor_color") + [float(st["floor_alpha"])]
    v += rgb(st["trajectory_color"], "trajectory_color") + [float(st["trajectory_alpha"]), float(st["trajectory_width"])]
    v += rgb(st["body_color"], "body_color") + [float(st["body_alpha"]), float(st["ambient"])] + light
    return (C.c_float * len(v))(*v)


def check_mesh(vertices, faces, lengths, root, normals, size):
    """Argument checks of ``render_mesh`` that need no device: -> (vertices (B, T, V, 3), faces (F, 3) int32 on the CPU, lengths
    (B,) int64 on the CPU or None, root (B, T, 3), normals or None, (H, W)).  Raises ValueError."""
    x = torch.as_tensor(vertices)
    one = x.dim() == 3
    if one:
        x = x[None]
    if x.dim() != 4 or x.shape[-1] != 3 or not x.dtype.is_floating_point:
        raise ValueError(f"vertices of shape {tuple(x.shape)} must be floating point (B, T, V, 3)")
    B, T, V = x.shape[:3]
    if T < 1 or V < 1 or V > 1 << 24:
        raise ValueError("a mesh motion needs at least one frame, and 1 to 2^24 vertices")
    f = torch.as_tensor(faces)
    if f.dim() != 2 or f.shape[1] != 3 or f.dtype.is_floating_point or f.dtype == torch.bool or not 1 <= f.shape[0] <= 1 << 24:
        raise ValueError(f"faces of shape {tuple(f.shape)} and dtype {f.dtype} must be integer (F, 3), F in [1, 2^24]")
    r = torch.as_tensor(root)
    if one and r.dim() in (2, 3) and r.shape[0] == T:
        r = r[None]
    if r.dim() == 4:
        r = r[:, :, 0]  # joints: joint 0 is the root
    if tuple(r.shape) != (B, T, 3):
        raise ValueError(f"root of shape {tuple(torch.as_tensor(root).shape)} must be ({B}, {T}, 3), or joints ({B}, {T}, J, 3)")
    n = None
    if normals is not None:
        n = torch.as_tensor(normals)
        if one and n.dim() == 3:
            n = n[None]
        if tuple(n.shape) != tuple(x.shape):
            raise ValueError(f"normals of shape {tuple(n.shape)} must have the vertices' shape {tuple(x.shape)}")
    H, W = (int(v) for v in size)
    if H < 4 or W < 4 or W % 4 or H > MAX_SIDE or W > MAX_SIDE:
        raise ValueError(f"size (H, W) = {(H, W)}: both in [4, {MAX_SIDE}] and W a multiple of 4 (a thread stores 4 pixels)")
    if lengths is not None:
        lengths = torch.as_tensor(lengths).flatten().to(torch.int64).cpu()
        if lengths.numel() != B or (B and (int(lengths.min()) < 1 or int(lengths.max()) > T)):
            raise ValueError(f"lengths must hold {B} entries in [1, {T}]")
    return x, f, lengths, r, n, (H, W)


@torch.no_grad()
def render_mesh(vertices, faces, lengths=None, *, root, normals=None, size=(480, 480), camera=None, palette=False, frames=None,
                **style):
    """The body view: vertices (B, T, V, 3) on a GPU (or one clip (T, V, 3)), as ``motion_mesh.skin_vertices``
    returns them, and ``faces`` (F, 3) integers shared by the batch -> frames (B, T, H, W, 3) uint8 on the device, or
    (B, T, H, W) palette indices: the mesh as triangles with a depth test per pixel, over §21's floor and trajectory.  ``root``
    (B, T, 3), or joints (B, T, J, 3) of which joint 0 is taken: every frame's x, z are relative to it, and it draws the
    trajectory.  ``normals`` (B, T, V, 3): smooth shading from the interpolated vertex normals; None: flat shading from each
    face's own normal.  A face is drawn from both sides; a face with a non-finite vertex, an index outside [0, V) or a vertex
    in front of the near plane is not drawn (it is dropped, not clipped).  ``lengths`` / ``size`` / ``camera`` / ``palette`` /
    ``frames`` as in ``render_motion``: frames at or past a length are zero and are never read.  ``**style``: see
    ``MESH_STYLE``.  All pixels are made in the kernel; no eager fallback."""
    x, f, lengths, r, n, (H, W) = check_mesh(vertices, faces, lengths, root, normals, size)
    B, T, V = x.shape[:3]
    cam = as_camera(camera).block()
    st = mesh_style_block(**style)
    idx = frame_indices(frames, T)
    L.require_cuda(x, r, n)
    dev = x.device
    if r.device != dev or (n is not None and n.device != dev):
        raise ValueError("root and normals must be on the vertices' device")
    x = x.detach().to(torch.float32).contiguous()
    r = r.detach().to(torch.float32).contiguous()
    n = None if n is None else n.detach().to(torch.float32).contiguous()
    f = f.detach().to(dev, torch.int32).contiguous()
    ln = None if lengths is None else lengths.to(dev, torch.int32).contiguous()
    fr = None if idx is None else torch.tensor(idx, dtype=torch.int32, device=dev)
    NF = T if idx is None else len(idx)
    if B > 65535 or NF > 65535:
        raise ValueError("at most 65535 samples and 65535 frames per call")
    out = torch.empty((B, NF, H, W) + (() if palette else (3,)), dtype=torch.uint8, device=dev)
    lib = L.lib()
    words = int(lib.mdm_mesh_render_scratch_floats(B, T, NF, V, f.shape[0], int(n is not None)))
    scratch = torch.empty(max(4, words), dtype=torch.float32, device=dev)
    mode = (1 if palette else 0) | (2 if n is not None else 0)
    with torch.cuda.device(dev):
        L.check(lib.mdm_mesh_render(x.data_ptr(), L.ptr(n), f.data_ptr(), r.data_ptr(), L.ptr(ln), B, T, V, f.shape[0], H, W, cam, st,
                                    mode, L.ptr(fr), NF, out.data_ptr(), scratch.data_ptr(), L.stream_ptr()), "mdm_mesh_render")
    return out
